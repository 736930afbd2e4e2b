// host_rans.hpp — plain rANS 4x16 entropy chains on a host core (host_rans.cpp)
//
// The same streams, bytes and ok / failed verdicts as k_rans_dec's NX = 4
// bodies (rans_chain.hip dec4_*): an order-0 or order-1 chain of 4
// interleaved states over 16-bit words.  One chain is serial whoever runs it;
// a host core steps it several times faster than a GPU wave, and
// Decompressor::run_djs (rans_decompress.cpp) places the long ones here by
// the cost model of host_sched.hpp.  The encoder's bare chains (the states at
// every chunk, no output words) follow below: Compressor::stage_encode
// (rans_compress.cpp) places those the same way.  No HIP in this file or its
// .cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fqz5 {
struct EncSym;   // rans_format.hpp
namespace host {

// The stream's frequency tables as the planner parses them
// (Decompressor::DJ): F rows x 256 normalised to 2^bits per non-empty row.
// Order-0: one row, bits 12.  Order-1: one row per context of `alpha`
// (ascending, alpha[0] == 0), a row of zeros for a context that never
// occurs.
// decode_freq + normalise_freq_shift of an order-0 table at [p, end):
// *used = its bytes.
bool rans_parse_o0(const uint8_t *p, const uint8_t *end, std::vector<uint32_t> &F, uint32_t *used,
                   bool skip = false);
// decode_freq1 of an (uncompressed) order-1 table at [p, end) for 2^bits
// slots: *used = its bytes.
bool rans_parse_o1(const uint8_t *p, const uint8_t *end, int bits, std::vector<uint32_t> &F,
                   std::vector<uint8_t> &alpha, uint32_t *used);

// n symbols from `in` (the 4 states, then the words; in_len bytes to the
// stream's end) into out[0, n).  True = the GPU decoder's status 0: the
// chain consumed no more words than the stream has.  Reads stay inside
// [in, in + in_len), writes inside [out, out + n).
bool rans_dec_o0(const uint32_t *F, int bits, const uint8_t *in, size_t in_len, uint8_t *out,
                 size_t n);
// split_table: the stream's table takes the GPU decoder's split layout
// (kernels.h dec_table_mode == DEC_TAB_SPLIT), which differs from the others
// only in what a damaged stream decodes from a context without a row.
bool rans_dec_o1(const uint32_t *F, const uint8_t *alpha, size_t rows, int bits, bool split_table,
                 const uint8_t *in, size_t in_len, uint8_t *out, size_t n);

// One entropy stream (table, nx states, words; `len` bytes to the stream's
// end) decoded as the reference decodes a stream that runs out of words: a
// state below 2^15 stays as it is once fewer than two bytes are left
// (RansDecRenormSafe), and the decode goes on.  The planner's slow path for a
// chain the kernels report starved (status -1), and its check of a stream of
// n = 0 symbols, whose table and states the reference still reads.  False
// where the reference returns NULL: a short stream, a table it refuses, a
// state below 2^15.  A context without a row decodes symbol 0 from a zeroed
// row.  Reads stay inside [in, in + len), writes inside [out, out + n).
bool rans_dec_ref(const uint8_t *in, uint32_t len, uint8_t *out, uint32_t n, bool o1, int nx);

// A whole rans_compress_4x16 stream whose order byte has only the order-1
// and NOSZ bits set (a compressed order-1 table is decoded here too);
// out_cap is the size itself for a NOSZ stream.  0, or -1 for any other
// stream and for a damaged one.
int rans_dec_stream(const uint8_t *in, size_t in_size, uint8_t *out, size_t out_cap,
                    size_t *out_size);

// ---- the encoder's bare chains ---------------------------------------------
// What k_enc_chain / k_enc_chain2w (rans_chain.hip) leave in EncJob::ck for an
// NX = 4 job, bit for bit: the four states before every chunk of 256 steps,
// from the top of the input down.  Words [0, 4) are RANS_LOW, the last four
// the final states; k_enc_replay emits the stream's words from them.  The step
// is chain_body_2w's: xr = x > xmax ? x >> 16 : x; q = mulhi(xr, rcp) >> sh;
// x = q * cmpl + xr + bias, without a branch.
//   Order-0: symbol i on state i & 3, ceil(n / 4) steps.
//   Order-1: state z codes in[z * (n/4) + k] in the context in[z * (n/4) + k - 1]
//   (0 at k = 0); state 3 also the tail, n - 3 * (n/4) steps in all.
// Reads stay inside [in, in + n) and the table, writes inside
// ck[0, rans_enc_ck_words(n, o1)).  n > 0.
size_t rans_enc_ck_words(size_t n, bool o1);
// syms: the 256 EncSym of the job (make_encsym over the normalised table)
void rans_enc_chain_o0(const EncSym *syms, const uint8_t *in, size_t n, uint32_t *ck);
// tab[A * A]: row = context, both by their index in the alphabet (remap)
void rans_enc_chain_o1(const EncSym *tab, const uint8_t *remap, int A, const uint8_t *in, size_t n,
                       uint32_t *ck);
// k_enc_tab on the host: the A x A normalised frequencies f1 (a row sums to
// 2^bits or 0) as encoder symbols, starts running in alphabet order
void rans_enc_tab_o1(const uint16_t *f1, int A, int bits, EncSym *tab);

}  // namespace host
}  // namespace fqz5
