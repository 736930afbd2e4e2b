// host_dec.hpp — the adaptive-model decode chains on host cores
// (host_dec.cpp); the plain rANS 4x16 decoders are in host_rans.hpp, the
// chains' placement in host_sched.hpp
#pragma once
#include <cstddef>
#include <cstdint>

namespace fqz5 {
namespace host {

// uncompress_block_fqz2f (fqzcomp_qual.c:1410-1634) of `in` into out (at
// most out_cap bytes; *out_size the decoded size).  lengths: the first
// nlengths record lengths out.  seq: per record its bases (the reference's
// s->seq[rec], nrec of them; nullptr: none).  Returns 0 or -1.
int fqz_decode(const uint8_t *in, size_t in_size, uint8_t *out, size_t out_cap, size_t *out_size,
               int *lengths, int nlengths, const uint8_t *const *seq, int nrec);

// decode_seq (fqzcomp5.c:1272-1406): n bases of records lens[nrec] with a
// k-mer context model (both: both strands update).  Returns 0 or -1.
int seq_decode(const uint8_t *in, uint32_t in_size, const uint32_t *lens, int nrec, int both, int k,
               uint8_t *out, uint32_t n);

}  // namespace host
}  // namespace fqz5
