// seq_match.hip — lookup by sequence content (fqz5file.find_seqs /
// extract_seqs_file): which records of a block's decoded bases contain one of
// a set of patterns as a contiguous substring.
//
// The patterns sit in an open-addressing table built on the host
// (fqz5_seqs_table_build), keyed by their first m bytes, the anchor: m is the
// shortest pattern's length, at most 12 (or what the caller forces).  The
// table, the hash and the probe are query_table.hpp's.  Unlike names, several
// patterns may share an anchor: they take separate slots of one probe, and a
// probe verifies every slot whose tag agrees up to the empty slot that ends it.
// k_seq_match hashes the m bytes at every position of the block's base array
// and probes; where a tag agrees it finds the record that owns the position,
// rejects a pattern that would run past that record's end and compares the
// pattern's bytes: tags never decide.  Per record the lowest pattern index
// that occurs is kept (atomicMin), per pattern a "seen somewhere" byte.  The
// hits are compacted as the name matcher's (nm_compact).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/fqz5_fastq.h"
#include "gpu_ctx.hpp"
#include "query_table.hpp"

namespace fqz5 {
GpuCtx &gpu();
void fqz5_set_error(const char *msg);
}  // namespace fqz5

struct fqz5_seq_table : fqz5::QueryTable {};    // (key_len: the anchor)

namespace fqz5 {
namespace {

constexpr uint32_t SM_TILE = 4096;              // bases per workgroup
constexpr uint32_t SM_THREADS = 256;
constexpr uint32_t SM_ANCHOR_MAX = 64;          // the staged tail (m - 1 bytes) is bounded by it
constexpr uint32_t SM_ANCHOR_DEFAULT = 12;
constexpr uint32_t SM_PATTERN_MAX = 65535;
constexpr uint64_t SM_QUERIES_MAX = 1ull << 20;
// the tile, the anchor's tail, and up to 15 bytes on either side from
// starting and ending the staging on 16-byte addresses
constexpr uint32_t SM_LDS = (SM_TILE + SM_ANCHOR_MAX + 32 + 15) / 16 * 16;

// the record that owns byte p: the first whose (inclusive) end lies past p,
// so of equal neighbours (zero-length records) never one of the empty ones
__host__ __device__ inline uint32_t owner(const uint64_t *end, uint32_t nrec, uint64_t p) {
    uint32_t lo = 0, hi = nrec;                 // (p < end[nrec - 1]: the answer is below nrec)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (end[mid] > p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// One workgroup per SM_TILE bases.  The tile and the m - 1 bytes after it
// are staged into LDS with 16-byte loads at 16-byte addresses (the section
// starts anywhere in its buffer, so the staged range may begin up to 15
// bytes before the tile; a chunk that is not wholly inside [0, seq_len) is
// read byte by byte).  Lane t then takes the positions tile0 + t + k * 256:
// neighbouring lanes read neighbouring LDS bytes, and global memory is
// touched again only where a tag agrees (the record search in end[], the
// byte compare against the section, hot in L2: a pattern may be far longer
// than a tile).
__global__ __launch_bounds__(SM_THREADS) void k_seq_match(const uint8_t *seq, uint64_t seq_len,
                                                          const uint64_t *end, uint32_t nrec,
                                                          QueryView T, uint32_t *hit,
                                                          uint8_t *seen) {
    __shared__ uint4 win4[SM_LDS / 16];
    const uint8_t *win = reinterpret_cast<const uint8_t *>(win4);
    const uint32_t m = T.key_len;
    const uint64_t t0 = uint64_t(blockIdx.x) * SM_TILE;
    const uint64_t tend = t0 + SM_TILE < seq_len ? t0 + SM_TILE : seq_len;   // positions end here
    const uint64_t send = tend + (m - 1) < seq_len ? tend + (m - 1) : seq_len;   // staging ends
    const int64_t w0 = aligned_start(seq, t0);
    for (uint32_t i = threadIdx.x; i < SM_LDS / 16; i += SM_THREADS) {
        const int64_t a = w0 + 16 * int64_t(i);
        if (a >= int64_t(send)) break;
        win4[i] = load16(seq, seq_len, a);
    }
    __syncthreads();
    for (uint64_t p = t0 + threadIdx.x; p < tend && p + m <= seq_len; p += SM_THREADS) {
        uint32_t rec = NM_NONE;
        nm_probe(T, nm_hash_of(win + (int64_t(p) - w0), m), [&](uint32_t qi) {
            if (rec == NM_NONE) rec = owner(end, nrec, p);
            const uint64_t qa = T.qoff[qi], len = T.len(qi);
            if (p + len > end[rec]) return false;
            uint64_t i = 0;
            while (i < len && seq[p + i] == T.q[qa + i]) i++;
            if (i != len) return false;
            atomicMin(&hit[rec], qi);
            if (seen) seen[qi] = 1;
            return false;                       // (on to the end of the probe)
        });
    }
}

}  // namespace
}  // namespace fqz5

using namespace fqz5;

extern "C" {

fqz5_seq_table *fqz5_seqs_table_build(const uint8_t *q, uint64_t q_len, uint64_t nq, int tag_bits,
                                      int anchor) {
    fqz5_seq_table *T = nullptr;
    try {
        if (tag_bits < 1 || tag_bits > 32) throw GpuError("seqs_table_build: tag_bits not in 1..32");
        if (!nq) throw GpuError("seqs_table_build: no pattern");
        if (nq > SM_QUERIES_MAX) throw GpuError("seqs_table_build: more than 2^20 patterns");
        if (anchor < 0 || uint32_t(anchor) > SM_ANCHOR_MAX)
            throw GpuError("seqs_table_build: anchor not in 0..64");
        T = new fqz5_seq_table();
        T->tag_bits = tag_bits;
        const uint64_t shortest = T->parse(q, q_len, nq, SM_PATTERN_MAX, "seqs_table_build",
                                           "pattern", "patterns");
        if (uint64_t(anchor) > shortest)
            throw GpuError("seqs_table_build: the anchor is longer than the shortest pattern");
        T->key_len = anchor ? uint32_t(anchor)
                            : uint32_t(std::min<uint64_t>(shortest, SM_ANCHOR_DEFAULT));
        T->fill("seqs_table_build", "pattern");
        return T;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        delete T;
        return nullptr;
    }
}

void fqz5_seqs_table_free(fqz5_seq_table *T) { delete T; }

uint32_t fqz5_seqs_table_anchor(const fqz5_seq_table *T) { return T ? T->key_len : 0; }

uint32_t fqz5_seqs_match_tile(void) { return SM_TILE; }

int fqz5_seqs_scan_host(const fqz5_seq_table *T, const uint8_t *seq, uint64_t seq_len,
                        const uint32_t *lens, uint64_t nrec, uint32_t *hit, uint8_t *seen) {
    try {
        if (!T) throw GpuError("seqs_scan_host: no table");
        check_records(nrec, 0, "seqs_scan_host");
        const std::vector<uint64_t> end = record_ends(lens, nrec, seq_len, "seqs_scan_host");
        for (uint64_t r = 0; r < nrec; r++) hit[r] = NM_NONE;
        const QueryView V = T->host();
        const uint32_t m = V.key_len, n = uint32_t(nrec);
        for (uint64_t p = 0; p + m <= seq_len; p++) {
            uint32_t rec = NM_NONE;
            nm_probe(V, nm_hash_of(seq + p, m), [&](uint32_t qi) {
                if (rec == NM_NONE) rec = owner(end.data(), n, p);
                const uint64_t len = V.len(qi);
                if (p + len > end[rec] || std::memcmp(seq + p, V.q + V.qoff[qi], size_t(len)))
                    return false;
                hit[rec] = std::min(hit[rec], qi);
                if (seen) seen[qi] |= 1;
                return false;
            });
        }
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

int fqz5_seqs_match(const fqz5_seq_table *T, const uint8_t *d_seq, uint64_t seq_len,
                    const uint32_t *h_len, uint64_t nrec, int pairs, uint32_t *d_rec,
                    uint32_t *d_query, uint64_t *n_hit, uint8_t *d_seen) {
    GpuCtx *gp = nullptr;
    try {
        *n_hit = 0;
        if (!T) throw GpuError("seqs_match: no table");
        check_records(nrec, 0, "seqs_match");
        const std::vector<uint64_t> end = record_ends(h_len, nrec, seq_len, "seqs_match");
        if (!nrec || seq_len < T->key_len) return 0;     // no position holds an anchor
        GpuCtx &g = gpu();
        gp = &g;
        const QueryView D = const_cast<fqz5_seq_table *>(T)->device_copy("seqs_match");
        const uint32_t n = uint32_t(nrec);
        const uint64_t *d_end = g.upload(end);
        uint32_t *hit = g.arena.alloc_n<uint32_t>(n);
        FQZ5_HIP(hipMemsetAsync(hit, 0xFF, size_t(n) * 4, g.stream));
        const uint64_t tiles = (seq_len + SM_TILE - 1) / SM_TILE;    // (seq_len < 2^32 * 2^31)
        if (tiles >= (1ull << 31)) throw GpuError("seqs_match: block too large");
        hipLaunchKernelGGL(k_seq_match, dim3(uint32_t(tiles)), dim3(SM_THREADS), 0, g.stream, d_seq,
                           seq_len, d_end, n, D, hit, d_seen);
        FQZ5_HIP(hipGetLastError());
        *n_hit = nm_compact(g, hit, n, pairs, d_rec, d_query);
        g.reset();
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { if (gp) gp->reset(); } catch (...) {}
        return -1;
    }
}

}  // extern "C"
