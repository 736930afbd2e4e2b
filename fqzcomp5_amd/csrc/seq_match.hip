// seq_match.hip — lookup by sequence content (fqz5file.find_seqs /
// extract_seqs_file): which records of a block's decoded bases contain one of
// a set of patterns as a contiguous substring.
//
// The patterns sit in an open-addressing table built on the host
// (fqz5_seqs_table_build), keyed by their first m bytes, the anchor: m is the
// shortest pattern's length, at most 12 (or what the caller forces).  The hash,
// the tag and the slot are name_match.hpp's.  Unlike names, several patterns
// may share an anchor: they take separate slots of one probe, and a probe
// verifies every slot whose tag agrees up to the empty slot that ends it.
// k_seq_match hashes the m bytes at every position of the block's base array
// and probes; where a tag agrees it finds the record that owns the position,
// rejects a pattern that would run past that record's end and compares the
// pattern's bytes: tags never decide.  Per record the lowest pattern index
// that occurs is kept (atomicMin), per pattern a "seen somewhere" byte.  The
// hits are compacted as the name matcher's (nm_compact).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <numeric>
#include <vector>

#include "../../include/fqz5_fastq.h"
#include "gpu_ctx.hpp"
#include "name_match.hpp"

namespace fqz5 {
GpuCtx &gpu();
void fqz5_set_error(const char *msg);
}  // namespace fqz5

// the patterns ('\0' after each), their offsets (nq + 1) and the slots; the
// device copies are made by the first fqz5_seqs_match and freed with the table
struct fqz5_seq_table {
    std::vector<uint8_t> q;
    std::vector<uint64_t> qoff;
    std::vector<uint64_t> slots;
    uint32_t mask = 0, anchor = 0;
    int tag_bits = 32;
    std::mutex m;
    int device = -1;
    uint8_t *d_q = nullptr;
    uint64_t *d_qoff = nullptr, *d_slots = nullptr;
};

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

struct SmDev {                                  // the table as the kernel reads it
    const uint64_t *slots;
    const uint8_t *q;
    const uint64_t *qoff;
    uint32_t mask, anchor;
    int tag_bits;
};

// the mixed hash of the m bytes at a
__host__ __device__ inline uint32_t anchor_hash(const uint8_t *a, uint32_t m) {
    uint32_t h = NM_HASH0;
    for (uint32_t i = 0; i < m; i++) h = nm_hash(h, a[i]);
    return nm_hash(h, 0, true);
}

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
                                                          SmDev T, uint32_t *hit, uint8_t *seen) {
    __shared__ uint4 win4[SM_LDS / 16];
    const uint8_t *win = reinterpret_cast<const uint8_t *>(win4);
    const uint32_t m = T.anchor;
    const uint64_t t0 = uint64_t(blockIdx.x) * SM_TILE;
    const uint64_t tend = t0 + SM_TILE < seq_len ? t0 + SM_TILE : seq_len;   // positions end here
    const uint64_t send = tend + (m - 1) < seq_len ? tend + (m - 1) : seq_len;   // staging ends
    const int64_t w0 = int64_t(t0) - int64_t((reinterpret_cast<uintptr_t>(seq) + t0) & 15u);
    for (uint32_t i = threadIdx.x; i < SM_LDS / 16; i += SM_THREADS) {
        const int64_t a = w0 + 16 * int64_t(i);
        if (a >= int64_t(send)) break;
        uint4 v;
        if (a >= 0 && uint64_t(a) + 16 <= seq_len) {
            v = *reinterpret_cast<const uint4 *>(seq + a);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (int k = 0; k < 16; k++)
                if (a + k >= 0 && uint64_t(a + k) < seq_len)
                    w[k >> 2] |= uint32_t(seq[a + k]) << (8 * (k & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        win4[i] = v;
    }
    __syncthreads();
    for (uint64_t p = t0 + threadIdx.x; p < tend && p + m <= seq_len; p += SM_THREADS) {
        const uint32_t mixed = anchor_hash(win + (int64_t(p) - w0), m);
        const uint32_t tag = nm_tag(mixed, T.tag_bits);
        uint32_t rec = NM_NONE;
        uint32_t sl = mixed & T.mask;
        for (uint32_t n = 0; n <= T.mask; n++, sl = (sl + 1) & T.mask) {
            const uint64_t ent = T.slots[sl];
            const uint32_t qi = uint32_t(ent >> 32);
            if (qi == NM_NONE) break;
            if (uint32_t(ent) != tag) continue;
            if (rec == NM_NONE) rec = owner(end, nrec, p);
            const uint64_t qa = T.qoff[qi];
            const uint64_t len = T.qoff[qi + 1] - 1 - qa;
            if (p + len > end[rec]) continue;
            uint64_t i = 0;
            while (i < len && seq[p + i] == T.q[qa + i]) i++;
            if (i != len) continue;
            atomicMin(&hit[rec], qi);
            if (seen) seen[qi] = 1;
        }
    }
}

// the table on the calling thread's device (made once)
SmDev device_copy(fqz5_seq_table &T) {
    std::lock_guard<std::mutex> lk(T.m);
    int dev = 0;
    FQZ5_HIP(hipGetDevice(&dev));
    if (!T.d_slots) {
        FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&T.d_q), T.q.size() + 1));
        FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&T.d_qoff), T.qoff.size() * 8));
        FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&T.d_slots), T.slots.size() * 8));
        FQZ5_HIP(hipMemcpy(T.d_q, T.q.data(), T.q.size(), hipMemcpyHostToDevice));
        FQZ5_HIP(hipMemcpy(T.d_qoff, T.qoff.data(), T.qoff.size() * 8, hipMemcpyHostToDevice));
        FQZ5_HIP(hipMemcpy(T.d_slots, T.slots.data(), T.slots.size() * 8, hipMemcpyHostToDevice));
        T.device = dev;
    } else if (T.device != dev) {
        throw GpuError("seqs_match: the table was uploaded to another device");
    }
    return SmDev{T.d_slots, T.d_q, T.d_qoff, T.mask, T.anchor, T.tag_bits};
}

}  // namespace

// the records' inclusive ends; fails unless the last is seq_len (name_match.hpp)
std::vector<uint64_t> record_ends(const uint32_t *lens, uint64_t nrec, uint64_t seq_len,
                                  const char *who) {
    std::vector<uint64_t> end(static_cast<size_t>(nrec));
    uint64_t at = 0;
    for (uint64_t r = 0; r < nrec; r++) end[size_t(r)] = at += lens[r];
    if (at != seq_len)
        throw GpuError(std::string(who) + ": the record lengths do not sum to the bases");
    return end;
}

}  // namespace fqz5

using namespace fqz5;

extern "C" {

fqz5_seq_table *fqz5_seqs_table_build(const uint8_t *q, uint64_t q_len, uint64_t nq, int tag_bits,
                                      int anchor) {
    fqz5_seq_table *T = nullptr;
    try {
        char msg[112];
        if (tag_bits < 1 || tag_bits > 32) throw GpuError("seqs_table_build: tag_bits not in 1..32");
        if (!nq) throw GpuError("seqs_table_build: no pattern");
        if (nq > SM_QUERIES_MAX) throw GpuError("seqs_table_build: more than 2^20 patterns");
        if (anchor < 0 || uint32_t(anchor) > SM_ANCHOR_MAX)
            throw GpuError("seqs_table_build: anchor not in 0..64");
        T = new fqz5_seq_table();
        T->tag_bits = tag_bits;
        T->q.assign(q, q + q_len);
        T->qoff.reserve(size_t(nq) + 1);
        uint64_t at = 0, shortest = SM_PATTERN_MAX;
        for (uint64_t k = 0; k < nq; k++) {
            const void *z = at < q_len ? std::memchr(q + at, 0, q_len - at) : nullptr;
            if (!z) throw GpuError("seqs_table_build: fewer terminated patterns than nq");
            const uint64_t e = uint64_t(static_cast<const uint8_t *>(z) - q);
            if (e == at || e - at > SM_PATTERN_MAX) {
                std::snprintf(msg, sizeof msg, "seqs_table_build: pattern %llu is %s",
                              static_cast<unsigned long long>(k),
                              e == at ? "empty" : "longer than 65535 bytes");
                throw GpuError(msg);
            }
            shortest = std::min(shortest, e - at);
            T->qoff.push_back(at);
            at = e + 1;
        }
        T->qoff.push_back(at);
        if (at != q_len) throw GpuError("seqs_table_build: bytes after the last pattern");
        if (uint64_t(anchor) > shortest)
            throw GpuError("seqs_table_build: the anchor is longer than the shortest pattern");
        T->anchor = anchor ? uint32_t(anchor)
                           : uint32_t(std::min<uint64_t>(shortest, SM_ANCHOR_DEFAULT));
        // duplicates: equal neighbours of the patterns in byte order
        const uint8_t *qb = T->q.data();
        const auto len_of = [&](uint32_t k) { return T->qoff[k + 1] - 1 - T->qoff[k]; };
        std::vector<uint32_t> ord(static_cast<size_t>(nq));
        std::iota(ord.begin(), ord.end(), 0u);
        const auto cmp = [&](uint32_t a, uint32_t b) {
            const uint64_t la = len_of(a), lb = len_of(b);
            const int c = std::memcmp(qb + T->qoff[a], qb + T->qoff[b], size_t(std::min(la, lb)));
            return c ? c : (la < lb ? -1 : la > lb);
        };
        std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
            const int c = cmp(a, b);
            return c ? c < 0 : a < b;
        });
        uint64_t dup = nq, of = 0;                  // the lowest duplicate and its first copy
        for (size_t i = 1, first = 0; i < ord.size(); i++) {
            if (cmp(ord[first], ord[i])) { first = i; continue; }
            if (ord[i] < dup) { dup = ord[i]; of = ord[first]; }
        }
        if (dup != nq) {
            std::snprintf(msg, sizeof msg,
                          "seqs_table_build: pattern %llu is a duplicate of pattern %llu",
                          static_cast<unsigned long long>(dup), static_cast<unsigned long long>(of));
            throw GpuError(msg);
        }
        uint64_t cap = 2;
        while (cap < 2 * nq) cap <<= 1;
        T->mask = uint32_t(cap - 1);
        T->slots.assign(size_t(cap), nm_slot(0, NM_NONE));
        for (uint64_t k = 0; k < nq; k++) {
            const uint32_t mixed = anchor_hash(qb + T->qoff[k], T->anchor);
            uint32_t sl = mixed & T->mask;
            while (uint32_t(T->slots[sl] >> 32) != NM_NONE) sl = (sl + 1) & T->mask;
            T->slots[sl] = nm_slot(nm_tag(mixed, tag_bits), uint32_t(k));
        }
        return T;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        delete T;
        return nullptr;
    }
}

void fqz5_seqs_table_free(fqz5_seq_table *T) {
    if (!T) return;
    if (T->d_q) (void)hipFree(T->d_q);
    if (T->d_qoff) (void)hipFree(T->d_qoff);
    if (T->d_slots) (void)hipFree(T->d_slots);
    delete T;
}

uint32_t fqz5_seqs_table_anchor(const fqz5_seq_table *T) { return T ? T->anchor : 0; }

uint32_t fqz5_seqs_match_tile(void) { return SM_TILE; }

int fqz5_seqs_scan_host(const fqz5_seq_table *T, const uint8_t *seq, uint64_t seq_len,
                        const uint32_t *lens, uint64_t nrec, uint32_t *hit, uint8_t *seen) {
    try {
        if (!T) throw GpuError("seqs_scan_host: no table");
        if (nrec >= (1ull << 31)) throw GpuError("seqs_scan_host: block too large");
        const std::vector<uint64_t> end = record_ends(lens, nrec, seq_len, "seqs_scan_host");
        for (uint64_t r = 0; r < nrec; r++) hit[r] = NM_NONE;
        const uint32_t m = T->anchor, n = uint32_t(nrec);
        for (uint64_t p = 0; p + m <= seq_len; p++) {
            const uint32_t mixed = anchor_hash(seq + p, m), tag = nm_tag(mixed, T->tag_bits);
            uint32_t rec = NM_NONE;
            uint32_t sl = mixed & T->mask;
            for (uint32_t k = 0; k <= T->mask; k++, sl = (sl + 1) & T->mask) {
                const uint64_t ent = T->slots[sl];
                const uint32_t qi = uint32_t(ent >> 32);
                if (qi == NM_NONE) break;
                if (uint32_t(ent) != tag) continue;
                if (rec == NM_NONE) rec = owner(end.data(), n, p);
                const uint64_t qa = T->qoff[qi], len = T->qoff[qi + 1] - 1 - qa;
                if (p + len > end[rec] || std::memcmp(seq + p, T->q.data() + qa, size_t(len))) continue;
                hit[rec] = std::min(hit[rec], qi);
                if (seen) seen[qi] |= 1;
            }
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
        if (nrec >= (1ull << 31)) throw GpuError("seqs_match: block too large");
        const std::vector<uint64_t> end = record_ends(h_len, nrec, seq_len, "seqs_match");
        if (!nrec || seq_len < T->anchor) return 0;      // no position holds an anchor
        GpuCtx &g = gpu();
        gp = &g;
        const SmDev D = device_copy(*const_cast<fqz5_seq_table *>(T));
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
