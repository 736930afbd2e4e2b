// filter.hip — filter by read metrics (fqz5file.filter_records /
// filter_file): which records of a block's decoded bases and qualities pass a
// rule over their length, N count, mean quality, low-quality share, GC share
// and complexity (the rule: include/fqz5_fastq.h).
//
// Two kernels per block:
//   k_filter_sums  streams the bases and the qualities with the tile walk of
//                  record_tile.hpp (the one k_stats_tiles runs, without its
//                  histograms) and leaves five sums per record: n, gc and
//                  diff from the bases, qsum and lowq from the qualities.  A
//                  record's partial sums of one chunk are added once: to the
//                  tile's LDS cells of that record (flushed to the record's
//                  global cells once per tile), or, past ST_KCAP records of
//                  one tile, straight to the global cells.  diff at position
//                  p needs byte p + 1: it is the next byte of the chunk, or
//                  for the chunk's last
//                  position one byte read on its own (the next chunk's first,
//                  which may be the next tile's first); it counts only when
//                  p + 1 lies before the end of p's record, which at a tile's
//                  last position the record's unclipped end decides.
//   k_filter_pick  one thread per unit (a record, with pairs two): the rule
//                  over the sums and the lengths, the reason counters in LDS
//                  (flushed once per workgroup), and per record whether it is
//                  selected.
// The selected records are then compacted by nm_compact (name_match.hip), the
// flag kernel, scan and scatter both lookups end with, into ascending indices.
// No stream is read outside [0, seq_len): load16 reads a chunk that is not
// wholly inside byte by byte, and the lone byte p + 1 is read only below
// seq_len.  LDS cells are u32: a tile adds at most ST_TILE * 255 to one, and
// launches are split at 2^31 bases as fqz5_stats_add splits them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fqz5_fastq.h"
#include "gpu_ctx.hpp"
#include "record_tile.hpp"

namespace fqz5 {
GpuCtx &gpu();
void fqz5_set_error(const char *msg);

namespace {

constexpr uint32_t FT_SUMS = 5;                 // n, gc, diff (bases); qsum, lowq (qualities)
constexpr uint32_t FT_NONE = FQZ5_FILTER_REASONS;

__host__ __device__ inline uint32_t is_n(uint32_t c) { return (c | 0x20u) == 'n'; }

__host__ __device__ inline bool base_criterion(const fqz5_filter_spec &f) {
    return (f.set & (1u << 2 | 1u << 5 | 1u << 6)) != 0;
}
__host__ __device__ inline bool qual_criterion(const fqz5_filter_spec &f) {
    return (f.set & (1u << 3 | 1u << 4)) != 0;
}
// the q below which criterion 4 counts (nothing is below 0)
__host__ __device__ inline uint32_t low_q_of(const fqz5_filter_spec &f) {
    return f.set & (1u << 4) ? f.low_q : 0;
}

// the lowest criterion a record fails, FT_NONE when it passes
__host__ __device__ inline uint32_t fails(const fqz5_filter_spec &f, uint64_t L, uint64_t n,
                                          uint64_t gc, uint64_t diff, uint64_t qsum,
                                          uint64_t lowq) {
    const uint32_t s = f.set;
    if ((s & 1u << 0) && !(L >= f.min_len)) return 0;
    if ((s & 1u << 1) && !(L <= f.max_len)) return 1;
    if ((s & 1u << 2) && !(n <= f.max_n)) return 2;
    if ((s & 1u << 3) && !(qsum >= uint64_t(f.min_mean_q) * L)) return 3;
    if ((s & 1u << 4) && !(100 * lowq <= uint64_t(f.max_low_pct) * L)) return 4;
    if ((s & 1u << 5) && !(uint64_t(f.gc_min_pct) * L <= 100 * gc &&
                           100 * gc <= uint64_t(f.gc_max_pct) * L)) return 5;
    if ((s & 1u << 6) && !(100 * diff >= uint64_t(f.min_complexity_pct) * (L ? L - 1 : 0)))
        return 6;
    return FT_NONE;
}

struct SumsDev {                                // (a NULL array: its sums are 0)
    uint32_t *n, *gc, *diff;
    uint64_t *qsum;
    uint32_t *lowq;
};

__global__ __launch_bounds__(ST_THREADS) void k_filter_sums(
    const uint8_t *seq, const uint8_t *qual, uint64_t seq_len, const uint64_t *end,
    const uint32_t *tf, uint32_t nrec, uint64_t tile_a, uint64_t tile_b, uint32_t low_q,
    SumsDev out) {
    __shared__ uint32_t lend[ST_KCAP];
    __shared__ uint32_t lsum[FT_SUMS * ST_KCAP];   // [sum][record of the tile]
    for (uint32_t i = threadIdx.x; i < FT_SUMS * ST_KCAP; i += ST_THREADS) lsum[i] = 0;
    for (uint64_t t = tile_a + blockIdx.x; t < tile_b; t += gridDim.x) {
        Tile T;
        T.open(end, tf, nrec, seq_len, t, lend);
        __syncthreads();                        // (the last tile's flush has read lsum)
        T.stage(lend);
        __syncthreads();
        const int64_t tend = int64_t(T.t0) + T.n;
        for (uint32_t s = 0; s < 2; s++) {
            const uint8_t *src = s ? qual : seq;
            if (!src) continue;
            tile_chunks(T, src, [&](int64_t a) {
                const uint4 v = load16(src, seq_len, a);
                // the byte after the chunk, for diff at the chunk's last position
                // when that is one of the tile's (a + 15 >= t0 always)
                uint32_t after = 0;
                if (!s && a + 15 < tend && uint64_t(a + 16) < seq_len) after = src[a + 16];
                const uint32_t w[5] = {v.x, v.y, v.z, v.w, after};
                ChunkWalk W(T, a);
                uint32_t acc0 = 0, acc1 = 0, acc2 = 0;
                W.bytes(T, a, v, [&](uint32_t q, uint32_t k, uint32_t c, int b) {
                    acc0 += s ? c : is_n(c);
                    acc1 += s ? c < low_q : is_gc(c);
                    if (s) return;
                    const uint32_t nx = (w[(b + 1) >> 2] >> (8 * ((b + 1) & 3))) & 0xFFu;
                    if (c == nx) return;
                    // is p + 1 still in p's record?  ek is clipped to the tile:
                    // at the tile's last position the record's own end decides
                    if (q + 1 < W.ek || (q + 1 == ST_TILE && T.end[T.r0 + k] > T.t0 + ST_TILE)) acc2++;
                }, [&](uint32_t rec) {
                    if (rec < ST_KCAP) {
                        uint32_t *cell = lsum + (s ? 3 : 0) * ST_KCAP + rec;
                        if (acc0) atomicAdd(cell, acc0);
                        if (acc1) atomicAdd(cell + ST_KCAP, acc1);
                        if (acc2) atomicAdd(cell + 2 * ST_KCAP, acc2);
                    } else if (s) {
                        flush_cell(out.qsum + T.r0 + rec, acc0);
                        if (acc1) atomicAdd(out.lowq + T.r0 + rec, acc1);
                    } else {
                        if (acc0) atomicAdd(out.n + T.r0 + rec, acc0);
                        if (acc1) atomicAdd(out.gc + T.r0 + rec, acc1);
                        if (acc2) atomicAdd(out.diff + T.r0 + rec, acc2);
                    }
                    acc0 = acc1 = acc2 = 0;
                });
            });
        }
        __syncthreads();
        flush_records<FT_SUMS>(T, lsum, [&](uint32_t j, uint32_t r, uint32_t x) {
            if (j == 3) flush_cell(out.qsum + r, x);
            else atomicAdd((j == 0 ? out.n : j == 1 ? out.gc : j == 2 ? out.diff : out.lowq) + r, x);
        });
    }
}

// hit[r] = 0 where record r is selected, NM_NONE where not (nm_compact's
// input); failed[reason] += the units that fail
__global__ __launch_bounds__(ST_THREADS) void k_filter_pick(fqz5_filter_spec f, const uint64_t *end,
                                                            uint32_t nrec, uint32_t mates,
                                                            int invert, SumsDev in, uint32_t *hit,
                                                            unsigned long long *failed) {
    __shared__ unsigned long long cnt[FQZ5_FILTER_REASONS];
    if (threadIdx.x < FQZ5_FILTER_REASONS) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t units = nrec / mates;
    for (uint64_t u = uint64_t(blockIdx.x) * ST_THREADS + threadIdx.x; u < units;
         u += uint64_t(gridDim.x) * ST_THREADS) {
        uint32_t reason = FT_NONE;
        for (uint32_t m = 0; m < mates; m++) {
            const uint32_t r = uint32_t(u) * mates + m;
            const uint64_t L = end[r] - (r ? end[r - 1] : 0);
            const uint32_t why = fails(f, L, in.n ? in.n[r] : 0, in.gc ? in.gc[r] : 0,
                                       in.diff ? in.diff[r] : 0, in.qsum ? in.qsum[r] : 0,
                                       in.lowq ? in.lowq[r] : 0);
            reason = why < reason ? why : reason;
        }
        if (reason != FT_NONE) atomicAdd(&cnt[reason], 1ull);
        const uint32_t h = ((reason == FT_NONE) != (invert != 0)) ? 0u : NM_NONE;
        for (uint32_t m = 0; m < mates; m++) hit[uint32_t(u) * mates + m] = h;
    }
    __syncthreads();
    if (threadIdx.x < FQZ5_FILTER_REASONS && cnt[threadIdx.x])
        atomicAdd(failed + threadIdx.x, cnt[threadIdx.x]);
}

// the checks both entry points make before anything is written
std::vector<uint64_t> check_call(const fqz5_filter_spec *f, bool has_seq, bool has_qual,
                                 uint64_t seq_len, const uint32_t *lens, uint64_t nrec, int pairs,
                                 const char *who) {
    if (!f) throw GpuError(std::string(who) + ": no criteria");
    if (f->set >> FQZ5_FILTER_REASONS) throw GpuError(std::string(who) + ": an unknown criterion");
    if (base_criterion(*f) && !has_seq)
        throw GpuError(std::string(who) + ": a base criterion without the bases");
    if (qual_criterion(*f) && !has_qual)
        throw GpuError(std::string(who) + ": a quality criterion without the qualities");
    check_records(nrec, pairs, who);
    return record_ends(lens, nrec, seq_len, who);
}

}  // namespace
}  // namespace fqz5

using namespace fqz5;

extern "C" {

uint32_t fqz5_filter_tile(void) { return ST_TILE; }

int fqz5_filter_match(const fqz5_filter_spec *f, const uint8_t *d_seq, const uint8_t *d_qual,
                      uint64_t seq_len, const uint32_t *h_len, uint64_t nrec, int pairs,
                      int invert, uint32_t *d_rec, uint64_t *n_hit, uint64_t *h_failed,
                      const fqz5_filter_sums *d_sums) {
    GpuCtx *gp = nullptr;
    unsigned long long failed[FQZ5_FILTER_REASONS] = {};   // (outlives the try: a copy lands here)
    try {
        *n_hit = 0;
        const std::vector<uint64_t> end = check_call(f, d_seq != nullptr, d_qual != nullptr, seq_len,
                                                     h_len, nrec, pairs, "filter_match");
        if (!nrec) return 0;
        GpuCtx &g = gpu();
        gp = &g;
        const uint32_t n = uint32_t(nrec);
        // the streams the call needs; one that is not streamed leaves zeros
        const uint8_t *seq = base_criterion(*f) || d_sums ? d_seq : nullptr;
        const uint8_t *qual = qual_criterion(*f) || d_sums ? d_qual : nullptr;
        SumsDev S = {nullptr, nullptr, nullptr, nullptr, nullptr};
        if (d_sums) S = SumsDev{d_sums->n, d_sums->gc, d_sums->diff, d_sums->qsum, d_sums->lowq};
        const auto want = [&](auto *&p, bool streamed) {
            using T = std::remove_reference_t<decltype(*p)>;
            if (!p && streamed) p = g.arena.alloc_n<T>(n);
            if (p) g.memset0(p, size_t(n) * sizeof(T));
        };
        want(S.n, seq != nullptr);
        want(S.gc, seq != nullptr);
        want(S.diff, seq != nullptr);
        want(S.qsum, qual != nullptr);
        want(S.lowq, qual != nullptr);
        const uint64_t *d_end = g.upload(end);
        const uint64_t tiles = (seq_len + ST_TILE - 1) / ST_TILE;
        if (tiles && (seq || qual)) {
            const uint32_t *d_tf = g.upload(tile_first(end, tiles));
            // launches of at most 2^31 bases (fqz5_stats_add's bound on a u32 LDS cell)
            for (uint64_t a = 0; a < tiles; a += ST_LAUNCH_TILES) {
                const uint64_t b = std::min(tiles, a + ST_LAUNCH_TILES);
                const uint32_t grid = uint32_t(std::min<uint64_t>(b - a, 4ull * g.cus));
                hipLaunchKernelGGL(k_filter_sums, dim3(grid), dim3(ST_THREADS), 0, g.stream, seq, qual,
                                   seq_len, d_end, d_tf, n, a, b, low_q_of(*f), S);
                FQZ5_HIP(hipGetLastError());
            }
        }
        const uint32_t mates = pairs ? 2 : 1;
        uint32_t *hit = g.arena.alloc_n<uint32_t>(n);
        uint32_t *query = g.arena.alloc_n<uint32_t>(n);
        unsigned long long *d_failed = g.arena.alloc_n<unsigned long long>(FQZ5_FILTER_REASONS);
        g.memset0(d_failed, FQZ5_FILTER_REASONS * 8);
        const uint32_t grid = uint32_t(std::min<uint64_t>((n / mates + ST_THREADS - 1) / ST_THREADS,
                                                          4ull * g.cus));
        hipLaunchKernelGGL(k_filter_pick, dim3(grid), dim3(ST_THREADS), 0, g.stream, *f, d_end, n,
                           mates, invert, S, hit, d_failed);
        FQZ5_HIP(hipGetLastError());
        g.download(failed, d_failed, FQZ5_FILTER_REASONS);
        *n_hit = nm_compact(g, hit, n, 0, d_rec, query);     // (synchronises: `failed` is here)
        for (int k = 0; k < FQZ5_FILTER_REASONS; k++) h_failed[k] += failed[k];
        g.reset();
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { if (gp) gp->reset(); } catch (...) {}
        return -1;
    }
}

int fqz5_filter_host(const fqz5_filter_spec *f, const uint8_t *seq, const uint8_t *qual,
                     uint64_t seq_len, const uint32_t *lens, uint64_t nrec, int pairs, int invert,
                     uint8_t *keep, uint64_t *failed, const fqz5_filter_sums *sums) {
    try {
        check_call(f, seq != nullptr, qual != nullptr, seq_len, lens, nrec, pairs, "filter_host");
        const uint32_t low_q = low_q_of(*f);
        std::vector<uint32_t> why(size_t(nrec), FT_NONE);
        uint64_t at = 0;
        for (uint64_t r = 0; r < nrec; r++) {
            const uint64_t L = lens[r];
            uint64_t n = 0, gc = 0, diff = 0, qsum = 0, lowq = 0;
            for (uint64_t i = 0; seq && i < L; i++) {
                const uint32_t c = seq[at + i];
                n += is_n(c);
                gc += is_gc(c);
                diff += i + 1 < L && c != seq[at + i + 1];
            }
            for (uint64_t i = 0; qual && i < L; i++) {
                qsum += qual[at + i];
                lowq += qual[at + i] < low_q;
            }
            why[size_t(r)] = fails(*f, L, n, gc, diff, qsum, lowq);
            if (sums) {
                if (sums->n) sums->n[r] = uint32_t(n);
                if (sums->gc) sums->gc[r] = uint32_t(gc);
                if (sums->diff) sums->diff[r] = uint32_t(diff);
                if (sums->qsum) sums->qsum[r] = qsum;
                if (sums->lowq) sums->lowq[r] = uint32_t(lowq);
            }
            at += L;
        }
        const uint64_t mates = pairs ? 2 : 1;
        for (uint64_t u = 0; u < nrec / mates; u++) {
            uint32_t reason = FT_NONE;
            for (uint64_t m = 0; m < mates; m++) reason = std::min(reason, why[size_t(u * mates + m)]);
            if (reason != FT_NONE) failed[reason]++;
            for (uint64_t m = 0; m < mates; m++)
                keep[u * mates + m] = (reason == FT_NONE) != (invert != 0);
        }
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

}  // extern "C"
