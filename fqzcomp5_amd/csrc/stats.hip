// stats.hip — read QC statistics of a block's decoded bases and qualities
// (fqz5file.stats): whole-file byte histograms, per-cycle tables up to a cap,
// and per-read mean quality and GC content, accumulated over the blocks of a
// file in one device table of u64 counts (layout: include/fqz5_fastq.h).
//
// Three kernels per block, all over tiles of ST_TILE bases:
//   k_stats_tiles   base_counts, qual_counts and the per-read sums.  Workgroups
//                   persist over tiles (grid-stride); the 256-bin histograms
//                   live in LDS for the workgroup's whole life, the per-read
//                   partial sums in LDS for one tile, so a read's gc / quality
//                   sum costs one global add per tile it touches.
//   k_stats_cycles  cycle_base and cycle_qual.  A workgroup owns a window of
//                   64 / mates cycles (64 KiB of u32 cells in LDS) and
//                   grid-strides over the tiles, skipping those in which no
//                   record can have a position inside its window.
//   k_stats_bin     read_qual and read_gc from the per-read sums.
// The tiles, the walk that gives every base its record, the loads and the
// flush of the per-read sums are record_tile.hpp's, shared with filter.hip:
// both arrays are streamed in 16-byte chunks at 16-byte addresses, each by
// its own alignment, and never read outside [0, seq_len).  No table is
// touched by a global atomic per base: LDS cells are u32, bounded by the bases
// of one launch (at most 2^31, launches are split), and flushed once per
// workgroup, non-zero cells only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/fqz5_fastq.h"
#include "gpu_ctx.hpp"
#include "record_tile.hpp"

namespace fqz5 {
GpuCtx &gpu();
void fqz5_set_error(const char *msg);
}  // namespace fqz5

// the device table (one mate's words after the other) and the four counts per
// mate the host keeps from the record lengths
struct fqz5_stats {
    uint32_t cycles = 0;
    int mates = 1;
    int device = -1;
    uint64_t *d_tab = nullptr;
    uint64_t scal[2][4] = {};
};

namespace fqz5 {
namespace {

constexpr uint32_t ST_WIN_CELLS = 64;           // cycles x mates of one cycle window
constexpr uint32_t ST_CYCLES_MAX = 1u << 16;
// words of one mate's block
constexpr uint64_t ST_RECORDS = 0, ST_BASES = 1, ST_QUAL_RECORDS = 2, ST_EMPTY = 3, ST_BASE = 4,
                   ST_QUAL = 260, ST_READ_QUAL = 516, ST_READ_GC = 772, ST_CYCLE_BASE = 873;
__host__ __device__ inline uint64_t st_cycle_qual(uint32_t cycles) {
    return ST_CYCLE_BASE + 6ull * cycles;
}
__host__ __device__ inline uint64_t st_words(uint32_t cycles) {
    return ST_CYCLE_BASE + 262ull * cycles;
}

// A, C, G, T, N, other (case folded)
__host__ __device__ inline uint32_t base_class(uint32_t c) {
    const uint32_t f = c | 0x20u;
    return f == 'a' ? 0 : f == 'c' ? 1 : f == 'g' ? 2 : f == 't' ? 3 : f == 'n' ? 4 : 5;
}
// base_counts, qual_counts, and per record the number of G/C bytes and the
// sum of the qualities.  A lane walks the records across its chunk and adds a
// record's partial sum once: to the tile's LDS cell of that record (flushed
// to the record's global cell once per tile: a read spanning many tiles gets
// one global add per tile), or, past ST_KCAP records of one tile, straight
// to the global cell (such records are a byte or two long: a few adds each).
__global__ __launch_bounds__(ST_THREADS) void k_stats_tiles(
    const uint8_t *seq, const uint8_t *qual, uint64_t seq_len, const uint64_t *end,
    const uint32_t *tf, uint32_t nrec, uint64_t tile_a, uint64_t tile_b, int mates, uint64_t *tab,
    uint64_t per, uint32_t *rec_gc, uint64_t *rec_qsum) {
    __shared__ uint32_t hist[2 * 2 * 256];      // [stream][mate][byte]
    __shared__ uint32_t lend[ST_KCAP];
    __shared__ uint32_t lsum[2 * ST_KCAP];      // [stream][record of the tile]
    for (uint32_t i = threadIdx.x; i < 2 * 2 * 256; i += ST_THREADS) hist[i] = 0;
    for (uint32_t i = threadIdx.x; i < 2 * ST_KCAP; i += ST_THREADS) lsum[i] = 0;
    const uint32_t pair = mates == 2 ? 1u : 0u;
    for (uint64_t t = tile_a + blockIdx.x; t < tile_b; t += gridDim.x) {
        Tile T;
        T.open(end, tf, nrec, seq_len, t, lend);
        __syncthreads();                        // (the last tile's flush has read lsum)
        T.stage(lend);
        __syncthreads();
        for (uint32_t s = 0; s < 2; s++) {
            const uint8_t *src = s ? qual : seq;
            if (!src) continue;
            tile_chunks(T, src, [&](int64_t a) {
                const uint4 v = load16(src, seq_len, a);
                ChunkWalk W(T, a);
                uint32_t acc = 0;
                W.bytes(T, a, v, [&](uint32_t, uint32_t k, uint32_t c, int) {
                    atomicAdd(&hist[(s * 2 + ((T.r0 + k) & pair)) * 256 + c], 1u);
                    acc += s ? c : is_gc(c);
                }, [&](uint32_t rec) {
                    const uint32_t sum = acc;
                    acc = 0;
                    if (!sum) return;
                    if (rec < ST_KCAP) atomicAdd(&lsum[s * ST_KCAP + rec], sum);
                    else if (s) flush_cell(rec_qsum + T.r0 + rec, sum);
                    else atomicAdd(rec_gc + T.r0 + rec, sum);
                });
            });
        }
        __syncthreads();
        flush_records<2>(T, lsum, [&](uint32_t j, uint32_t r, uint32_t x) {
            if (j) flush_cell(rec_qsum + r, x);
            else atomicAdd(rec_gc + r, x);
        });
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2 * 2 * 256; i += ST_THREADS) {
        const uint32_t s = i >> 9, m = (i >> 8) & 1, c = i & 255;
        flush_cell(tab + m * per + (s ? ST_QUAL : ST_BASE) + c, hist[i]);   // (mate 1 of one: zero)
    }
}

// cycle_base and cycle_qual of the cycles [lo, hi) = window blockIdx.x % nwin
// of `win` cycles below `ceff` (the cap, or the block's longest record when
// that is shorter).  The workgroup takes the tiles g, g + G, ... of the
// launch, g = blockIdx.x / nwin.  A tile is skipped when neither its first
// record has a position of the window inside it nor a later record can
// (those start at or after the first one's end: one reaches cycle lo inside
// the tile only if that end + lo lies before the tile's end).
__global__ __launch_bounds__(ST_THREADS) void k_stats_cycles(
    const uint8_t *seq, const uint8_t *qual, uint64_t seq_len, const uint64_t *end,
    const uint32_t *tf, uint32_t nrec, uint64_t tile_a, uint64_t tile_b, int mates, uint32_t win,
    uint32_t nwin, uint32_t ceff, uint32_t cycles, uint64_t *tab, uint64_t per) {
    extern __shared__ uint4 st_dyn[];
    uint32_t *cq = reinterpret_cast<uint32_t *>(st_dyn);     // [mate][cycle of the window][256]
    uint32_t *cb = cq + ST_WIN_CELLS * 256;                   // [mate][cycle of the window][6]
    uint32_t *lend = cb + ST_WIN_CELLS * 6;
    for (uint32_t i = threadIdx.x; i < ST_WIN_CELLS * 262; i += ST_THREADS) cq[i] = 0;
    const uint32_t pair = mates == 2 ? 1u : 0u;
    const uint32_t wi = blockIdx.x % nwin, g = blockIdx.x / nwin, G = gridDim.x / nwin;
    const uint64_t lo = uint64_t(wi) * win;
    const uint64_t hi = lo + win < ceff ? lo + win : ceff;
    for (uint64_t t = tile_a + g; t < tile_b; t += G) {
        Tile T;
        T.open(end, tf, nrec, seq_len, t, lend);
        const int64_t t0 = int64_t(T.t0), tend = t0 + T.n;
        const int64_t e0 = int64_t(end[T.r0]), s0 = t0 + T.start0;
        const bool first = uint64_t(t0 - s0) < hi && uint64_t((e0 < tend ? e0 : tend) - s0) > lo;
        const bool later = e0 < tend && uint64_t(tend - e0) > lo;
        if (!first && !later) continue;         // (uniform: every thread sees the same tile)
        __syncthreads();                        // (the last tile's walks have read lend)
        T.stage(lend);
        __syncthreads();
        for (uint32_t s = 0; s < 2; s++) {
            const uint8_t *src = s ? qual : seq;
            if (!src) continue;
            tile_chunks(T, src, [&](int64_t a) {
                ChunkWalk W(T, a);
                // the whole chunk inside one record and outside the window: no load
                if (W.ek >= W.q0 + 16 && (uint64_t(int64_t(W.q0) - W.st) >= hi ||
                                          uint64_t(int64_t(W.q0) + 15 - W.st) < lo))
                    return;
                const uint4 v = load16(src, seq_len, a);
                W.bytes(T, a, v, [&](uint32_t q, uint32_t k, uint32_t c, int) {
                    const uint64_t cyc = uint64_t(int64_t(q) - W.st);
                    if (cyc < lo || cyc >= hi) return;
                    const uint32_t cell = ((T.r0 + k) & pair) * win + uint32_t(cyc - lo);
                    if (s) atomicAdd(&cq[cell * 256 + c], 1u);
                    else atomicAdd(&cb[cell * 6 + base_class(c)], 1u);
                }, [](uint32_t) {});
            });
        }
    }
    __syncthreads();
    const uint32_t nc = uint32_t(hi - lo);      // cycles of the window below the cap
    for (uint32_t i = threadIdx.x; i < uint32_t(mates) * win * 256; i += ST_THREADS) {
        const uint32_t m = i / (win * 256), c = (i / 256) % win;
        if (c < nc) flush_cell(tab + m * per + st_cycle_qual(cycles) + (lo + c) * 256 + (i & 255), cq[i]);
    }
    for (uint32_t i = threadIdx.x; i < uint32_t(mates) * win * 6; i += ST_THREADS) {
        const uint32_t m = i / (win * 6), c = (i / 6) % win;
        if (c < nc) flush_cell(tab + m * per + ST_CYCLE_BASE + (lo + c) * 6 + i % 6, cb[i]);
    }
}

// read_gc and read_qual from the records' sums (records of length 0 in neither)
__global__ __launch_bounds__(ST_THREADS) void k_stats_bin(const uint64_t *end, uint32_t nrec,
                                                          const uint32_t *rec_gc,
                                                          const uint64_t *rec_qsum, int has_qual,
                                                          int mates, uint64_t *tab, uint64_t per) {
    __shared__ uint32_t h[2 * 357];             // [mate][256 read_qual, 101 read_gc]
    for (uint32_t i = threadIdx.x; i < 2 * 357; i += ST_THREADS) h[i] = 0;
    __syncthreads();
    const uint32_t pair = mates == 2 ? 1u : 0u;
    for (uint64_t r = uint64_t(blockIdx.x) * ST_THREADS + threadIdx.x; r < nrec;
         r += uint64_t(gridDim.x) * ST_THREADS) {
        const uint64_t len = end[r] - (r ? end[r - 1] : 0);
        if (!len) continue;
        uint32_t *hm = h + (uint32_t(r) & pair) * 357;
        atomicAdd(&hm[256 + uint32_t(100ull * rec_gc[r] / len)], 1u);
        if (has_qual) atomicAdd(&hm[uint32_t(rec_qsum[r] / len)], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2 * 357; i += ST_THREADS) {
        const uint32_t m = i / 357, c = i % 357;
        flush_cell(tab + m * per + (c < 256 ? ST_READ_QUAL + c : ST_READ_GC + (c - 256)), h[i]);
    }
}

// records, bases, qual_records and empty per mate, from the lengths
void count_records(const uint32_t *lens, uint64_t nrec, int mates, bool has_qual,
                   uint64_t scal[2][4]) {
    for (uint64_t r = 0; r < nrec; r++) {
        uint64_t *s = scal[mates == 2 ? r & 1 : 0];
        s[ST_RECORDS]++;
        s[ST_BASES] += lens[r];
        s[ST_QUAL_RECORDS] += has_qual;
        s[ST_EMPTY] += lens[r] == 0;
    }
}

void check_shape(uint32_t cycles, int mates, uint64_t nrec, const char *who) {
    if (mates != 1 && mates != 2) throw GpuError(std::string(who) + ": mates is not 1 or 2");
    if (cycles < 1 || cycles > ST_CYCLES_MAX)
        throw GpuError(std::string(who) + ": cycles not in 1..65536");
    check_records(nrec, mates == 2, who);
}

}  // namespace
}  // namespace fqz5

using namespace fqz5;

extern "C" {

uint32_t fqz5_stats_tile(void) { return ST_TILE; }

uint64_t fqz5_stats_words(uint32_t cycles, int mates) { return uint64_t(mates) * st_words(cycles); }

fqz5_stats *fqz5_stats_new(uint32_t cycles, int mates) {
    fqz5_stats *S = nullptr;
    try {
        check_shape(cycles, mates, 0, "stats_new");
        GpuCtx &g = gpu();
        S = new fqz5_stats();
        S->cycles = cycles;
        S->mates = mates;
        FQZ5_HIP(hipGetDevice(&S->device));
        const size_t bytes = size_t(mates) * st_words(cycles) * 8;
        FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&S->d_tab), bytes));
        FQZ5_HIP(hipMemsetAsync(S->d_tab, 0, bytes, g.stream));
        g.sync();
        return S;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        if (S && S->d_tab) (void)hipFree(S->d_tab);
        delete S;
        return nullptr;
    }
}

void fqz5_stats_free(fqz5_stats *S) {
    if (!S) return;
    if (S->d_tab) (void)hipFree(S->d_tab);
    delete S;
}

int fqz5_stats_add(fqz5_stats *S, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t seq_len,
                   const uint32_t *h_lens, uint64_t nrec, uint64_t *d_rec_qsum,
                   uint32_t *d_rec_gc) {
    GpuCtx *gp = nullptr;
    try {
        if (!S) throw GpuError("stats_add: no accumulator");
        check_shape(S->cycles, S->mates, nrec, "stats_add");
        const std::vector<uint64_t> end = record_ends(h_lens, nrec, seq_len, "stats_add");
        if (!nrec) return 0;
        GpuCtx &g = gpu();
        gp = &g;
        int dev = 0;
        FQZ5_HIP(hipGetDevice(&dev));
        if (dev != S->device) throw GpuError("stats_add: the accumulator is on another device");
        const uint32_t n = uint32_t(nrec);
        const uint64_t per = st_words(S->cycles);
        uint32_t *rec_gc = d_rec_gc ? d_rec_gc : g.arena.alloc_n<uint32_t>(n);
        uint64_t *rec_qsum = d_rec_qsum ? d_rec_qsum : g.arena.alloc_n<uint64_t>(n);
        g.memset0(rec_gc, size_t(n) * 4);
        g.memset0(rec_qsum, size_t(n) * 8);
        const uint64_t *d_end = g.upload(end);
        const uint64_t tiles = (seq_len + ST_TILE - 1) / ST_TILE;
        if (tiles) {
            const std::vector<uint32_t> tf = tile_first(end, tiles);
            uint32_t longest = 0;
            for (uint64_t k = 0; k < nrec; k++) longest = std::max(longest, h_lens[k]);
            const uint32_t *d_tf = g.upload(tf);
            const uint32_t ceff = std::min(S->cycles, longest);
            const uint32_t win = ST_WIN_CELLS / uint32_t(S->mates);
            const uint32_t nwin = (ceff + win - 1) / win;
            const uint32_t lds = (ST_WIN_CELLS * 262 + ST_KCAP) * 4;
            FQZ5_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_stats_cycles),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
            // launches of at most 2^31 bases: what bounds every u32 cell in LDS
            for (uint64_t a = 0; a < tiles; a += ST_LAUNCH_TILES) {
                const uint64_t b = std::min(tiles, a + ST_LAUNCH_TILES), nt = b - a;
                const uint32_t grid = uint32_t(std::min<uint64_t>(nt, 4ull * g.cus));
                hipLaunchKernelGGL(k_stats_tiles, dim3(grid), dim3(ST_THREADS), 0, g.stream, d_seq,
                                   d_qual, seq_len, d_end, d_tf, n, a, b, S->mates, S->d_tab, per,
                                   rec_gc, rec_qsum);
                FQZ5_HIP(hipGetLastError());
                const uint32_t G = uint32_t(std::min<uint64_t>(
                    nt, std::max<uint64_t>(1, 2ull * g.cus / nwin)));
                hipLaunchKernelGGL(k_stats_cycles, dim3(nwin * G), dim3(ST_THREADS), lds, g.stream,
                                   d_seq, d_qual, seq_len, d_end, d_tf, n, a, b, S->mates, win, nwin,
                                   ceff, S->cycles, S->d_tab, per);
                FQZ5_HIP(hipGetLastError());
            }
            const uint32_t grid = uint32_t(std::min<uint64_t>((nrec + ST_THREADS - 1) / ST_THREADS,
                                                              4ull * g.cus));
            hipLaunchKernelGGL(k_stats_bin, dim3(grid), dim3(ST_THREADS), 0, g.stream, d_end, n,
                               rec_gc, rec_qsum, d_qual ? 1 : 0, S->mates, S->d_tab, per);
            FQZ5_HIP(hipGetLastError());
        }
        g.reset();
        count_records(h_lens, nrec, S->mates, d_qual != nullptr, S->scal);
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { if (gp) gp->reset(); } catch (...) {}
        return -1;
    }
}

int fqz5_stats_read(const fqz5_stats *S, uint64_t *h_out, uint64_t cap) {
    try {
        if (!S) throw GpuError("stats_read: no accumulator");
        const uint64_t per = st_words(S->cycles), words = uint64_t(S->mates) * per;
        if (cap < words) throw GpuError("stats_read: the output is smaller than the tables");
        FQZ5_HIP(hipMemcpy(h_out, S->d_tab, size_t(words) * 8, hipMemcpyDeviceToHost));
        for (int m = 0; m < S->mates; m++)
            for (int k = 0; k < 4; k++) h_out[m * per + k] = S->scal[m][k];
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

int fqz5_stats_host(uint32_t cycles, int mates, const uint8_t *seq, const uint8_t *qual,
                    uint64_t seq_len, const uint32_t *lens, uint64_t nrec, uint64_t *h_out,
                    uint64_t cap, uint64_t *rec_qsum, uint32_t *rec_gc) {
    try {
        check_shape(cycles, mates, nrec, "stats_host");
        const uint64_t per = st_words(cycles);
        if (cap < uint64_t(mates) * per)
            throw GpuError("stats_host: the output is smaller than the tables");
        const std::vector<uint64_t> end = record_ends(lens, nrec, seq_len, "stats_host");
        uint64_t scal[2][4] = {};
        count_records(lens, nrec, mates, qual != nullptr, scal);
        uint64_t at = 0;
        for (uint64_t r = 0; r < nrec; r++) {
            const int m = mates == 2 ? int(r & 1) : 0;
            uint64_t *tab = h_out + m * per;
            const uint64_t len = lens[r];
            uint64_t gc = 0, qs = 0;
            for (uint64_t i = 0; i < len; i++) {
                const uint32_t c = seq[at + i];
                tab[ST_BASE + c]++;
                gc += is_gc(c);
                if (i < cycles) tab[ST_CYCLE_BASE + i * 6 + base_class(c)]++;
                if (!qual) continue;
                const uint32_t q = qual[at + i];
                tab[ST_QUAL + q]++;
                qs += q;
                if (i < cycles) tab[st_cycle_qual(cycles) + i * 256 + q]++;
            }
            if (len) {
                tab[ST_READ_GC + 100 * gc / len]++;
                if (qual) tab[ST_READ_QUAL + qs / len]++;
            }
            if (rec_gc) rec_gc[r] = uint32_t(gc);
            if (rec_qsum) rec_qsum[r] = qs;
            at += len;
        }
        for (int m = 0; m < mates; m++)
            for (int k = 0; k < 4; k++) h_out[m * per + k] += scal[m][k];
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

}  // extern "C"
