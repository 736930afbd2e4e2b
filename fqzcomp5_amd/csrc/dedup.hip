// dedup.hip — duplicates (fqz5file.dedup_records / dedup_file / duplication):
// which units of a file are the first of their sequence (the rule, the key and
// the table: include/fqz5_fastq.h).
//
// Per block:
//   k_dedup_keys    streams the bases with the tile walk of record_tile.hpp, as
//                   k_filter_sums does, and leaves per record two sums of
//                   mix(seed + (position << 8 | byte)) (four with revcomp: the
//                   reverse complement's, or with pairs the sums under the
//                   second mate's seeds).  A record's partial sums of one chunk
//                   are added once: to the tile's LDS cells of that record
//                   (u64, flushed to the record's global cells once per tile),
//                   or, past ST_KCAP records of one tile, straight to the
//                   global cells.  Sums mod 2^64 in any order give the same
//                   bits.
//   k_dedup_fold    one lane per unit: the length terms (from the record ends,
//                   so an empty record gets its key without owning a base),
//                   mates and strands folded into the unit's key.
//   k_dedup_insert  one lane per unit, wait-free.  A slot's key sits in three
//                   words that start 0 (empty): the key words shifted right by
//                   one with bit 63 set (never 0), and a tag holding the two
//                   bits shifted out (never 0).  A lane claims them in turn
//                   with atomicCAS; a word that already holds another value
//                   sends the lane to the next slot.  Only lanes whose earlier
//                   words equal the slot's reach a later word, so whoever wins
//                   each word the slot ends holding exactly one unit's full
//                   key, and no lane ever waits for another lane's store.  The
//                   lane whose three words match owns the slot: atomicMin on
//                   `first`, atomicAdd on `count`.  At most `slots` probes; a
//                   key without a slot sets a flag the entry point reports.
//   k_dedup_pick    a later launch on the same stream (every insert of the
//                   block has landed): a unit is the first of its key when
//                   first[slot] is its own number.
// The selected records are then compacted by nm_compact (name_match.hip).
//   k_dedup_levels  one pass over the slots: the histogram of the counts (LDS
//                   partials, then global), the keys and the largest count.
// No stream is read outside [0, seq_len): load16 reads a chunk that is not
// wholly inside byte by byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/fqz5_fastq.h"
#include "gpu_ctx.hpp"
#include "record_tile.hpp"

namespace fqz5 {
GpuCtx &gpu();
void fqz5_set_error(const char *msg);

namespace {

using u64 = unsigned long long;
static_assert(sizeof(u64) == sizeof(uint64_t), "u64");

constexpr uint32_t DD_PAIRS = 1, DD_REVCOMP = 2;             // the modes' bits
constexpr uint32_t DD_LEVELS = FQZ5_DEDUP_LEVELS;
constexpr uint64_t DD_MAX_SLOTS = 1ull << 31;                // (slot numbers are u32, NM_NONE none)

struct Slot {                                   // 32 bytes: two to a 64-byte line
    u64 lo, hi;                                 // (word >> 1) | 1 << 63; 0: not yet claimed
    u64 first;                                  // the smallest unit number; starts all ones
    uint32_t count;
    uint32_t tag;                               // 4 | (lo & 1) << 1 | (hi & 1); 0: not yet claimed
};
static_assert(sizeof(Slot) == 32, "Slot");

__host__ __device__ inline u64 mix(u64 x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
__host__ __device__ inline u64 seed_of(uint32_t s) {
    return s == 0 ? FQZ5_DEDUP_SEED0 : s == 1 ? FQZ5_DEDUP_SEED1
         : s == 2 ? FQZ5_DEDUP_SEED2 : FQZ5_DEDUP_SEED3;
}
__host__ __device__ inline uint32_t comp(uint32_t c) {
    switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'a': return 't';
    case 't': return 'a';
    case 'c': return 'g';
    case 'g': return 'c';
    default: return c;
    }
}
// the sums a record keeps under a mode: two, or with revcomp four
__host__ __device__ inline uint32_t sums_of(uint32_t mode) { return mode & DD_REVCOMP ? 4 : 2; }

// Byte c at position i of record r (L bases) into the record's sums:
//   plain          K_0, K_1
//   pairs          K_0, K_1 of an even record, K_2, K_3 of an odd one
//   revcomp        K_0, K_1, and K_0, K_1 of the reverse complement
//   both           K_0 .. K_3
template <uint32_t MODE>
__host__ __device__ inline void add_terms(u64 *acc, uint32_t odd, u64 i, u64 lm1, uint32_t c) {
    const u64 x = i << 8 | c;
    if (MODE == DD_PAIRS) {
        acc[0] += mix(seed_of(2 * odd) + x);
        acc[1] += mix(seed_of(2 * odd + 1) + x);
        return;
    }
    acc[0] += mix(FQZ5_DEDUP_SEED0 + x);
    acc[1] += mix(FQZ5_DEDUP_SEED1 + x);
    if (MODE == DD_REVCOMP) {
        const u64 y = (lm1 - i) << 8 | comp(c);
        acc[2] += mix(FQZ5_DEDUP_SEED0 + y);
        acc[3] += mix(FQZ5_DEDUP_SEED1 + y);
    } else if (MODE == (DD_PAIRS | DD_REVCOMP)) {
        acc[2] += mix(FQZ5_DEDUP_SEED2 + x);
        acc[3] += mix(FQZ5_DEDUP_SEED3 + x);
    }
}

__host__ __device__ inline bool key_less(u64 alo, u64 ahi, u64 blo, u64 bhi) {
    return alo < blo || (alo == blo && ahi < bhi);
}

// Unit u's key from the records' sums (sums[j * nrec + r], without their
// length terms) and ends.
__host__ __device__ inline void fold_unit(uint32_t mode, const u64 *sums, const uint64_t *end,
                                          uint64_t nrec, uint64_t u, u64 *lo, u64 *hi) {
    const auto len = [&](uint64_t r) { return u64(end[r] - (r ? end[r - 1] : 0)); };
    // K_s of record r kept in sum j
    const auto K = [&](uint32_t j, uint32_t s, uint64_t r) {
        return sums[j * nrec + r] + mix(seed_of(s) ^ len(r));
    };
    if (mode == 0) {
        *lo = K(0, 0, u);
        *hi = K(1, 1, u);
    } else if (mode == DD_PAIRS) {
        *lo = K(0, 0, 2 * u) + K(0, 2, 2 * u + 1);
        *hi = K(1, 1, 2 * u) + K(1, 3, 2 * u + 1);
    } else if (mode == DD_REVCOMP) {
        const u64 flo = K(0, 0, u), fhi = K(1, 1, u), rlo = K(2, 0, u), rhi = K(3, 1, u);
        const bool f = !key_less(rlo, rhi, flo, fhi);
        *lo = f ? flo : rlo;
        *hi = f ? fhi : rhi;
    } else {
        const uint64_t a = 2 * u, b = 2 * u + 1;
        const u64 flo = K(0, 0, a) + K(2, 2, b), fhi = K(1, 1, a) + K(3, 3, b);
        const u64 rlo = K(0, 0, b) + K(2, 2, a), rhi = K(1, 1, b) + K(3, 3, a);
        const bool f = !key_less(rlo, rhi, flo, fhi);
        *lo = f ? flo : rlo;
        *hi = f ? fhi : rhi;
    }
}

template <uint32_t MODE>
__global__ __launch_bounds__(ST_THREADS) void k_dedup_keys(const uint8_t *seq, uint64_t seq_len,
                                                           const uint64_t *end, const uint32_t *tf,
                                                           uint32_t nrec, uint64_t tile_a,
                                                           uint64_t tile_b, u64 *sums) {
    constexpr uint32_t NS = MODE & DD_REVCOMP ? 4 : 2;
    __shared__ uint32_t lend[ST_KCAP];
    __shared__ u64 lsum[NS * ST_KCAP];          // [sum][record of the tile]
    for (uint32_t i = threadIdx.x; i < NS * ST_KCAP; i += ST_THREADS) lsum[i] = 0;
    for (uint64_t t = tile_a + blockIdx.x; t < tile_b; t += gridDim.x) {
        Tile T;
        T.open(end, tf, nrec, seq_len, t, lend);
        __syncthreads();                        // (the last tile's flush has read lsum)
        T.stage(lend);
        __syncthreads();
        tile_chunks(T, seq, [&](int64_t a) {
            const uint4 v = load16(seq, seq_len, a);
            ChunkWalk W(T, a);
            u64 acc[NS];
#pragma unroll
            for (uint32_t j = 0; j < NS; j++) acc[j] = 0;
            uint32_t cur = NM_NONE, odd = 0;    // the record the walk stands in
            u64 lm1 = 0;                        // its length - 1 (revcomp alone reads it)
            W.bytes(T, a, v, [&](uint32_t q, uint32_t k, uint32_t c, int) {
                if (k != cur) {
                    cur = k;
                    odd = (T.r0 + k) & 1u;
                    // W.st is the record's true start: a record that owns a byte
                    // of the tile starts at start0 or at an unclipped end
                    if (MODE == DD_REVCOMP)
                        lm1 = u64(int64_t(T.end[T.r0 + k]) - int64_t(T.t0) - W.st) - 1;
                }
                add_terms<MODE>(acc, odd, u64(int64_t(q) - W.st), lm1, c);
            }, [&](uint32_t rec) {
#pragma unroll
                for (uint32_t j = 0; j < NS; j++) {
                    if (!acc[j]) continue;
                    if (rec < ST_KCAP) atomicAdd(&lsum[j * ST_KCAP + rec], acc[j]);
                    else atomicAdd(sums + uint64_t(j) * nrec + T.r0 + rec, acc[j]);
                    acc[j] = 0;
                }
            });
        });
        __syncthreads();
        const uint32_t k1 = T.nrt < ST_KCAP ? T.nrt : ST_KCAP;
        for (uint32_t k = threadIdx.x; k < k1; k += ST_THREADS) {
#pragma unroll
            for (uint32_t j = 0; j < NS; j++) {
                const u64 x = lsum[j * ST_KCAP + k];
                if (!x) continue;
                atomicAdd(sums + uint64_t(j) * nrec + T.r0 + k, x);
                lsum[j * ST_KCAP + k] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(ST_THREADS) void k_dedup_fold(uint32_t mode, const u64 *sums,
                                                           const uint64_t *end, uint32_t nrec,
                                                           uint32_t units, u64 *keys) {
    for (uint64_t u = uint64_t(blockIdx.x) * ST_THREADS + threadIdx.x; u < units;
         u += uint64_t(gridDim.x) * ST_THREADS)
        fold_unit(mode, sums, end, nrec, u, keys + 2 * u, keys + 2 * u + 1);
}

__global__ __launch_bounds__(ST_THREADS) void k_dedup_clear(Slot *tab, uint64_t slots) {
    for (uint64_t s = uint64_t(blockIdx.x) * ST_THREADS + threadIdx.x; s < slots;
         s += uint64_t(gridDim.x) * ST_THREADS)
        tab[s] = Slot{0, 0, ~0ull, 0, 0};
}

__global__ __launch_bounds__(ST_THREADS) void k_dedup_insert(Slot *tab, uint64_t slots,
                                                             const u64 *keys, uint32_t n,
                                                             uint64_t first_unit, uint32_t *slot_of,
                                                             uint32_t *full) {
    const uint64_t mask = slots - 1;
    for (uint64_t u = uint64_t(blockIdx.x) * ST_THREADS + threadIdx.x; u < n;
         u += uint64_t(gridDim.x) * ST_THREADS) {
        const u64 lo = keys[2 * u], hi = keys[2 * u + 1];
        const u64 wlo = lo >> 1 | 1ull << 63, whi = hi >> 1 | 1ull << 63;
        const uint32_t tag = 4u | uint32_t(lo & 1) << 1 | uint32_t(hi & 1);
        uint32_t mine = NM_NONE;
        uint64_t s = lo & mask;
        for (uint64_t probe = 0; probe < slots; probe++, s = (s + 1) & mask) {
            Slot *p = tab + s;
            const u64 a = atomicCAS(&p->lo, 0ull, wlo);
            if (a != 0 && a != wlo) continue;
            const u64 b = atomicCAS(&p->hi, 0ull, whi);
            if (b != 0 && b != whi) continue;
            const uint32_t c = atomicCAS(&p->tag, 0u, tag);
            if (c != 0 && c != tag) continue;
            atomicMin(&p->first, u64(first_unit + u));
            atomicAdd(&p->count, 1u);
            mine = uint32_t(s);
            break;
        }
        if (mine == NM_NONE) atomicOr(full, 1u);
        slot_of[u] = mine;
    }
}

// hit[r] = 0 where record r is selected, NM_NONE where not (nm_compact's input)
__global__ __launch_bounds__(ST_THREADS) void k_dedup_pick(const Slot *tab, const uint32_t *slot_of,
                                                           uint32_t units, uint32_t mates,
                                                           uint64_t first_unit, int invert,
                                                           uint32_t *hit, u64 *first_out) {
    for (uint64_t u = uint64_t(blockIdx.x) * ST_THREADS + threadIdx.x; u < units;
         u += uint64_t(gridDim.x) * ST_THREADS) {
        const uint32_t s = slot_of[u];
        const u64 f = s == NM_NONE ? ~0ull : tab[s].first;   // (none: the call fails)
        const uint32_t h = ((f == first_unit + u) != (invert != 0)) && s != NM_NONE ? 0u : NM_NONE;
        for (uint32_t m = 0; m < mates; m++) hit[uint32_t(u) * mates + m] = h;
        if (first_out) first_out[u] = f;
    }
}

// out: [c] the slots with count c (1024 and more in [1024]), [1025] the
// occupied slots, [1026] the largest count
__global__ __launch_bounds__(ST_THREADS) void k_dedup_levels(const Slot *tab, uint64_t slots,
                                                             u64 *out) {
    __shared__ uint32_t hist[DD_LEVELS];        // (a workgroup sees fewer than 2^32 slots)
    __shared__ uint32_t top;
    for (uint32_t i = threadIdx.x; i < DD_LEVELS; i += ST_THREADS) hist[i] = 0;
    if (!threadIdx.x) top = 0;
    __syncthreads();
    for (uint64_t s = uint64_t(blockIdx.x) * ST_THREADS + threadIdx.x; s < slots;
         s += uint64_t(gridDim.x) * ST_THREADS) {
        const uint32_t c = tab[s].count;
        if (!c) continue;
        atomicAdd(&hist[c < DD_LEVELS - 1 ? c : DD_LEVELS - 1], 1u);
        atomicMax(&top, c);
    }
    __syncthreads();
    u64 mine = 0;
    for (uint32_t i = threadIdx.x; i < DD_LEVELS; i += ST_THREADS) {
        if (!hist[i]) continue;
        atomicAdd(out + i, u64(hist[i]));
        mine += hist[i];
    }
    if (mine) atomicAdd(out + DD_LEVELS, mine);
    if (!threadIdx.x && top) atomicMax(out + DD_LEVELS + 1, u64(top));
}

uint64_t slots_for(uint64_t units) {            // 0: too many
    if (units > DD_MAX_SLOTS / 2) return 0;
    uint64_t s = 8;
    while (s < 2 * units) s <<= 1;
    return s;
}

uint32_t grid_for(const GpuCtx &g, uint64_t n) {
    return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>((n + ST_THREADS - 1) / ST_THREADS,
                                                             4ull * g.cus)));
}

uint32_t mode_of(int pairs, int revcomp) {
    return (pairs ? DD_PAIRS : 0) | (revcomp ? DD_REVCOMP : 0);
}

// the block's unit keys into d_keys (2 * units words, device), queued on g's stream
void keys_device(GpuCtx &g, const uint8_t *d_seq, uint64_t seq_len,
                 const std::vector<uint64_t> &end, uint32_t mode, u64 *d_keys) {
    const uint32_t n = uint32_t(end.size()), ns = sums_of(mode);
    const uint32_t units = n / (mode & DD_PAIRS ? 2 : 1);
    u64 *sums = g.arena.alloc_n<u64>(size_t(ns) * n);
    g.memset0(sums, size_t(ns) * n * sizeof(u64));
    const uint64_t *d_end = g.upload(end);
    const uint64_t tiles = (seq_len + ST_TILE - 1) / ST_TILE;
    if (tiles) {
        const uint32_t *d_tf = g.upload(tile_first(end, tiles));
        for (uint64_t a = 0; a < tiles; a += ST_LAUNCH_TILES) {
            const uint64_t b = std::min(tiles, a + ST_LAUNCH_TILES);
            const uint32_t grid = uint32_t(std::min<uint64_t>(b - a, 4ull * g.cus));
            const auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(ST_THREADS), 0, g.stream, d_seq, seq_len,
                                   d_end, d_tf, n, a, b, sums);
            };
            switch (mode) {
            case 0: launch(k_dedup_keys<0>); break;
            case DD_PAIRS: launch(k_dedup_keys<DD_PAIRS>); break;
            case DD_REVCOMP: launch(k_dedup_keys<DD_REVCOMP>); break;
            default: launch(k_dedup_keys<DD_PAIRS | DD_REVCOMP>); break;
            }
            FQZ5_HIP(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_dedup_fold, dim3(grid_for(g, units)), dim3(ST_THREADS), 0, g.stream, mode,
                       sums, d_end, n, units, d_keys);
    FQZ5_HIP(hipGetLastError());
}

struct KeyHash {
    size_t operator()(const std::pair<uint64_t, uint64_t> &k) const {
        return size_t(k.first ^ (k.second * 0x9E3779B97F4A7C15ull));
    }
};

void levels_add(uint64_t *out, uint64_t count) {
    out[count < DD_LEVELS - 1 ? count : DD_LEVELS - 1]++;
    out[DD_LEVELS]++;
    out[DD_LEVELS + 1] = std::max(out[DD_LEVELS + 1], count);
}

}  // namespace
}  // namespace fqz5

using namespace fqz5;

struct fqz5_dedup_table {
    Slot *tab = nullptr;
    uint32_t *full = nullptr;                   // device flag: a key found no slot
    uint64_t slots = 0;
};

struct fqz5_dedup_host_table {
    struct Entry { uint64_t first, count; };
    std::unordered_map<std::pair<uint64_t, uint64_t>, Entry, KeyHash> map;
};

namespace {

void insert_device(GpuCtx &g, fqz5_dedup_table *t, const u64 *d_keys, uint32_t n,
                   uint64_t first_unit, uint32_t *d_slot) {
    g.memset0(t->full, sizeof(uint32_t));
    hipLaunchKernelGGL(k_dedup_insert, dim3(grid_for(g, n)), dim3(ST_THREADS), 0, g.stream, t->tab,
                       t->slots, d_keys, n, first_unit, d_slot, t->full);
    FQZ5_HIP(hipGetLastError());
}

void clear_device(GpuCtx &g, fqz5_dedup_table *t) {
    hipLaunchKernelGGL(k_dedup_clear, dim3(grid_for(g, t->slots)), dim3(ST_THREADS), 0, g.stream,
                       t->tab, t->slots);
    FQZ5_HIP(hipGetLastError());
    g.memset0(t->full, sizeof(uint32_t));
    g.sync();
}

}  // namespace

extern "C" {

uint64_t fqz5_dedup_table_bytes(uint64_t units) { return slots_for(units) * sizeof(Slot); }

fqz5_dedup_table *fqz5_dedup_table_new(uint64_t units) {
    fqz5_dedup_table *t = nullptr;
    try {
        const uint64_t slots = slots_for(units);
        if (!slots) throw GpuError("dedup_table_new: more than 2^31 slots");
        GpuCtx &g = gpu();
        t = new fqz5_dedup_table();
        t->slots = slots;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&t->tab), slots * sizeof(Slot));
        if (e != hipSuccess) {                  // the pool's idle chunks back to the device, once more
            ChunkPool::get().trim(0);
            e = hipMalloc(reinterpret_cast<void **>(&t->tab), slots * sizeof(Slot));
        }
        if (e != hipSuccess) {
            t->tab = nullptr;
            throw GpuError("dedup_table_new: no device memory for a table of " +
                           std::to_string(slots * sizeof(Slot)) + " bytes");
        }
        FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&t->full), 256));
        clear_device(g, t);
        return t;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        fqz5_dedup_table_free(t);
        return nullptr;
    }
}

void fqz5_dedup_table_free(fqz5_dedup_table *t) {
    if (!t) return;
    if (t->tab) (void)hipFree(t->tab);
    if (t->full) (void)hipFree(t->full);
    delete t;
}

uint64_t fqz5_dedup_table_slots(const fqz5_dedup_table *t) { return t ? t->slots : 0; }

int fqz5_dedup_table_reset(fqz5_dedup_table *t) {
    try {
        if (!t) throw GpuError("dedup_table_reset: no table");
        clear_device(gpu(), t);
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

int fqz5_dedup_table_slot(const fqz5_dedup_table *t, uint64_t slot, uint64_t *out) {
    try {
        if (!t || slot >= t->slots) throw GpuError("dedup_table_slot: no such slot");
        GpuCtx &g = gpu();
        Slot s;
        FQZ5_HIP(hipMemcpyAsync(&s, t->tab + slot, sizeof(Slot), hipMemcpyDeviceToHost, g.stream));
        g.sync();
        out[0] = s.count ? (s.lo << 1 | (s.tag >> 1 & 1)) : 0;
        out[1] = s.count ? (s.hi << 1 | (s.tag & 1)) : 0;
        out[2] = s.first;
        out[3] = s.count;
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

int fqz5_dedup_keys(const uint8_t *d_seq, uint64_t seq_len, const uint32_t *h_len, uint64_t nrec,
                    int pairs, int revcomp, uint64_t *d_keys) {
    GpuCtx *gp = nullptr;
    try {
        check_records(nrec, pairs, "dedup_keys");
        const std::vector<uint64_t> end = record_ends(h_len, nrec, seq_len, "dedup_keys");
        if (!nrec) return 0;
        GpuCtx &g = gpu();
        gp = &g;
        keys_device(g, d_seq, seq_len, end, mode_of(pairs, revcomp), reinterpret_cast<u64 *>(d_keys));
        g.reset();
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { if (gp) gp->reset(); } catch (...) {}
        return -1;
    }
}

int fqz5_dedup_insert_keys(fqz5_dedup_table *t, const uint64_t *d_keys, uint64_t n,
                           uint64_t first_unit, uint32_t *d_slot) {
    GpuCtx *gp = nullptr;
    uint32_t full = 0;                          // (outlives the try: a copy lands here)
    try {
        if (!t) throw GpuError("dedup_insert_keys: no table");
        if (n >= (1ull << 31)) throw GpuError("dedup_insert_keys: block too large");
        if (!n) return 0;
        GpuCtx &g = gpu();
        gp = &g;
        insert_device(g, t, reinterpret_cast<const u64 *>(d_keys), uint32_t(n), first_unit, d_slot);
        g.download(&full, t->full, 1);
        g.reset();
        if (full) throw GpuError("dedup_insert_keys: table full (" + std::to_string(t->slots) +
                                 " slots)");
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { if (gp) gp->reset(); } catch (...) {}
        return -1;
    }
}

int fqz5_dedup_match(fqz5_dedup_table *t, const uint8_t *d_seq, uint64_t seq_len,
                     const uint32_t *h_len, uint64_t nrec, int pairs, int revcomp, int invert,
                     uint64_t first_unit, uint32_t *d_rec, uint64_t *n_hit, uint64_t *d_first) {
    GpuCtx *gp = nullptr;
    uint32_t full = 0;                          // (outlives the try: a copy lands here)
    try {
        *n_hit = 0;
        if (!t) throw GpuError("dedup_match: no table");
        check_records(nrec, pairs, "dedup_match");
        const std::vector<uint64_t> end = record_ends(h_len, nrec, seq_len, "dedup_match");
        if (!nrec) return 0;
        GpuCtx &g = gpu();
        gp = &g;
        const uint32_t n = uint32_t(nrec), mates = pairs ? 2 : 1, units = n / mates;
        u64 *keys = g.arena.alloc_n<u64>(2 * size_t(units));
        uint32_t *slot = g.arena.alloc_n<uint32_t>(units);
        uint32_t *hit = g.arena.alloc_n<uint32_t>(n);
        uint32_t *query = g.arena.alloc_n<uint32_t>(n);
        keys_device(g, d_seq, seq_len, end, mode_of(pairs, revcomp), keys);
        insert_device(g, t, keys, units, first_unit, slot);
        hipLaunchKernelGGL(k_dedup_pick, dim3(grid_for(g, units)), dim3(ST_THREADS), 0, g.stream,
                           t->tab, slot, units, mates, first_unit, invert, hit,
                           reinterpret_cast<u64 *>(d_first));
        FQZ5_HIP(hipGetLastError());
        g.download(&full, t->full, 1);
        const uint64_t got = nm_compact(g, hit, n, 0, d_rec, query);   // (synchronises: `full` is here)
        g.reset();
        if (full) throw GpuError("dedup_match: table full (" + std::to_string(t->slots) + " slots)");
        *n_hit = got;
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { if (gp) gp->reset(); } catch (...) {}
        return -1;
    }
}

int fqz5_dedup_levels(const fqz5_dedup_table *t, uint64_t *h_out) {
    GpuCtx *gp = nullptr;
    try {
        if (!t) throw GpuError("dedup_levels: no table");
        GpuCtx &g = gpu();
        gp = &g;
        u64 *out = g.arena.alloc_n<u64>(FQZ5_DEDUP_LEVEL_WORDS);
        g.memset0(out, FQZ5_DEDUP_LEVEL_WORDS * sizeof(u64));
        hipLaunchKernelGGL(k_dedup_levels, dim3(grid_for(g, t->slots)), dim3(ST_THREADS), 0, g.stream,
                           t->tab, t->slots, out);
        FQZ5_HIP(hipGetLastError());
        g.download(reinterpret_cast<u64 *>(h_out), out, FQZ5_DEDUP_LEVEL_WORDS);
        g.reset();
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { if (gp) gp->reset(); } catch (...) {}
        return -1;
    }
}

int fqz5_dedup_keys_host(const uint8_t *seq, uint64_t seq_len, const uint32_t *lens, uint64_t nrec,
                         int pairs, int revcomp, uint64_t *keys) {
    try {
        check_records(nrec, pairs, "dedup_keys_host");
        const std::vector<uint64_t> end = record_ends(lens, nrec, seq_len, "dedup_keys_host");
        const uint32_t mode = mode_of(pairs, revcomp), ns = sums_of(mode);
        std::vector<u64> sums(size_t(ns) * size_t(nrec), 0);
        uint64_t at = 0;
        for (uint64_t r = 0; r < nrec; r++) {
            const uint64_t L = lens[r];
            u64 acc[4] = {0, 0, 0, 0};
            for (uint64_t i = 0; i < L; i++) {
                const uint32_t c = seq[at + i];
                switch (mode) {
                case 0: add_terms<0>(acc, 0, i, 0, c); break;
                case DD_PAIRS: add_terms<DD_PAIRS>(acc, uint32_t(r & 1), i, 0, c); break;
                case DD_REVCOMP: add_terms<DD_REVCOMP>(acc, 0, i, L - 1, c); break;
                default: add_terms<DD_PAIRS | DD_REVCOMP>(acc, 0, i, 0, c); break;
                }
            }
            for (uint32_t j = 0; j < ns; j++) sums[size_t(j) * size_t(nrec) + size_t(r)] = acc[j];
            at += L;
        }
        const uint64_t units = nrec / (pairs ? 2 : 1);
        for (uint64_t u = 0; u < units; u++) {
            u64 lo, hi;
            fold_unit(mode, sums.data(), end.data(), nrec, u, &lo, &hi);
            keys[2 * u] = lo;
            keys[2 * u + 1] = hi;
        }
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

fqz5_dedup_host_table *fqz5_dedup_host_new(void) {
    try {
        return new fqz5_dedup_host_table();
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return nullptr;
    }
}

void fqz5_dedup_host_free(fqz5_dedup_host_table *t) { delete t; }

int fqz5_dedup_host_add(fqz5_dedup_host_table *t, const uint64_t *keys, uint64_t n,
                        uint64_t first_unit, int invert, uint8_t *keep, uint64_t *first) {
    try {
        if (!t) throw GpuError("dedup_host_add: no table");
        // every key of the call lands before any unit is judged, as on the device
        for (uint64_t u = 0; u < n; u++) {
            auto it = t->map.emplace(std::make_pair(keys[2 * u], keys[2 * u + 1]),
                                     fqz5_dedup_host_table::Entry{first_unit + u, 0}).first;
            it->second.first = std::min(it->second.first, first_unit + u);
            it->second.count++;
        }
        for (uint64_t u = 0; u < n; u++) {
            const uint64_t f = t->map.at(std::make_pair(keys[2 * u], keys[2 * u + 1])).first;
            if (keep) keep[u] = (f == first_unit + u) != (invert != 0);
            if (first) first[u] = f;
        }
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

int fqz5_dedup_host_levels(const fqz5_dedup_host_table *t, uint64_t *out) {
    try {
        if (!t) throw GpuError("dedup_host_levels: no table");
        std::fill(out, out + FQZ5_DEDUP_LEVEL_WORDS, uint64_t(0));
        for (const auto &kv : t->map) levels_add(out, kv.second.count);
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

}  // extern "C"
