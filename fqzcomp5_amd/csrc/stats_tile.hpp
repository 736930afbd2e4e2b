// stats_tile.hpp — the tile machinery the statistics (stats.hip) and the
// filter by read metrics (filter.hip) share: a block's bases cut into tiles of
// ST_TILE, each tile's first record (tf, merged on the host from the records'
// ends), the tile's record ends staged into LDS, and the 16-byte loads that
// never leave [0, seq_len).
//
// The record that owns a base comes from the records' ends: a lane searches
// the tile's ends once for the first byte of its 16-byte chunk (Tile::owner)
// and walks from there; equal ends (empty records) are stepped over and never
// own a base.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace fqz5 {

constexpr uint32_t ST_TILE = 4096;              // bases per tile
constexpr uint32_t ST_THREADS = 256;
constexpr uint32_t ST_KCAP = 2048;              // a tile's record ends kept in LDS
constexpr uint64_t ST_LAUNCH_TILES = (1ull << 31) / ST_TILE;   // bases per launch <= 2^31

__host__ __device__ inline uint32_t is_gc(uint32_t c) {
    const uint32_t f = c | 0x20u;
    return f == 'c' || f == 'g';
}

// the 16 bytes at s + a: one load where they lie wholly inside [0, len)
__device__ inline uint4 load16(const uint8_t *s, uint64_t len, int64_t a) {
    if (a >= 0 && uint64_t(a) + 16 <= len) return *reinterpret_cast<const uint4 *>(s + a);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int k = 0; k < 16; k++)
        if (a + k >= 0 && uint64_t(a + k) < len)
            w[k >> 2] |= uint32_t(s[a + k]) << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// One tile as its workgroup sees it: the records r0 .. r0 + nrt - 1 are those
// that can own one of its n bases; their ends, relative to the tile and
// clipped to ST_TILE, are in `lend` for the first ST_KCAP of them and read
// from the ends array beyond (tiles of more than 2048 records).
struct Tile {
    const uint64_t *end;
    const uint32_t *lend;
    uint64_t t0;
    uint32_t n, r0, nrt;
    int64_t start0;                             // where r0 starts, relative to the tile (<= 0)

    __device__ void open(const uint64_t *ends, const uint32_t *tf, uint32_t nrec, uint64_t seq_len,
                         uint64_t t, uint32_t *lds) {
        end = ends;
        lend = lds;
        t0 = t * ST_TILE;
        n = uint32_t(seq_len - t0 < ST_TILE ? seq_len - t0 : ST_TILE);
        r0 = tf[t];
        const uint32_t r1 = tf[t + 1] < nrec - 1 ? tf[t + 1] : nrec - 1;
        nrt = r1 - r0 + 1;
        start0 = int64_t(r0 ? ends[r0 - 1] : 0) - int64_t(t0);
    }
    // (all threads, then a barrier)
    __device__ void stage(uint32_t *lds) const {
        const uint32_t k1 = nrt < ST_KCAP ? nrt : ST_KCAP;
        for (uint32_t k = threadIdx.x; k < k1; k += ST_THREADS) {
            const uint64_t e = end[r0 + k] - t0;
            lds[k] = e < ST_TILE ? uint32_t(e) : ST_TILE;
        }
    }
    __device__ uint32_t relend(uint32_t k) const {
        if (k < ST_KCAP) return lend[k];
        const uint64_t e = end[r0 + k] - t0;
        return e < ST_TILE ? uint32_t(e) : ST_TILE;
    }
    // the record (index within the tile) that owns relative position q < n:
    // the first whose end lies past q, so never an empty one
    __device__ uint32_t owner(uint32_t q) const {
        uint32_t lo = 0, hi = nrt - 1;          // (relend(nrt - 1) >= n > q)
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (relend(mid) > q) hi = mid; else lo = mid + 1;
        }
        return lo;
    }
    __device__ int64_t start(uint32_t k) const { return k ? int64_t(relend(k - 1)) : start0; }
};

// a non-zero LDS cell into its u64 global cell
__device__ inline void flush_cell(uint64_t *g, uint32_t v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(g), static_cast<unsigned long long>(v));
}

// each tile's first record, the first whose end lies past the tile's start
// (tiles + 1 entries, the last nrec - 1); end: the records' ends, the last of
// them the number of bases, tiles = ceil(bases / ST_TILE) > 0
inline std::vector<uint32_t> tile_first(const std::vector<uint64_t> &end, uint64_t tiles) {
    std::vector<uint32_t> tf(size_t(tiles) + 1);
    uint32_t r = 0;
    for (uint64_t t = 0; t < tiles; t++) {
        while (end[r] <= t * ST_TILE) r++;
        tf[size_t(t)] = r;
    }
    tf[size_t(tiles)] = uint32_t(end.size() - 1);
    return tf;
}

}  // namespace fqz5
