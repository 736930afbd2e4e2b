// record_tile.hpp — a block's decoded streams as the record passes read them
// (name_match.hip, seq_match.hip, stats.hip, filter.hip): the 16-byte loads
// that never leave a stream, the records' ends, the checks on a block's
// record count, the compaction the lookups and the filter end with, and the
// tile walk of the statistics and the filter.
//
// The tile walk: a block's bases are cut into tiles of ST_TILE, each tile's
// first record (tile_first, merged on the host from the records' ends) and
// its record ends staged into LDS (Tile).  A stream is read in 16-byte chunks
// at 16-byte addresses (tile_chunks).  The record that owns a base comes from
// the records' ends: a lane searches the tile's ends once for the first byte
// of its chunk (ChunkWalk) and walks from there; equal ends (empty records)
// are stepped over and never own a base.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "gpu_ctx.hpp"

namespace fqz5 {

constexpr uint32_t NM_NONE = 0xFFFFFFFFu;       // no query / an empty slot / a record not selected
constexpr uint32_t ST_TILE = 4096;              // bases per tile
constexpr uint32_t ST_THREADS = 256;
constexpr uint32_t ST_KCAP = 2048;              // a tile's record ends kept in LDS
constexpr uint64_t ST_LAUNCH_TILES = (1ull << 31) / ST_TILE;   // bases per launch <= 2^31

// name_match.hip: the compaction the lookups and the filter end with.
// hit[0..n) holds per record a query index or NM_NONE; the records to report
// (a hit, or with pairs the mate of one) go, ascending, into d_rec with their
// hit[] value in d_query (a flag kernel, an exclusive scan, a scatter).
// Returns their number after synchronising g's stream; scratch comes from g's
// arena.
uint32_t nm_compact(GpuCtx &g, const uint32_t *hit, uint32_t n, int pairs, uint32_t *d_rec,
                    uint32_t *d_query);

// what every pass refuses of a block's record count
inline void check_records(uint64_t nrec, int pairs, const char *who) {
    if (nrec >= (1ull << 31)) throw GpuError(std::string(who) + ": block too large");
    if (pairs && (nrec & 1))
        throw GpuError(std::string(who) + ": an odd record count in a block of pairs");
}

// where each of a block's records ends in its base array (the inclusive scan
// of the lengths: record r holds the positions below end[r])
inline std::vector<uint64_t> record_ends(const uint32_t *lens, uint64_t nrec, uint64_t seq_len,
                                         const char *who) {
    std::vector<uint64_t> end(static_cast<size_t>(nrec));
    uint64_t at = 0;
    for (uint64_t r = 0; r < nrec; r++) end[size_t(r)] = at += lens[r];
    if (at != seq_len)
        throw GpuError(std::string(who) + ": the record lengths do not sum to the bases");
    return end;
}

// each tile's first record, the first whose end lies past the tile's start
// (tiles + 1 entries, the last nrec - 1); end: record_ends', the last of them
// the number of bases, tiles = ceil(bases / ST_TILE) > 0
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

__host__ __device__ inline uint32_t is_gc(uint32_t c) {
    const uint32_t f = c | 0x20u;
    return f == 'c' || f == 'g';
}

// the offset of the 16-byte address at or below s + at: where staging or a
// chunk loop that covers s[at] starts (s may start anywhere in its buffer,
// so this may lie before offset 0)
__device__ inline int64_t aligned_start(const uint8_t *s, uint64_t at) {
    return int64_t(at) - int64_t((reinterpret_cast<uintptr_t>(s) + at) & 15u);
}

// the 16 bytes at s + a: one load where they lie wholly inside [0, len),
// else byte by byte, never outside
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

// The chunk loop of one stream over an opened, staged tile: chunk(a) for the
// 16-byte chunks at s + a that hold a base of the tile, this lane's share of
// them (a is 16-byte aligned as an address, so the first may start before
// the tile and the last end after it).
template <class Chunk>
__device__ __forceinline__ void tile_chunks(const Tile &T, const uint8_t *s, Chunk chunk) {
    const int64_t tend = int64_t(T.t0) + T.n;
    for (int64_t a = aligned_start(s, T.t0) + 16 * int64_t(threadIdx.x); a < tend;
         a += 16 * int64_t(ST_THREADS))
        chunk(a);
}

// The byte walk of one chunk.  Constructed, it stands at the chunk's first
// position inside the tile, q0: record k of the tile owns it, which starts
// at st and ends at ek, both relative to the tile (ek clipped to ST_TILE).
// bytes() then calls byte(q, k, c, b) for every byte c of the chunk v that is
// one of the tile's, b its index in the chunk and q its position in the
// tile, with k, st and ek those of the record that owns it, and leave(k)
// each time the walk steps out of a record that owned a byte, the chunk's
// last one included.
struct ChunkWalk {
    uint32_t q0, k, ek;
    int64_t st;

    __device__ __forceinline__ ChunkWalk(const Tile &T, int64_t a) {
        const int64_t t0 = int64_t(T.t0);
        q0 = uint32_t((a > t0 ? a : t0) - t0);
        k = T.owner(q0);
        ek = T.relend(k);
        st = T.start(k);
    }
    template <class Byte, class Leave>
    __device__ __forceinline__ void bytes(const Tile &T, int64_t a, const uint4 &v, Byte byte,
                                          Leave leave) {
        const int64_t t0 = int64_t(T.t0), tend = t0 + T.n;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int b = 0; b < 16; b++) {
            const int64_t p = a + b;
            if (p < t0 || p >= tend) continue;
            const uint32_t q = uint32_t(p - t0);
            if (q >= ek) {
                leave(k);
                do {
                    st = int64_t(ek);
                    ek = T.relend(++k);
                } while (q >= ek);
            }
            byte(q, k, (w[b >> 2] >> (8 * (b & 3))) & 0xFFu, b);
        }
        leave(k);
    }
};

// a non-zero LDS cell into its u64 global cell
__device__ inline void flush_cell(uint64_t *g, uint32_t v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(g), static_cast<unsigned long long>(v));
}

// The tile's per-record sums in LDS, lsum[sum][record of the tile], to their
// global cells: put(j, r, x) for every non-zero sum j of block record r, the
// cell zeroed after it is read.  (All threads, after a barrier; the records
// past ST_KCAP of one tile add to the global cells themselves.)
template <uint32_t NSUM, class Put>
__device__ __forceinline__ void flush_records(const Tile &T, uint32_t *lsum, Put put) {
    const uint32_t k1 = T.nrt < ST_KCAP ? T.nrt : ST_KCAP;
    for (uint32_t k = threadIdx.x; k < k1; k += ST_THREADS) {
#pragma unroll
        for (uint32_t j = 0; j < NSUM; j++) {
            const uint32_t x = lsum[j * ST_KCAP + k];
            if (!x) continue;
            put(j, T.r0 + k, x);
            lsum[j * ST_KCAP + k] = 0;
        }
    }
}

}  // namespace fqz5
