// name_match.hpp — the query table of lookup by read name (name_match.hip):
// the hash the host builder and the device kernel share, and the table's
// slot rule.
//
// A key is hashed byte by byte (FNV-1a's step, so a lane of k_name_match
// carries the state across its staging windows) and mixed once at the key's
// end.  The mixed value's low bits give the first slot of the open-addressing
// probe, its top tag_bits the slot's tag.  A tag only spares byte
// comparisons: a match is decided by the bytes alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace fqz5 {

constexpr uint32_t NM_NONE = 0xFFFFFFFFu;       // no query / an empty slot
constexpr uint32_t NM_HASH0 = 2166136261u;      // the state before a key's first byte

// the state after byte c; with last: the key has ended, c is ignored and the
// state is mixed (murmur3's finaliser) into the value slots and tags come from
__host__ __device__ inline uint32_t nm_hash(uint32_t h, uint8_t c, bool last = false) {
    if (!last) return (h ^ c) * 16777619u;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

__host__ __device__ inline uint32_t nm_tag(uint32_t mixed, int tag_bits) {
    return tag_bits >= 32 ? mixed : mixed >> (32 - tag_bits);
}

// one slot: the tag in the low word, the query index (NM_NONE: empty) above
__host__ __device__ inline uint64_t nm_slot(uint32_t tag, uint32_t query) {
    return uint64_t(query) << 32 | tag;
}

struct GpuCtx;

// name_match.hip: the compaction both matchers end with.  hit[0..n) holds
// per record a query index or NM_NONE; the records to report (a hit, or with
// pairs the mate of one) go, ascending, into d_rec with their hit[] value in
// d_query (a flag kernel, an exclusive scan, a scatter).  Returns their number
// after synchronising g's stream; scratch comes from g's arena.
uint32_t nm_compact(GpuCtx &g, const uint32_t *hit, uint32_t n, int pairs, uint32_t *d_rec,
                    uint32_t *d_query);

// seq_match.hip: where each of a block's records ends in its base array (the
// inclusive scan of the lengths: record r holds the positions below end[r]),
// for the sequence matcher and the statistics (stats.hip);
// throws GpuError("<who>: the record lengths do not sum to the bases") unless
// the last end is seq_len.
std::vector<uint64_t> record_ends(const uint32_t *lens, uint64_t nrec, uint64_t seq_len,
                                  const char *who);

}  // namespace fqz5
