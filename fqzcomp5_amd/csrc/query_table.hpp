// query_table.hpp — the query table of lookup by read name (name_match.hip)
// and by sequence content (seq_match.hip): the hash the host builder and the
// device kernels share, the table's slot rule, its builder, its device copy
// and the one probe all of them walk.
//
// A key is hashed byte by byte (FNV-1a's step, so a lane of k_name_match
// carries the state across its staging windows) and mixed once at the key's
// end.  The mixed value's low bits give the first slot of the open-addressing
// probe, its top tag_bits the slot's tag.  A tag only spares byte
// comparisons: a match is decided by the bytes alone.  A query's key is the
// whole query (key_len 0: names) or its first key_len bytes, the anchor
// (patterns): queries that share a key take separate slots of one probe.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "gpu_ctx.hpp"
#include "record_tile.hpp"

namespace fqz5 {

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

// the mixed hash of the m bytes at a
__host__ __device__ inline uint32_t nm_hash_of(const uint8_t *a, uint64_t m) {
    uint32_t h = NM_HASH0;
    for (uint64_t i = 0; i < m; i++) h = nm_hash(h, a[i]);
    return nm_hash(h, 0, true);
}

__host__ __device__ inline uint32_t nm_tag(uint32_t mixed, int tag_bits) {
    return tag_bits >= 32 ? mixed : mixed >> (32 - tag_bits);
}

// one slot: the tag in the low word, the query index (NM_NONE: empty) above
__host__ __device__ inline uint64_t nm_slot(uint32_t tag, uint32_t query) {
    return uint64_t(query) << 32 | tag;
}

// the table as a kernel or a host loop reads it: the queries ('\0' after
// each), their offsets (nq + 1) and the slots
struct QueryView {
    const uint64_t *slots;
    const uint8_t *q;
    const uint64_t *qoff;
    uint32_t mask, key_len;
    int tag_bits;
    __host__ __device__ uint64_t len(uint32_t qi) const { return qoff[qi + 1] - 1 - qoff[qi]; }
};

// The probe of a key whose mixed hash is `mixed`: from its first slot to the
// empty slot that ends it (or once around), verify(qi) for the query of every
// slot whose tag agrees, until one returns true.  Returns the slot it stopped
// at.
template <class Verify>
__host__ __device__ __forceinline__ uint32_t nm_probe(const QueryView &T, uint32_t mixed,
                                                       Verify verify) {
    const uint32_t tag = nm_tag(mixed, T.tag_bits);
    uint32_t sl = mixed & T.mask;
    for (uint32_t n = 0; n <= T.mask; n++, sl = (sl + 1) & T.mask) {
        const uint64_t ent = T.slots[sl];
        const uint32_t qi = uint32_t(ent >> 32);
        if (qi == NM_NONE || (uint32_t(ent) == tag && verify(qi))) break;
    }
    return sl;
}

// The table on the host, with the device copy the first match makes of it.
struct QueryTable {
    std::vector<uint8_t> q;
    std::vector<uint64_t> qoff, slots;
    uint32_t mask = 0, key_len = 0;
    int tag_bits = 32;
    std::mutex m;
    int device = -1;
    uint8_t *d_q = nullptr;
    uint64_t *d_qoff = nullptr, *d_slots = nullptr;

    ~QueryTable() {
        if (d_q) (void)hipFree(d_q);
        if (d_qoff) (void)hipFree(d_qoff);
        if (d_slots) (void)hipFree(d_slots);
    }
    QueryView host() const {
        return QueryView{slots.data(), q.data(), qoff.data(), mask, key_len, tag_bits};
    }
    // the table on the calling thread's device (made once)
    QueryView device_copy(const char *who) {
        std::lock_guard<std::mutex> lk(m);
        int dev = 0;
        FQZ5_HIP(hipGetDevice(&dev));
        if (!d_slots) {
            FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&d_q), q.size() + 1));
            FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&d_qoff), qoff.size() * 8));
            FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&d_slots), slots.size() * 8));
            if (!q.empty()) FQZ5_HIP(hipMemcpy(d_q, q.data(), q.size(), hipMemcpyHostToDevice));
            FQZ5_HIP(hipMemcpy(d_qoff, qoff.data(), qoff.size() * 8, hipMemcpyHostToDevice));
            FQZ5_HIP(hipMemcpy(d_slots, slots.data(), slots.size() * 8, hipMemcpyHostToDevice));
            device = dev;
        } else if (device != dev) {
            throw GpuError(std::string(who) + ": the table was uploaded to another device");
        }
        return QueryView{d_slots, d_q, d_qoff, mask, key_len, tag_bits};
    }
    // q[0..q_len) as nq queries, '\0' after each, none of them empty or longer
    // than `limit` bytes (0: any length); returns the shortest one's length.
    // noun, nouns: what the messages call a query ("pattern", "patterns").
    uint64_t parse(const uint8_t *q, uint64_t q_len, uint64_t nq, uint64_t limit, const char *who,
                   const char *noun, const char *nouns) {
        const std::string w = std::string(who) + ": ";
        this->q.assign(q, q + q_len);
        qoff.reserve(size_t(nq) + 1);
        uint64_t at = 0, shortest = UINT64_MAX;
        for (uint64_t k = 0; k < nq; k++) {
            const void *z = at < q_len ? std::memchr(q + at, 0, q_len - at) : nullptr;
            if (!z) throw GpuError(w + "fewer terminated " + nouns + " than nq");
            const uint64_t len = uint64_t(static_cast<const uint8_t *>(z) - q) - at;
            if (!len) throw GpuError(w + noun + " " + std::to_string(k) + " is empty");
            if (limit && len > limit)
                throw GpuError(w + noun + " " + std::to_string(k) + " is longer than " +
                               std::to_string(limit) + " bytes");
            shortest = len < shortest ? len : shortest;
            qoff.push_back(at);
            at += len + 1;
        }
        qoff.push_back(at);
        if (at != q_len) throw GpuError(w + "bytes after the last " + noun);
        return shortest;
    }
    // The slots of the parsed queries under key_len and tag_bits: a power of
    // two of at least twice the queries, linear probing.  A query equal to an
    // earlier one lies behind it in one probe (equal queries have equal keys):
    // it is refused where it would be inserted, so the message names the
    // lowest index that repeats and the first copy.
    void fill(const char *who, const char *noun) {
        const uint64_t nq = qoff.size() - 1;
        uint64_t cap = 2;
        while (cap < 2 * nq) cap <<= 1;
        mask = uint32_t(cap - 1);
        slots.assign(size_t(cap), nm_slot(0, NM_NONE));
        const QueryView V = host();
        for (uint64_t k = 0; k < nq; k++) {
            const uint8_t *key = V.q + V.qoff[k];
            const uint64_t len = V.len(uint32_t(k));
            const uint32_t mixed = nm_hash_of(key, key_len ? key_len : len);
            uint32_t dup = NM_NONE;
            const uint32_t sl = nm_probe(V, mixed, [&](uint32_t qi) {
                if (V.len(qi) == len && !std::memcmp(V.q + V.qoff[qi], key, size_t(len))) dup = qi;
                return dup != NM_NONE;
            });
            if (dup != NM_NONE)
                throw GpuError(std::string(who) + ": " + noun + " " + std::to_string(k) +
                               " is a duplicate of " + noun + " " + std::to_string(dup));
            slots[sl] = nm_slot(nm_tag(mixed, tag_bits), uint32_t(k));
        }
    }
};

}  // namespace fqz5
