// name_match.hip — lookup by read name (fqz5file.find_names /
// extract_names_file): which records of a decoded name section belong to a
// set of query names.
//
// The queries sit in an open-addressing table built on the host
// (fqz5_names_table_build): capacity a power of two of at least twice the
// queries, each slot {tag, query index}, linear probing, the hash of
// name_match.hpp.  k_name_match hashes every record's key (whole = 0: the
// name up to the first ' ' or '\t', kseq's name; else the whole header line),
// probes the table and, where a tag agrees, compares the key's bytes with the
// query's: equal tags never decide.  The hits are compacted on the device (a
// scan and a scatter) into ascending record indices with their query
// indices; pairs adds the mate of every hit (records 2k and 2k + 1).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/fqz5_fastq.h"
#include "gpu_ctx.hpp"
#include "name_match.hpp"

namespace fqz5 {
GpuCtx &gpu();
void fqz5_set_error(const char *msg);
// fastq.hip: the positions of every `ch` byte of d_text[0..len), in order
uint64_t *fastq_find_delims(GpuCtx &g, const uint8_t *d_text, uint64_t len, uint8_t ch,
                            uint64_t *count);
}  // namespace fqz5

// the queries ('\0' after each), their offsets (nq + 1) and the slots; the
// device copies are made by the first fqz5_names_match and freed with the table
struct fqz5_name_table {
    std::vector<uint8_t> q;
    std::vector<uint64_t> qoff;
    std::vector<uint64_t> slots;
    uint32_t mask = 0;
    int tag_bits = 32;
    std::mutex m;
    int device = -1;
    uint8_t *d_q = nullptr;
    uint64_t *d_qoff = nullptr, *d_slots = nullptr;
};

namespace fqz5 {
namespace {

constexpr uint32_t NM_WIN = 8192;               // bytes of the LDS staging window

struct NmDev {                                  // the table as the kernel reads it
    const uint64_t *slots;
    const uint8_t *q;
    const uint64_t *qoff;
    uint32_t mask;
    int tag_bits;
};

// One wave per 64 consecutive records (the shape of k_fqz_ev_fill,
// fqz_kernels.hip): their names are one contiguous byte range of the
// section, which the wave stages window by window into LDS with coalesced
// 16-byte loads (a thread per record reading its own bytes would touch 64
// lines with every load).  Each lane walks its own record's key through the
// windows (its position, the hash state and the key length carry from one
// window to the next, so a key may span any number of them), then probes the
// table; only on a tag match does it read the key again, from the section,
// against the query's bytes.  zpos: the section's '\0' positions.
__global__ __launch_bounds__(64) void k_name_match(const uint8_t *names, uint64_t name_len,
                                                   const uint64_t *zpos, uint32_t nrec, int whole,
                                                   NmDev T, uint32_t *hit) {
    __shared__ uint4 win4[NM_WIN / 16];
    const uint8_t *win = reinterpret_cast<const uint8_t *>(win4);
    const uint32_t lane = threadIdx.x;
    const uint32_t r0 = blockIdx.x * 64u, r = r0 + lane;
    const bool act = r < nrec;
    const uint32_t rend = min(r0 + 64u, nrec);
    const uint64_t B0 = r0 ? zpos[r0 - 1] + 1 : 0, B1 = zpos[rend - 1] + 1;
    const uint64_t s = act ? (r ? zpos[r - 1] + 1 : 0) : B1;      // the record's bytes [s, e)
    const uint64_t e = act ? zpos[r] : B1;
    // windows start where the address is a multiple of 16 (the section may
    // start anywhere in its buffer), so the first may start before offset 0
    const uint64_t mis = reinterpret_cast<uintptr_t>(names) & 15u;
    uint64_t p = s;
    uint32_t h = NM_HASH0, klen = 0;
    bool done = !act;
    for (int64_t w0 = int64_t(B0) - int64_t((B0 + mis) & 15u); w0 < int64_t(B1); w0 += NM_WIN) {
        for (uint32_t i = lane; i < NM_WIN / 16; i += 64u) {
            const int64_t a = w0 + 16 * int64_t(i);
            if (a >= int64_t(B1)) break;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (a >= 0 && uint64_t(a) + 16 <= name_len) {
                v = *reinterpret_cast<const uint4 *>(names + a);
            } else {
                uint32_t w[4] = {0, 0, 0, 0};
                for (int k = 0; k < 16; k++)
                    if (a + k >= 0 && uint64_t(a + k) < name_len)
                        w[k >> 2] |= uint32_t(names[a + k]) << (8 * (k & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            win4[i] = v;
        }
        __syncthreads();
        if (!done) {
            const uint64_t wfull = uint64_t(w0 + int64_t(NM_WIN));
            const uint64_t wend = wfull < B1 ? wfull : B1;
            const uint64_t stop = e < wend ? e : wend;
            while (p < stop) {
                const uint8_t c = win[p - w0];
                if (!whole && (c == ' ' || c == '\t')) {
                    done = true;
                    break;
                }
                h = nm_hash(h, c);
                klen++;
                p++;
            }
            if (p == e) done = true;
        }
        __syncthreads();
    }
    if (!act) return;
    uint32_t found = NM_NONE;
    if (klen) {                                  // (no query is empty)
        const uint32_t m = nm_hash(h, 0, true), tag = nm_tag(m, T.tag_bits);
        uint32_t sl = m & T.mask;
        for (uint32_t n = 0; n <= T.mask; n++, sl = (sl + 1) & T.mask) {
            const uint64_t ent = T.slots[sl];
            const uint32_t qi = uint32_t(ent >> 32);
            if (qi == NM_NONE) break;
            if (uint32_t(ent) != tag) continue;
            const uint64_t qa = T.qoff[qi];
            if (T.qoff[qi + 1] - 1 - qa != klen) continue;
            uint32_t i = 0;
            while (i < klen && names[s + i] == T.q[qa + i]) i++;
            if (i == klen) {
                found = qi;
                break;
            }
        }
    }
    hit[r] = found;
}

// the records to report: a hit, or (pairs) the mate of one; entry nrec is 0,
// so the exclusive scan over nrec + 1 entries ends with the count
__global__ void k_nm_flag(const uint32_t *hit, uint32_t nrec, int pairs, uint32_t *flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nrec) return;
    uint32_t f = 0;
    if (i < nrec) {
        f = hit[i] != NM_NONE;
        if (pairs && (i ^ 1u) < nrec) f |= hit[i ^ 1u] != NM_NONE;
    }
    flag[i] = f;
}

__global__ void k_nm_scatter(const uint32_t *flag, const uint32_t *pos, const uint32_t *hit,
                             uint32_t nrec, uint32_t *rec, uint32_t *query) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nrec && flag[i]) {
        rec[pos[i]] = i;
        query[pos[i]] = hit[i];
    }
}

// the first slot of the probe of `key` that holds it (its query index), or
// the empty slot that ends the probe (*at, the index NM_NONE)
uint32_t probe(const fqz5_name_table &T, const uint8_t *key, uint64_t len, uint32_t *at) {
    uint32_t h = NM_HASH0;
    for (uint64_t i = 0; i < len; i++) h = nm_hash(h, key[i]);
    const uint32_t m = nm_hash(h, 0, true), tag = nm_tag(m, T.tag_bits);
    for (uint32_t sl = m & T.mask;; sl = (sl + 1) & T.mask) {
        const uint64_t ent = T.slots[sl];
        const uint32_t qi = uint32_t(ent >> 32);
        if (at) *at = sl;
        if (qi == NM_NONE) return NM_NONE;
        if (uint32_t(ent) != tag) continue;
        const uint64_t qa = T.qoff[qi];
        if (T.qoff[qi + 1] - 1 - qa == len && !std::memcmp(T.q.data() + qa, key, len)) return qi;
    }
}

// the table on the calling thread's device (made once)
NmDev device_copy(fqz5_name_table &T) {
    std::lock_guard<std::mutex> lk(T.m);
    int dev = 0;
    FQZ5_HIP(hipGetDevice(&dev));
    if (!T.d_slots) {
        FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&T.d_q), T.q.size() + 1));
        FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&T.d_qoff), T.qoff.size() * 8));
        FQZ5_HIP(hipMalloc(reinterpret_cast<void **>(&T.d_slots), T.slots.size() * 8));
        if (!T.q.empty()) FQZ5_HIP(hipMemcpy(T.d_q, T.q.data(), T.q.size(), hipMemcpyHostToDevice));
        FQZ5_HIP(hipMemcpy(T.d_qoff, T.qoff.data(), T.qoff.size() * 8, hipMemcpyHostToDevice));
        FQZ5_HIP(hipMemcpy(T.d_slots, T.slots.data(), T.slots.size() * 8, hipMemcpyHostToDevice));
        T.device = dev;
    } else if (T.device != dev) {
        throw GpuError("names_match: the table was uploaded to another device");
    }
    return NmDev{T.d_slots, T.d_q, T.d_qoff, T.mask, T.tag_bits};
}

}  // namespace

uint32_t nm_compact(GpuCtx &g, const uint32_t *hit, uint32_t n, int pairs, uint32_t *d_rec,
                    uint32_t *d_query) {
    uint32_t *flag = g.arena.alloc_n<uint32_t>(size_t(n) + 1);
    uint32_t *pos = g.arena.alloc_n<uint32_t>(size_t(n) + 1);
    hipLaunchKernelGGL(k_nm_flag, dim3(n / 256 + 1), dim3(256), 0, g.stream, hit, n, pairs, flag);
    FQZ5_HIP(hipGetLastError());
    size_t tb = 0;
    FQZ5_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flag, pos, int(n + 1), g.stream));
    void *tmp = g.arena.alloc_n<uint8_t>(tb ? tb : 1);
    FQZ5_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, flag, pos, int(n + 1), g.stream));
    hipLaunchKernelGGL(k_nm_scatter, dim3(n / 256 + 1), dim3(256), 0, g.stream, flag, pos, hit, n,
                       d_rec, d_query);
    FQZ5_HIP(hipGetLastError());
    uint32_t cnt = 0;
    g.download(&cnt, pos + n, 1);
    g.sync();
    return cnt;
}

}  // namespace fqz5

using namespace fqz5;

extern "C" {

fqz5_name_table *fqz5_names_table_build(const uint8_t *q, uint64_t q_len, uint64_t nq,
                                        int tag_bits) {
    fqz5_name_table *T = nullptr;
    try {
        if (tag_bits < 1 || tag_bits > 32) throw GpuError("names_table_build: tag_bits not in 1..32");
        if (nq > (1ull << 30)) throw GpuError("names_table_build: more than 2^30 queries");
        T = new fqz5_name_table();
        T->tag_bits = tag_bits;
        T->q.assign(q, q + q_len);
        T->qoff.reserve(size_t(nq) + 1);
        uint64_t at = 0;
        for (uint64_t k = 0; k < nq; k++) {
            const void *z = at < q_len ? std::memchr(q + at, 0, q_len - at) : nullptr;
            if (!z) throw GpuError("names_table_build: fewer terminated queries than nq");
            T->qoff.push_back(at);
            at = uint64_t(static_cast<const uint8_t *>(z) - q) + 1;
        }
        T->qoff.push_back(at);
        if (at != q_len) throw GpuError("names_table_build: bytes after the last query");
        uint64_t cap = 2;
        while (cap < 2 * nq) cap <<= 1;
        T->mask = uint32_t(cap - 1);
        T->slots.assign(size_t(cap), nm_slot(0, NM_NONE));
        for (uint64_t k = 0; k < nq; k++) {
            const uint8_t *key = q + T->qoff[k];
            const uint64_t len = T->qoff[k + 1] - 1 - T->qoff[k];
            char msg[96];
            if (!len) {
                std::snprintf(msg, sizeof msg, "names_table_build: query %llu is empty",
                              static_cast<unsigned long long>(k));
                throw GpuError(msg);
            }
            uint32_t sl = 0;
            const uint32_t dup = probe(*T, key, len, &sl);
            if (dup != NM_NONE) {
                std::snprintf(msg, sizeof msg, "names_table_build: query %llu is a duplicate of query %u",
                              static_cast<unsigned long long>(k), dup);
                throw GpuError(msg);
            }
            uint32_t h = NM_HASH0;
            for (uint64_t i = 0; i < len; i++) h = nm_hash(h, key[i]);
            T->slots[sl] = nm_slot(nm_tag(nm_hash(h, 0, true), tag_bits), uint32_t(k));
        }
        return T;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        delete T;
        return nullptr;
    }
}

void fqz5_names_table_free(fqz5_name_table *T) {
    if (!T) return;
    if (T->d_q) (void)hipFree(T->d_q);
    if (T->d_qoff) (void)hipFree(T->d_qoff);
    if (T->d_slots) (void)hipFree(T->d_slots);
    delete T;
}

int64_t fqz5_names_table_find(const fqz5_name_table *T, const uint8_t *key, uint64_t len) {
    if (!T || !len) return -1;
    const uint32_t qi = probe(*T, key, len, nullptr);
    return qi == NM_NONE ? -1 : int64_t(qi);
}

uint32_t fqz5_names_match_window(void) { return NM_WIN; }

int fqz5_names_match(const fqz5_name_table *T, const uint8_t *d_names, uint64_t name_len,
                     uint64_t nrec, int whole, int pairs, uint32_t *d_rec, uint32_t *d_query,
                     uint64_t *n_hit) {
    GpuCtx *gp = nullptr;
    try {
        *n_hit = 0;
        if (!T) throw GpuError("names_match: no table");
        if (!nrec) return 0;
        if (nrec >= (1ull << 31)) throw GpuError("names_match: block too large");
        GpuCtx &g = gpu();
        gp = &g;
        const NmDev D = device_copy(*const_cast<fqz5_name_table *>(T));
        uint64_t nz = 0;
        const uint64_t *z = fastq_find_delims(g, d_names, name_len, 0, &nz);
        if (nz < nrec) throw GpuError("names_match: fewer names than records");
        const uint32_t n = uint32_t(nrec);
        uint32_t *hit = g.arena.alloc_n<uint32_t>(n);
        hipLaunchKernelGGL(k_name_match, dim3((n + 63) / 64), dim3(64), 0, g.stream, d_names, name_len,
                           z, n, whole, D, hit);
        FQZ5_HIP(hipGetLastError());
        const uint32_t cnt = nm_compact(g, hit, n, pairs, d_rec, d_query);
        *n_hit = cnt;
        g.reset();
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { if (gp) gp->reset(); } catch (...) {}
        return -1;
    }
}

}  // extern "C"
