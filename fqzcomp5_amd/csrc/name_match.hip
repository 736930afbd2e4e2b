// name_match.hip — lookup by read name (fqz5file.find_names /
// extract_names_file): which records of a decoded name section belong to a
// set of query names.
//
// The queries sit in an open-addressing table built on the host
// (fqz5_names_table_build: the table, hash and probe of query_table.hpp, the
// whole query its key).  k_name_match hashes every record's key (whole = 0:
// the name up to the first ' ' or '\t', kseq's name; else the whole header line),
// probes the table and, where a tag agrees, compares the key's bytes with the
// query's: equal tags never decide.  The hits are compacted on the device (a
// scan and a scatter) into ascending record indices with their query
// indices; pairs adds the mate of every hit (records 2k and 2k + 1).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstring>
#include <vector>

#include "../../include/fqz5_fastq.h"
#include "gpu_ctx.hpp"
#include "query_table.hpp"

namespace fqz5 {
GpuCtx &gpu();
void fqz5_set_error(const char *msg);
// fastq.hip: the positions of every `ch` byte of d_text[0..len), in order
uint64_t *fastq_find_delims(GpuCtx &g, const uint8_t *d_text, uint64_t len, uint8_t ch,
                            uint64_t *count);
}  // namespace fqz5

struct fqz5_name_table : fqz5::QueryTable {};

namespace fqz5 {
namespace {

constexpr uint32_t NM_WIN = 8192;               // bytes of the LDS staging window

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
                                                   QueryView T, uint32_t *hit) {
    __shared__ uint4 win4[NM_WIN / 16];
    const uint8_t *win = reinterpret_cast<const uint8_t *>(win4);
    const uint32_t lane = threadIdx.x;
    const uint32_t r0 = blockIdx.x * 64u, r = r0 + lane;
    const bool act = r < nrec;
    const uint32_t rend = min(r0 + 64u, nrec);
    const uint64_t B0 = r0 ? zpos[r0 - 1] + 1 : 0, B1 = zpos[rend - 1] + 1;
    const uint64_t s = act ? (r ? zpos[r - 1] + 1 : 0) : B1;      // the record's bytes [s, e)
    const uint64_t e = act ? zpos[r] : B1;
    uint64_t p = s;
    uint32_t h = NM_HASH0, klen = 0;
    bool done = !act;
    // windows start where the address is a multiple of 16 (the section may
    // start anywhere in its buffer), so the first may start before offset 0
    for (int64_t w0 = aligned_start(names, B0); w0 < int64_t(B1); w0 += NM_WIN) {
        for (uint32_t i = lane; i < NM_WIN / 16; i += 64u) {
            const int64_t a = w0 + 16 * int64_t(i);
            if (a >= int64_t(B1)) break;
            win4[i] = load16(names, name_len, a);
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
    if (klen)                                    // (no query is empty)
        nm_probe(T, nm_hash(h, 0, true), [&](uint32_t qi) {
            if (T.len(qi) != klen) return false;
            const uint64_t qa = T.qoff[qi];
            uint32_t i = 0;
            while (i < klen && names[s + i] == T.q[qa + i]) i++;
            if (i == klen) found = qi;
            return i == klen;
        });
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
        T->parse(q, q_len, nq, 0, "names_table_build", "query", "queries");
        T->fill("names_table_build", "query");
        return T;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        delete T;
        return nullptr;
    }
}

void fqz5_names_table_free(fqz5_name_table *T) { delete T; }

int64_t fqz5_names_table_find(const fqz5_name_table *T, const uint8_t *key, uint64_t len) {
    if (!T || !len) return -1;
    const QueryView V = T->host();
    int64_t found = -1;
    nm_probe(V, nm_hash_of(key, len), [&](uint32_t qi) {
        if (V.len(qi) == len && !std::memcmp(V.q + V.qoff[qi], key, size_t(len))) found = qi;
        return found >= 0;
    });
    return found;
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
        check_records(nrec, 0, "names_match");
        GpuCtx &g = gpu();
        gp = &g;
        const QueryView D = const_cast<fqz5_name_table *>(T)->device_copy("names_match");
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
