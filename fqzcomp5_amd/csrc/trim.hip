// trim.hip — trim and clip (fqz5file.trim_records / trim_file): per record of
// a block's decoded bases and qualities the interval that is kept after the
// clip, quality, adapter, trim_n and crop steps (the rule:
// include/fqz5_fastq.h), and the streams compacted to those intervals.
//
// Two kernels per block:
//   k_trim_cuts    one wave per record (k_fq_format's shape), the steps in
//                  order, every one of them a loop over 64 positions at a time
//                  that ends with the record.  A quality end: the 64 terms
//                  cutoff - q[i] from the end in question, a wave-wide
//                  inclusive scan plus the carry of the chunks before, a
//                  ballot of sum < 0 for the break, the strict arg-max over
//                  the lanes before the break (the first lane in scan order
//                  that holds the maximum), and out at the first chunk that
//                  breaks.  The scan within a chunk is i32 (64 terms of at
//                  most 255 in size: below 2^15); the carry, the sums that
//                  are compared and `best` are i64.  The adapter: lane l of
//                  chunk i takes p = a + l + 64 i and counts its mismatches
//                  against each adapter in turn (the table in LDS), leaving an
//                  adapter at the first mismatch past the allowance; the wave
//                  ballots and stops at the first chunk with a match, which
//                  holds the smallest p, its lowest lane.  trim_n: a ballot
//                  of the bytes that are not N from either end.  Lane 0 adds
//                  the record's accounting to the workgroup's LDS counters
//                  (u64, so no launch split), flushed once per workgroup.
//   k_trim_gather  one wave per record: the bytes [start, start + new_len) of
//                  the record to the exclusive scan of the new lengths, 64
//                  consecutive bytes per step, so reads and writes coalesce.
// A stream is read byte by byte at positions inside the record the wave
// stands on, which lie in [0, seq_len) since the records' ends are checked to
// sum to it: nothing outside a stream is read.  A stream no step needs is
// never dereferenced.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fqz5_fastq.h"
#include "gpu_ctx.hpp"
#include "record_tile.hpp"

namespace fqz5 {
GpuCtx &gpu();
void fqz5_set_error(const char *msg);

namespace {

constexpr uint32_t TR_WAVE = 64;
constexpr uint32_t TR_WAVES = ST_THREADS / TR_WAVE;
constexpr uint32_t TR_SLOTS = 2 * FQZ5_TRIM_ADAPTERS;
constexpr uint32_t TR_NONE = 0xFFFFFFFFu;

__host__ __device__ inline bool is_n(uint32_t c) { return (c | 0x20u) == 'n'; }
__host__ __device__ inline bool needs_seq(const fqz5_trim_spec &t) {
    return (t.set & (FQZ5_TRIM_ADAPTER | FQZ5_TRIM_N)) != 0;
}
__host__ __device__ inline bool needs_qual(const fqz5_trim_spec &t) {
    return (t.set & (FQZ5_TRIM_Q5 | FQZ5_TRIM_Q3)) != 0;
}

// the parts of the rule both sides share
__host__ __device__ inline void clip_step(const fqz5_trim_spec &t, uint32_t L, uint32_t &a,
                                          uint32_t &b) {
    a = uint32_t(t.head < L ? t.head : L);
    const uint32_t e = L - uint32_t(t.tail < L ? t.tail : L);
    b = e > a ? e : a;
}
__host__ __device__ inline uint32_t crop_step(const fqz5_trim_spec &t, uint32_t a, uint32_t b) {
    return uint64_t(b - a) > t.max_len ? a + uint32_t(t.max_len) : b;
}
// the adapter slots of a mate: [first, first + count)
__host__ __device__ inline void mate_slots(const fqz5_trim_spec &t, uint32_t mate, uint32_t &first,
                                           uint32_t &count) {
    const bool own = mate && t.n_adapters[1];
    first = own ? t.n_adapters[0] : 0;
    count = own ? t.n_adapters[1] : t.n_adapters[0];
}
__host__ __device__ inline uint32_t allowance(const fqz5_trim_spec &t, uint32_t ov) {
    return (t.max_err_pct * ov) / 100;         // (100 * 128: no overflow)
}
// the lowest slot of [first, first + count) whose adapter matches at p of
// s[0..b), TR_NONE when none does
__host__ __device__ inline uint32_t adapter_at(const fqz5_trim_spec &t, const uint32_t *alen,
                                               const uint8_t *abytes, uint32_t first,
                                               uint32_t count, const uint8_t *s, uint32_t p,
                                               uint32_t b) {
    for (uint32_t j = first; j < first + count; j++) {
        const uint32_t m = alen[j], ov = m < b - p ? m : b - p;
        if (ov < t.min_overlap) continue;
        const uint32_t allowed = allowance(t, ov);
        const uint8_t *A = abytes + size_t(j) * FQZ5_TRIM_ADAPTER_MAX;
        uint32_t miss = 0, k = 0;
        for (; k < ov; k++)
            if (s[p + k] != A[k] && ++miss > allowed) break;
        if (k == ov) return j;
    }
    return TR_NONE;
}

// One quality end of q[a0..b0), the whole wave: from5 the 5' end (returns
// start), else the 3' end (returns stop).
__device__ __forceinline__ uint32_t quality_end(const uint8_t *q, uint32_t a0, uint32_t b0,
                                                int cutoff, bool from5, uint32_t lane) {
    const uint32_t n = b0 - a0;
    uint32_t cut = from5 ? a0 : b0;
    long long carry = 0, best = 0;
    for (uint64_t done = 0; done < n; done += TR_WAVE) {
        const uint32_t left = uint32_t(n - done), j = uint32_t(done) + lane;
        const bool in = lane < left;
        int s = in ? cutoff - int(q[from5 ? a0 + j : b0 - 1 - j]) : 0;
#pragma unroll
        for (uint32_t d = 1; d < TR_WAVE; d <<= 1) {
            const int up = __shfl_up(s, d);
            if (lane >= d) s += up;
        }
        const unsigned long long brk = __ballot(in && carry + s < 0);
        const uint32_t valid = brk ? uint32_t(__ffsll(brk)) - 1 : (left < TR_WAVE ? left : TR_WAVE);
        // the strict arg-max of the lanes before the break, the first of equals
        int m = lane < valid ? s : INT32_MIN;
#pragma unroll
        for (uint32_t d = TR_WAVE / 2; d; d >>= 1) {
            const int o = __shfl_xor(m, d);
            m = o > m ? o : m;
        }
        if (valid && carry + m > best) {
            best = carry + m;
            const unsigned long long eq = __ballot(lane < valid && s == m);
            const uint32_t at = uint32_t(done) + uint32_t(__ffsll(eq)) - 1;
            cut = from5 ? a0 + at + 1 : b0 - 1 - at;
        }
        if (brk) break;
        carry += __shfl(s, TR_WAVE - 1);
    }
    return cut;
}

// counts: FQZ5_TRIM_COUNTS words (include/fqz5_fastq.h)
__global__ __launch_bounds__(ST_THREADS) void k_trim_cuts(
    fqz5_trim_spec t, const fqz5_trim_adapters *adapters, const uint8_t *seq, const uint8_t *qual,
    const uint64_t *end, uint32_t nrec, int pairs, uint32_t *start, uint32_t *new_len,
    unsigned long long *counts) {
    __shared__ unsigned long long cnt[FQZ5_TRIM_COUNTS];
    __shared__ uint32_t alen[TR_SLOTS];
    __shared__ uint8_t abytes[TR_SLOTS * FQZ5_TRIM_ADAPTER_MAX];
    if (threadIdx.x < FQZ5_TRIM_COUNTS) cnt[threadIdx.x] = 0;
    if (t.set & FQZ5_TRIM_ADAPTER) {
        const uint32_t slots = t.n_adapters[0] + t.n_adapters[1];
        if (threadIdx.x < slots) alen[threadIdx.x] = adapters->len[threadIdx.x];
        for (uint32_t i = threadIdx.x; i < slots * FQZ5_TRIM_ADAPTER_MAX; i += ST_THREADS)
            abytes[i] = adapters->bytes[i / FQZ5_TRIM_ADAPTER_MAX][i % FQZ5_TRIM_ADAPTER_MAX];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x % TR_WAVE, wave = threadIdx.x / TR_WAVE;
    for (uint64_t r = uint64_t(blockIdx.x) * TR_WAVES + wave; r < nrec;
         r += uint64_t(gridDim.x) * TR_WAVES) {
        const uint64_t at = r ? end[r - 1] : 0;
        const uint32_t L = uint32_t(end[r] - at);
        const uint8_t *s = seq ? seq + at : nullptr, *q = qual ? qual + at : nullptr;
        uint32_t a = 0, b = L, took[FQZ5_TRIM_STEPS], hit = TR_NONE;
        if (t.set & FQZ5_TRIM_CLIP) clip_step(t, L, a, b);
        took[0] = L - (b - a);
        uint32_t len = b - a;
        if (t.set & (FQZ5_TRIM_Q5 | FQZ5_TRIM_Q3)) {
            const uint32_t a0 = a, b0 = b;
            if (t.set & FQZ5_TRIM_Q5) a = quality_end(q, a0, b0, int(t.q5), true, lane);
            if (t.set & FQZ5_TRIM_Q3) b = quality_end(q, a0, b0, int(t.q3), false, lane);
            b = b > a ? b : a;
        }
        took[1] = len - (b - a);
        len = b - a;
        if ((t.set & FQZ5_TRIM_ADAPTER) && len >= t.min_overlap) {
            uint32_t first, count;
            mate_slots(t, pairs ? uint32_t(r & 1) : 0, first, count);
            const uint64_t last = uint64_t(b) - t.min_overlap;       // the largest p
            for (uint64_t base = a; base <= last; base += TR_WAVE) {
                const uint64_t p = base + lane;
                const uint32_t j = p <= last ? adapter_at(t, alen, abytes, first, count, s,
                                                          uint32_t(p), b) : TR_NONE;
                const unsigned long long any = __ballot(j != TR_NONE);
                if (!any) continue;
                const uint32_t l = uint32_t(__ffsll(any)) - 1;
                hit = __shfl(j, l);
                b = uint32_t(base) + l;
                break;
            }
        }
        took[2] = len - (b - a);
        len = b - a;
        if (t.set & FQZ5_TRIM_N) {
            for (uint64_t base = a; base < b; base += TR_WAVE) {
                const uint64_t p = base + lane;
                const unsigned long long stay = __ballot(p < b && !is_n(s[p]));
                a = stay ? uint32_t(base) + uint32_t(__ffsll(stay)) - 1
                         : uint32_t(base + TR_WAVE < b ? base + TR_WAVE : b);
                if (stay) break;
            }
            while (b > a) {                                          // (b falls every turn)
                const uint32_t left = b - a < TR_WAVE ? b - a : TR_WAVE;
                const unsigned long long stay = __ballot(lane < left && !is_n(s[b - 1 - lane]));
                b -= stay ? uint32_t(__ffsll(stay)) - 1 : left;
                if (stay) break;
            }
        }
        took[3] = len - (b - a);
        len = b - a;
        if (t.set & FQZ5_TRIM_CROP) b = crop_step(t, a, b);
        took[4] = len - (b - a);
        if (lane == 0) {
            start[r] = a;
            new_len[r] = b - a;
            atomicAdd(&cnt[0], static_cast<unsigned long long>(L));
            atomicAdd(&cnt[1], static_cast<unsigned long long>(b - a));
#pragma unroll
            for (uint32_t k = 0; k < FQZ5_TRIM_STEPS; k++) {
                if (!took[k]) continue;
                atomicAdd(&cnt[2 + k], 1ull);
                atomicAdd(&cnt[7 + k], static_cast<unsigned long long>(took[k]));
            }
            if (hit != TR_NONE) atomicAdd(&cnt[12 + hit], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x < FQZ5_TRIM_COUNTS && cnt[threadIdx.x])
        atomicAdd(counts + threadIdx.x, cnt[threadIdx.x]);
}

// to[r]: where record r's kept bytes go (nrec + 1 entries, the exclusive scan
// of the new lengths)
__global__ __launch_bounds__(ST_THREADS) void k_trim_gather(const uint8_t *src, const uint64_t *end,
                                                            const uint32_t *start,
                                                            const uint64_t *to, uint32_t nrec,
                                                            uint8_t *dst) {
    const uint32_t lane = threadIdx.x % TR_WAVE, wave = threadIdx.x / TR_WAVE;
    for (uint64_t r = uint64_t(blockIdx.x) * TR_WAVES + wave; r < nrec;
         r += uint64_t(gridDim.x) * TR_WAVES) {
        const uint64_t at = r ? end[r - 1] : 0, L = end[r] - at;
        const uint64_t st = start[r] < L ? start[r] : L;             // (never outside the record)
        uint64_t n = to[r + 1] - to[r];
        n = n < L - st ? n : L - st;
        const uint8_t *from = src + at + st;
        uint8_t *out = dst + to[r];
        for (uint64_t i = lane; i < n; i += TR_WAVE) out[i] = from[i];
    }
}

// the checks fqz5_trim_cuts and fqz5_trim_host make before anything is written
std::vector<uint64_t> check_call(const fqz5_trim_spec *t, const fqz5_trim_adapters *ad,
                                 bool has_seq, bool has_qual, uint64_t seq_len,
                                 const uint32_t *lens, uint64_t nrec, int pairs, const char *who) {
    const std::string w(who);
    if (!t) throw GpuError(w + ": no steps");
    if (t->set >> 6) throw GpuError(w + ": an unknown step");
    if (((t->set & FQZ5_TRIM_Q5) && t->q5 > 93) || ((t->set & FQZ5_TRIM_Q3) && t->q3 > 93))
        throw GpuError(w + ": a quality cutoff over 93");
    if (t->set & FQZ5_TRIM_ADAPTER) {
        if (!ad) throw GpuError(w + ": the adapter step without adapters");
        if (!t->n_adapters[0] || t->n_adapters[0] > FQZ5_TRIM_ADAPTERS ||
            t->n_adapters[1] > FQZ5_TRIM_ADAPTERS)
            throw GpuError(w + ": 1 to 16 adapters per mate");
        if (t->min_overlap < 1 || t->max_err_pct > 100)
            throw GpuError(w + ": min_overlap below 1 or max_err_pct over 100");
        for (uint32_t j = 0; j < t->n_adapters[0] + t->n_adapters[1]; j++)
            if (!ad->len[j] || ad->len[j] > FQZ5_TRIM_ADAPTER_MAX)
                throw GpuError(w + ": an adapter of 0 or more than 128 bytes");
    }
    if (needs_seq(*t) && !has_seq) throw GpuError(w + ": a base step without the bases");
    if (needs_qual(*t) && !has_qual) throw GpuError(w + ": a quality step without the qualities");
    check_records(nrec, pairs, who);
    return record_ends(lens, nrec, seq_len, who);
}

uint32_t wave_grid(const GpuCtx &g, uint64_t nrec) {
    return uint32_t(std::min<uint64_t>((nrec + TR_WAVES - 1) / TR_WAVES, 8ull * g.cus));
}

}  // namespace
}  // namespace fqz5

using namespace fqz5;

extern "C" {

int fqz5_trim_cuts(const fqz5_trim_spec *t, const fqz5_trim_adapters *adapters,
                   const uint8_t *d_seq, const uint8_t *d_qual, uint64_t seq_len,
                   const uint32_t *h_len, uint64_t nrec, int pairs, uint32_t *d_start,
                   uint32_t *h_new_len, uint64_t *h_counts) {
    GpuCtx *gp = nullptr;
    unsigned long long counts[FQZ5_TRIM_COUNTS] = {};      // (outlives the try: a copy lands here)
    try {
        const std::vector<uint64_t> end = check_call(t, adapters, d_seq != nullptr,
                                                     d_qual != nullptr, seq_len, h_len, nrec, pairs,
                                                     "trim_cuts");
        if (!nrec) return 0;
        GpuCtx &g = gpu();
        gp = &g;
        const uint32_t n = uint32_t(nrec);
        const uint64_t *d_end = g.upload(end);
        const fqz5_trim_adapters *d_ad =
            (t->set & FQZ5_TRIM_ADAPTER) ? g.upload(adapters, 1) : nullptr;
        uint32_t *d_new = g.arena.alloc_n<uint32_t>(n);
        unsigned long long *d_counts = g.arena.alloc_n<unsigned long long>(FQZ5_TRIM_COUNTS);
        g.memset0(d_counts, FQZ5_TRIM_COUNTS * 8);
        hipLaunchKernelGGL(k_trim_cuts, dim3(wave_grid(g, nrec)), dim3(ST_THREADS), 0, g.stream, *t,
                           d_ad, needs_seq(*t) ? d_seq : nullptr, needs_qual(*t) ? d_qual : nullptr,
                           d_end, n, pairs, d_start, d_new, d_counts);
        FQZ5_HIP(hipGetLastError());
        g.download(h_new_len, d_new, n);
        g.download(counts, d_counts, FQZ5_TRIM_COUNTS);
        g.sync();
        for (int k = 0; k < FQZ5_TRIM_COUNTS; k++) h_counts[k] += counts[k];
        g.reset();
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { if (gp) gp->reset(); } catch (...) {}
        return -1;
    }
}

int fqz5_trim_gather(const uint8_t *d_src, uint64_t seq_len, const uint32_t *h_len,
                     const uint32_t *d_start, const uint32_t *h_new_len, uint64_t nrec,
                     uint8_t *d_dst, uint64_t dst_cap, uint64_t *out_len) {
    GpuCtx *gp = nullptr;
    try {
        *out_len = 0;
        check_records(nrec, 0, "trim_gather");
        const std::vector<uint64_t> end = record_ends(h_len, nrec, seq_len, "trim_gather");
        std::vector<uint64_t> to(size_t(nrec) + 1, 0);
        for (uint64_t r = 0; r < nrec; r++) {
            if (h_new_len[r] > h_len[r]) throw GpuError("trim_gather: an interval outside its record");
            to[size_t(r) + 1] = to[size_t(r)] + h_new_len[r];
        }
        const uint64_t total = to[size_t(nrec)];
        if (total > dst_cap) throw GpuError("trim_gather: the destination is too small");
        if ((!d_src && seq_len) || (!d_dst && total) || (!d_start && nrec))
            throw GpuError("trim_gather: a buffer is missing");
        // distinct buffers: [d_src, d_src + seq_len) and [d_dst, d_dst + dst_cap) apart
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
        if (d_src == d_dst || (s0 < d0 + dst_cap && d0 < s0 + seq_len))
            throw GpuError("trim_gather: source and destination overlap");
        *out_len = total;
        if (!total) return 0;
        GpuCtx &g = gpu();
        gp = &g;
        const uint64_t *d_end = g.upload(end), *d_to = g.upload(to);
        hipLaunchKernelGGL(k_trim_gather, dim3(wave_grid(g, nrec)), dim3(ST_THREADS), 0, g.stream,
                           d_src, d_end, d_start, d_to, uint32_t(nrec), d_dst);
        FQZ5_HIP(hipGetLastError());
        g.reset();
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { if (gp) gp->reset(); } catch (...) {}
        return -1;
    }
}

int fqz5_trim_host(const fqz5_trim_spec *t, const fqz5_trim_adapters *adapters,
                   const uint8_t *seq, const uint8_t *qual, uint64_t seq_len,
                   const uint32_t *lens, uint64_t nrec, int pairs, uint32_t *start,
                   uint32_t *new_len, uint64_t *counts, uint8_t *out_seq, uint8_t *out_qual) {
    try {
        check_call(t, adapters, seq != nullptr, qual != nullptr, seq_len, lens, nrec, pairs,
                   "trim_host");
        if ((out_seq && !seq) || (out_qual && !qual))
            throw GpuError("trim_host: a stream to compact is missing");
        uint64_t at = 0, to = 0;
        for (uint64_t r = 0; r < nrec; r++) {
            const uint32_t L = lens[r];
            const uint8_t *s = seq ? seq + at : nullptr, *q = qual ? qual + at : nullptr;
            uint32_t a = 0, b = L, len = L, took[FQZ5_TRIM_STEPS], hit = TR_NONE;
            if (t->set & FQZ5_TRIM_CLIP) clip_step(*t, L, a, b);
            took[0] = len - (b - a);
            len = b - a;
            if (needs_qual(*t)) {
                const uint32_t a0 = a, b0 = b;
                if (t->set & FQZ5_TRIM_Q5) {
                    int64_t sum = 0, best = 0;
                    for (uint32_t i = a0; i < b0; i++) {
                        sum += int64_t(t->q5) - q[i];
                        if (sum < 0) break;
                        if (sum > best) best = sum, a = i + 1;
                    }
                }
                if (t->set & FQZ5_TRIM_Q3) {
                    int64_t sum = 0, best = 0;
                    for (uint32_t i = b0; i-- > a0; ) {
                        sum += int64_t(t->q3) - q[i];
                        if (sum < 0) break;
                        if (sum > best) best = sum, b = i;
                    }
                }
                b = std::max(a, b);
            }
            took[1] = len - (b - a);
            len = b - a;
            if ((t->set & FQZ5_TRIM_ADAPTER) && len >= t->min_overlap) {
                uint32_t first, count;
                mate_slots(*t, pairs ? uint32_t(r & 1) : 0, first, count);
                for (uint64_t p = a; p + t->min_overlap <= b; p++) {
                    hit = adapter_at(*t, adapters->len, &adapters->bytes[0][0], first, count, s,
                                     uint32_t(p), b);
                    if (hit == TR_NONE) continue;
                    b = uint32_t(p);
                    break;
                }
            }
            took[2] = len - (b - a);
            len = b - a;
            if (t->set & FQZ5_TRIM_N) {
                while (a < b && is_n(s[a])) a++;
                while (b > a && is_n(s[b - 1])) b--;
            }
            took[3] = len - (b - a);
            len = b - a;
            if (t->set & FQZ5_TRIM_CROP) b = crop_step(*t, a, b);
            took[4] = len - (b - a);
            start[r] = a;
            new_len[r] = b - a;
            counts[0] += L;
            counts[1] += b - a;
            for (uint32_t k = 0; k < FQZ5_TRIM_STEPS; k++) {
                counts[2 + k] += took[k] != 0;
                counts[7 + k] += took[k];
            }
            if (hit != TR_NONE) counts[12 + hit]++;
            if (out_seq) std::memcpy(out_seq + to, s + a, b - a);
            if (out_qual) std::memcpy(out_qual + to, q + a, b - a);
            at += L;
            to += b - a;
        }
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

}  // extern "C"
