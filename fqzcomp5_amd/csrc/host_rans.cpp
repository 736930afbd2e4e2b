// host_rans.cpp — plain rANS 4x16 entropy chains on a host core.
//
// The arithmetic of k_rans_dec's NX = 4 bodies (rans_chain.hip dec4_body,
// dec4_lean_body), stated once more in scalar C++:
//   slot = x & (2^bits - 1) selects the symbol s whose [start, start + f)
//   holds it;  x' = f * (x >> bits) + slot - start (32-bit wrap-around, as
//   the kernel's 24-bit multiply gives for f <= 2^12);  a state below 2^15
//   takes the next 16-bit word: x = x' << 16 | word.  Within one step the
//   states renormalise in the order 0..3.
//   Order-0: step t, state z decodes byte 4t + z; the last step has n % 4
//   states.  Order-1: state z decodes the bytes [z * (n/4), ...) in the
//   context of its previous byte (0 at the start), the last state also the
//   n % 4 bytes of the tail.
//   Verdict: ok when the chain took no more words than (in_len - 16) / 2.
// The table is the kernel's LDS image: (f-1) << (bits+8) | (slot-start) << 8
// | symbol (order-1: its index in the context alphabet).  A context row
// without frequencies (reached by a damaged stream only) decodes as the
// kernel's zero-filled image does: symbol index 0 with f = 1 and
// slot - start = 0, or = slot in the split layout.
#include "host_rans.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "rans_format.hpp"

namespace fqz5 {
namespace host {

bool rans_parse_o0(const uint8_t *p, const uint8_t *end, std::vector<uint32_t> &Fv, uint32_t *used,
                   bool skip) {
    uint32_t F[256] = {0}, tot = 0;
    const int k = get_freq0(p, end, F, &tot);
    if (!k) return false;
    scale_pow2(F, tot, 4096);
    uint32_t x = 0;
    for (int s = 0; s < 256; s++) {
        // skip: a frequency larger than the slots left is passed over, as the
        // 32-state decoder's table builder does (rans_F_to_s3,
        // rANS_static16_int.h:540); the 4-state decoder refuses the table
        if (skip && F[s] > 4096 - std::min(x, 4096u)) F[s] = 0;
        x += F[s];
    }
    if (x != 4096) return false;
    Fv.assign(F, F + 256);
    *used = uint32_t(k);
    return true;
}

bool rans_parse_o1(const uint8_t *p0, const uint8_t *end, int bits, std::vector<uint32_t> &Fv,
                   std::vector<uint8_t> &alpha, uint32_t *used) {
    const uint8_t *p = p0;
    uint32_t A[256] = {0};
    int k = get_alphabet(p, end, A);
    if (!k) return false;
    p += k;
    if (p >= end) return false;
    alpha.clear();
    for (int s = 0; s < 256; s++)
        if (A[s]) alpha.push_back(uint8_t(s));
    if (alpha.empty() || alpha[0] != 0) return false;
    Fv.assign(alpha.size() * 256, 0);
    for (size_t r = 0; r < alpha.size(); r++) {
        uint32_t F[256] = {0}, T = 0;
        k = get_freq_row(p, end, A, F, &T);
        if (!k) return false;
        p += k;
        if (!T) continue;
        scale_pow2(F, T, 1u << bits);
        uint32_t x = 0;
        for (int s = 0; s < 256; s++) x += F[s];
        if (x != (1u << bits)) return false;
        std::memcpy(&Fv[r * 256], F, sizeof F);
    }
    *used = uint32_t(p - p0);
    return true;
}

namespace {

constexpr uint32_t LOW = 1u << 15;

inline uint32_t rd32(const uint8_t *p) {
    return p[0] | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

// the four states' renormalisation with at least four words left at p: one
// load of the window, each state's word picked from it by the count of the
// states before it that took one (no load waits for another state's verdict)
inline void renorm4(uint32_t &x0, uint32_t &x1, uint32_t &x2, uint32_t &x3, const uint8_t *&p) {
    uint64_t win;
    std::memcpy(&win, p, 8);                 // little-endian words
    const uint32_t c0 = x0 < LOW, c1 = x1 < LOW, c2 = x2 < LOW, c3 = x3 < LOW;
    x0 = c0 ? (x0 << 16) | uint32_t(win & 0xffffu) : x0;
    win >>= 16 * c0;
    x1 = c1 ? (x1 << 16) | uint32_t(win & 0xffffu) : x1;
    win >>= 16 * c1;
    x2 = c2 ? (x2 << 16) | uint32_t(win & 0xffffu) : x2;
    win >>= 16 * c2;
    x3 = c3 ? (x3 << 16) | uint32_t(win & 0xffffu) : x3;
    p += 2 * (c0 + c1 + c2 + c3);
}
inline bool renorm_checked(uint32_t &x, const uint8_t *&p, const uint8_t *end) {
    if (x >= LOW) return true;
    if (p + 2 > end) return false;
    x = (x << 16) | p[0] | uint32_t(p[1]) << 8;
    p += 2;
    return true;
}

// the table rows of F (rows x 256) for 2^bits slots; idx: the symbol's
// emitted value (order-1: its alphabet index), -1 where it has none
bool build_table(std::vector<uint32_t> &tab, const uint32_t *F, size_t rows, int bits,
                 const int *idx, bool split_table) {
    const uint32_t M = 1u << bits;
    tab.assign(rows << bits, 0);
    for (size_t r = 0; r < rows; r++) {
        const uint32_t *Fr = F + r * 256;
        uint32_t *t = tab.data() + (r << bits);
        uint32_t x = 0;
        for (int s = 0; s < 256; s++) {
            const uint32_t f = Fr[s];
            if (!f) continue;
            if (idx[s] < 0 || f > M - x) return false;
            for (uint32_t y = 0; y < f; y++) t[x + y] = (f - 1) << (bits + 8) | y << 8 | uint32_t(idx[s]);
            x += f;
        }
        if (x == 0 && split_table)
            for (uint32_t y = 0; y < M; y++) t[y] = y << 8;
        else if (x != 0 && x != M)
            return false;
    }
    return true;
}

// the GPU decoder's table layout rule (kernels.h dec_table_mode): the split
// layout for an order-1 table too large for the whole-entry image
bool split_layout(size_t rows, int bits) {
    constexpr size_t LDS_MAX = 147456;
    const size_t slots = rows << bits;
    size_t rpl = 0;
    while ((size_t(1) << rpl) < rows) rpl++;
    return slots * 4 > LDS_MAX && (slots / 4 + (rows << rpl)) * 4 <= LDS_MAX;
}

}  // namespace

bool rans_dec_o0(const uint32_t *F, int bits, const uint8_t *in, size_t in_len, uint8_t *out,
                 size_t n) {
    if (bits < 1 || bits > 12 || in_len < 16) return false;
    int idx[256];
    for (int s = 0; s < 256; s++) idx[s] = s;
    std::vector<uint32_t> tabv;
    if (!build_table(tabv, F, 1, bits, idx, false)) return false;
    const uint32_t *tab = tabv.data();
    const uint32_t mask = (1u << bits) - 1;
    const int sh = bits + 8;
    uint32_t x0 = rd32(in), x1 = rd32(in + 4), x2 = rd32(in + 8), x3 = rd32(in + 12);
    const uint8_t *p = in + 16, *end = p + ((in_len - 16) & ~size_t(1));
    const size_t steps = n / 4;
    size_t t = 0;
#define FQZ5_O0_SYM(x, o)                                                     \
    {                                                                         \
        const uint32_t e = tab[(x) & mask], xh = (x) >> bits;                 \
        (o) = uint8_t(e);                                                     \
        (x) = (e >> sh) * xh + xh + ((e >> 8) & mask);                        \
    }
    // while four words are left, no step can run out of them
    for (; t < steps && p + 8 <= end; t++) {
        uint8_t *o = out + 4 * t;
        FQZ5_O0_SYM(x0, o[0]);
        FQZ5_O0_SYM(x1, o[1]);
        FQZ5_O0_SYM(x2, o[2]);
        FQZ5_O0_SYM(x3, o[3]);
        renorm4(x0, x1, x2, x3, p);
    }
    for (; t < steps; t++) {
        uint8_t *o = out + 4 * t;
        FQZ5_O0_SYM(x0, o[0]);
        FQZ5_O0_SYM(x1, o[1]);
        FQZ5_O0_SYM(x2, o[2]);
        FQZ5_O0_SYM(x3, o[3]);
        if (!renorm_checked(x0, p, end) || !renorm_checked(x1, p, end) ||
            !renorm_checked(x2, p, end) || !renorm_checked(x3, p, end))
            return false;
    }
    // the last step: n % 4 states
    const size_t r = n % 4;
    uint8_t *o = out + 4 * steps;
    if (r > 0) {
        FQZ5_O0_SYM(x0, o[0]);
        if (!renorm_checked(x0, p, end)) return false;
    }
    if (r > 1) {
        FQZ5_O0_SYM(x1, o[1]);
        if (!renorm_checked(x1, p, end)) return false;
    }
    if (r > 2) {
        FQZ5_O0_SYM(x2, o[2]);
        if (!renorm_checked(x2, p, end)) return false;
    }
#undef FQZ5_O0_SYM
    return true;
}

bool rans_dec_o1(const uint32_t *F, const uint8_t *alpha, size_t rows, int bits, bool split_table,
                 const uint8_t *in, size_t in_len, uint8_t *out, size_t n) {
    if (bits < 1 || bits > 12 || rows < 1 || rows > 256 || in_len < 16) return false;
    int idx[256];
    for (int s = 0; s < 256; s++) idx[s] = -1;
    for (size_t r = 0; r < rows; r++) idx[alpha[r]] = int(r);
    std::vector<uint32_t> tabv;
    if (!build_table(tabv, F, rows, bits, idx, split_table)) return false;
    const uint32_t *tab = tabv.data();
    const uint32_t mask = (1u << bits) - 1;
    const int sh = bits + 8;
    uint32_t x0 = rd32(in), x1 = rd32(in + 4), x2 = rd32(in + 8), x3 = rd32(in + 12);
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;             // each state's context row (slots)
    const uint8_t *p = in + 16, *end = p + ((in_len - 16) & ~size_t(1));
    const size_t isz = n / 4;
    uint8_t *o0 = out, *o1 = out + isz, *o2 = out + 2 * isz, *o3 = out + 3 * isz;
    size_t t = 0;
#define FQZ5_O1_SYM(x, r, o)                                                  \
    {                                                                         \
        const uint32_t e = tab[(r) + ((x) & mask)], xh = (x) >> bits;         \
        (o) = alpha[e & 0xffu];                                               \
        (r) = (e & 0xffu) << bits;                                            \
        (x) = (e >> sh) * xh + xh + ((e >> 8) & mask);                        \
    }
    for (; t < isz && p + 8 <= end; t++) {
        FQZ5_O1_SYM(x0, r0, o0[t]);
        FQZ5_O1_SYM(x1, r1, o1[t]);
        FQZ5_O1_SYM(x2, r2, o2[t]);
        FQZ5_O1_SYM(x3, r3, o3[t]);
        renorm4(x0, x1, x2, x3, p);
    }
    for (; t < isz; t++) {
        FQZ5_O1_SYM(x0, r0, o0[t]);
        FQZ5_O1_SYM(x1, r1, o1[t]);
        FQZ5_O1_SYM(x2, r2, o2[t]);
        FQZ5_O1_SYM(x3, r3, o3[t]);
        if (!renorm_checked(x0, p, end) || !renorm_checked(x1, p, end) ||
            !renorm_checked(x2, p, end) || !renorm_checked(x3, p, end))
            return false;
    }
    // the tail on the last state
    for (const size_t last = n - 3 * isz; t < last; t++) {
        FQZ5_O1_SYM(x3, r3, o3[t]);
        if (!renorm_checked(x3, p, end)) return false;
    }
#undef FQZ5_O1_SYM
    return true;
}

int rans_dec_stream(const uint8_t *in, size_t in_size, uint8_t *out, size_t out_cap,
                    size_t *out_size) {
    if (!in || !out_size || in_size < 1 || in_size > 0xffffffffu || out_cap > 0xffffffffu) return -1;
    const int order = in[0];
    if (order & ~(1 | ORD_NOSZ)) return -1;
    const uint8_t *end = in + in_size;
    uint32_t p = 1, osz = uint32_t(out_cap);
    if (!(order & ORD_NOSZ)) p += varint_get(in + p, end, &osz);
    if (osz > out_cap) return -1;
    const uint8_t *h = in + p;
    const uint32_t len = uint32_t(in_size) - p;
    *out_size = 0;
    if (!len || !osz) return 0;                       // (the planner's empty leaf)
    std::vector<uint32_t> F;
    std::vector<uint8_t> alpha;
    uint32_t tab_len = 0;
    if (!(order & 1)) {
        if (!rans_parse_o0(h, h + len, F, &tab_len)) return -1;
        if (len < tab_len + 16u) return -1;
        if (!rans_dec_o0(F.data(), 12, h + tab_len, len - tab_len, out, osz)) return -1;
        *out_size = osz;
        return 0;
    }
    // order-1 header byte: shift << 4 | compressed
    const int bits = h[0] >> 4;
    if (bits != 10 && bits != 12) return -1;
    uint32_t used = 0;
    if (h[0] & 1) {
        uint32_t u, c, q = 1;
        q += varint_get(h + q, h + len, &u);
        q += varint_get(h + q, h + len, &c);
        if (c > len - q || u > (1u << 24)) return -1;
        tab_len = q + c;
        std::vector<uint8_t> hdr(u);
        if (u) {
            std::vector<uint32_t> F0;
            uint32_t t0 = 0;
            if (!rans_parse_o0(h + q, h + q + c, F0, &t0)) return -1;
            if (c < t0 + 16u) return -1;
            if (!rans_dec_o0(F0.data(), 12, h + q + t0, c - t0, hdr.data(), u)) return -1;
        }
        if (!rans_parse_o1(hdr.data(), hdr.data() + hdr.size(), bits, F, alpha, &used)) return -1;
    } else {
        if (!rans_parse_o1(h + 1, h + len, bits, F, alpha, &used)) return -1;
        tab_len = 1 + used;
    }
    if (len < tab_len + 16u) return -1;
    if (!rans_dec_o1(F.data(), alpha.data(), alpha.size(), bits, split_layout(alpha.size(), bits),
                     h + tab_len, len - tab_len, out, osz))
        return -1;
    *out_size = osz;
    return 0;
}

// ---- a stream that runs out of words, as the reference decodes it -----------
// (rANS_static4x16pr.c:335-340, :740-790; rANS_static32x16pr.c:360-400)

namespace {

// slot -> symbol, and each symbol's frequency and first slot; zeroed for a
// context without frequencies
struct RefRow {
    std::vector<uint8_t> sym;
    uint16_t f[256] = {0}, b[256] = {0};
};

void ref_row(const uint32_t *F, int bits, RefRow &t) {
    t.sym.assign(size_t(1) << bits, 0);
    uint32_t x = 0;
    for (int s = 0; s < 256; s++) {
        if (!F[s] || F[s] > (1u << bits) - x) continue;
        t.f[s] = uint16_t(F[s]);
        t.b[s] = uint16_t(x);
        std::memset(&t.sym[x], s, F[s]);
        x += F[s];
    }
}

inline uint32_t ref_renorm(uint32_t x, const uint8_t *&p, const uint8_t *end) {
    if (x < LOW && p + 1 < end) {
        x = (x << 16) | p[0] | uint32_t(p[1]) << 8;
        p += 2;
    }
    return x;
}

inline uint32_t ref_step(uint32_t &x, const RefRow &t, int bits, const uint8_t *&p,
                         const uint8_t *end) {
    const uint32_t m = x & ((1u << bits) - 1), s = t.sym[m];
    x = ref_renorm(t.f[s] * (x >> bits) + m - t.b[s], p, end);
    return s;
}

}  // namespace

bool rans_dec_ref(const uint8_t *in, uint32_t len, uint8_t *out, uint32_t n, bool o1, int nx) {
    if (nx != 4 && nx != 32) return false;
    if (len < (o1 && nx == 32 ? 128u : 16u)) return false;
    const uint8_t *end = in + len, *cp = in;
    std::vector<uint32_t> F;
    std::vector<uint8_t> alpha(1, 0);
    int bits = 12;
    uint32_t used = 0;
    if (!o1) {
        if (!rans_parse_o0(in, end, F, &used, nx == 32)) return false;
        cp = in + used;
    } else {
        bits = in[0] >> 4;
        if (bits != 10 && bits != 12) return false;
        if (in[0] & 1) {
            uint32_t u, c, q = 1;
            q += varint_get(in + q, end, &u);
            q += varint_get(in + q, end, &c);
            if (c > len - q || u > (1u << 24)) return false;
            std::vector<uint8_t> hdr(u);
            if (!rans_dec_ref(in + q, c, hdr.data(), u, false, 4)) return false;
            if (!rans_parse_o1(hdr.data(), hdr.data() + u, bits, F, alpha, &used)) return false;
            cp = in + q + c;
        } else {
            if (!rans_parse_o1(in + 1, end, bits, F, alpha, &used)) return false;
            cp = in + 1 + used;
        }
    }
    if (end - cp < 4 * nx) return false;
    uint32_t R[32];
    for (int z = 0; z < nx; z++, cp += 4) {
        R[z] = rd32(cp);
        if (R[z] < LOW) return false;
    }
    std::vector<RefRow> rows(alpha.size() + 1);      // the last: a context without a row
    int rowof[256];
    std::fill(rowof, rowof + 256, int(alpha.size()));
    for (size_t r = 0; r < alpha.size(); r++) {
        ref_row(&F[r * 256], bits, rows[r]);
        rowof[alpha[r]] = int(r);
    }
    rows.back().sym.assign(size_t(1) << bits, 0);
    if (!o1) {
        for (uint32_t i = 0; i < n; i++) out[i] = uint8_t(ref_step(R[i % nx], rows[0], bits, cp, end));
        return true;
    }
    const uint32_t isz = n / uint32_t(nx);
    uint8_t L[32] = {0};
    for (uint32_t k = 0; k < isz; k++)
        for (int z = 0; z < nx; z++)
            out[z * isz + k] = L[z] = uint8_t(ref_step(R[z], rows[rowof[L[z]]], bits, cp, end));
    for (uint32_t p = nx * isz; p < n; p++)
        out[p] = L[nx - 1] = uint8_t(ref_step(R[nx - 1], rows[rowof[L[nx - 1]]], bits, cp, end));
    return true;
}

// ---- the encoder's bare chains (rans_chain.hip chain_body_2w) ---------------
// Chunk j holds the steps [256 j, 256 j + 256), the chunks run from the top
// one (jtop = (T - 1) / 256) down, and checkpoint c = jtop - j holds the states
// before chunk j: so checkpoint 0 is RANS_LOW and a checkpoint follows every
// step k with k % 256 == 0, the last of them (k = 0) being the final states.
// The steps the kernel pads a chunk or a short state with are identity steps
// and are simply not made here.

namespace {

constexpr size_t ENC_CHUNK = 256;                // enc_chunk_steps(4)
constexpr size_t O1_PAIR_MIN = 1u << 16;         // order-1 chains that build the 64 K pair table

inline size_t enc_steps4(size_t n, bool o1) { return o1 ? n - 3 * (n / 4) : (n + 3) / 4; }

// The encoder symbol as the host step reads it: the two fields of cmpl_sh
// apart, the reciprocal's two shifts (32 and rcp_shift - 32) as one.
struct HSym { uint32_t rcp, xmax, bias; uint16_t cmpl, sh; };
inline HSym hsym(const EncSym &e) {
    return {e.rcp, e.xmax, e.bias, uint16_t(e.cmpl_sh), uint16_t(32u + (e.cmpl_sh >> 16))};
}

// RansEncPutSymbol without its word.
// The renormalisation must not become a branch (it is taken about every other
// step: a mispredicting branch cost 2.4x).  clang keeps the select of the two
// candidates a conditional move when told it is unpredictable (0.64 / 0.83 ns
// per symbol for order 0 / 1 on the MI355X box's cores, against 0.81 / 1.19
// for the shift below); gcc makes that select a branch, so it gets the shift
// count from the comparison instead.
inline uint32_t enc_step(uint32_t x, const HSym &e) {
#if defined(__clang__)
    const uint32_t xs = x >> 16;
    const uint32_t xr = __builtin_unpredictable(x > e.xmax) ? xs : x;
#else
    const uint32_t xr = x >> (uint32_t(x > e.xmax) << 4);
#endif
    const uint32_t q = uint32_t((uint64_t(xr) * e.rcp) >> e.sh);
    return q * e.cmpl + (xr + e.bias);
}

inline void enc_put(uint32_t *ck, size_t c, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    ck[4 * c] = x0;
    ck[4 * c + 1] = x1;
    ck[4 * c + 2] = x2;
    ck[4 * c + 3] = x3;
}

}  // namespace

size_t rans_enc_ck_words(size_t n, bool o1) {
    const size_t T = enc_steps4(n, o1);
    return ((T + ENC_CHUNK - 1) / ENC_CHUNK + 1) * 4;
}

void rans_enc_chain_o0(const EncSym *syms_in, const uint8_t *in, size_t n, uint32_t *ck) {
    if (!n) return;
    const size_t T = enc_steps4(n, false), jtop = (T - 1) / ENC_CHUNK;
    HSym syms[256];
    for (int s = 0; s < 256; s++) syms[s] = hsym(syms_in[s]);
    uint32_t x0 = LOW, x1 = LOW, x2 = LOW, x3 = LOW;
    enc_put(ck, 0, x0, x1, x2, x3);
    size_t k = T;                                // steps left: [0, k)
    if (n & 3) {                                 // the top step has n % 4 states
        k--;
        const uint8_t *p = in + 4 * k;
        x0 = enc_step(x0, syms[p[0]]);
        if ((n & 3) > 1) x1 = enc_step(x1, syms[p[1]]);
        if ((n & 3) > 2) x2 = enc_step(x2, syms[p[2]]);
        if (k % ENC_CHUNK == 0) enc_put(ck, jtop - k / ENC_CHUNK + 1, x0, x1, x2, x3);
    }
    while (k) {
        const size_t lo = (k - 1) & ~(ENC_CHUNK - 1);
        for (size_t t = k; t-- > lo;) {
            const uint8_t *p = in + 4 * t;
            x0 = enc_step(x0, syms[p[0]]);
            x1 = enc_step(x1, syms[p[1]]);
            x2 = enc_step(x2, syms[p[2]]);
            x3 = enc_step(x3, syms[p[3]]);
        }
        enc_put(ck, jtop - lo / ENC_CHUNK + 1, x0, x1, x2, x3);
        k = lo;
    }
}

// `at(c, s)`: the symbol of byte s in the context of byte c
template <class At>
static void enc_chain_o1(const At &at, const uint8_t *in, size_t n, uint32_t *ck) {
    const size_t isz = n / 4, T = enc_steps4(n, true), jtop = (T - 1) / ENC_CHUNK;
    const uint8_t *p0 = in, *p1 = in + isz, *p2 = in + 2 * isz, *p3 = in + 3 * isz;
    uint32_t x0 = LOW, x1 = LOW, x2 = LOW, x3 = LOW;
    enc_put(ck, 0, x0, x1, x2, x3);
    size_t k = T;
    while (k) {
        const size_t lo = (k - 1) & ~(ENC_CHUNK - 1);
        size_t t = k;
        // the tail: state 3 alone (its context is 0 at step 0: p3[-1] belongs to state 2)
        for (; t > lo && t > isz; t--) x3 = enc_step(x3, at(t > 1 ? p3[t - 2] : 0, p3[t - 1]));
        for (; t > lo && t > 1; t--) {                    // steps isz > t - 1 >= 1
            const size_t s = t - 1;
            x0 = enc_step(x0, at(p0[s - 1], p0[s]));
            x1 = enc_step(x1, at(p1[s - 1], p1[s]));
            x2 = enc_step(x2, at(p2[s - 1], p2[s]));
            x3 = enc_step(x3, at(p3[s - 1], p3[s]));
        }
        if (t > lo) {                                     // step 0 of the quarters: context 0
            x0 = enc_step(x0, at(0, p0[0]));
            x1 = enc_step(x1, at(0, p1[0]));
            x2 = enc_step(x2, at(0, p2[0]));
            x3 = enc_step(x3, at(0, p3[0]));
        }
        enc_put(ck, jtop - lo / ENC_CHUNK + 1, x0, x1, x2, x3);
        k = lo;
    }
}

void rans_enc_chain_o1(const EncSym *tab, const uint8_t *remap, int A, const uint8_t *in, size_t n,
                       uint32_t *ck) {
    if (!n) return;
    uint32_t row[256], col[256];                 // a byte as a context / as a symbol
    for (int s = 0; s < 256; s++) {
        col[s] = remap[s];
        row[s] = uint32_t(remap[s]) * uint32_t(A);
    }
    if (n < O1_PAIR_MIN) {
        std::vector<HSym> hs(size_t(A) * A);
        for (size_t i = 0; i < hs.size(); i++) hs[i] = hsym(tab[i]);
        const HSym *h = hs.data();
        enc_chain_o1([&](uint32_t c, uint32_t s) -> const HSym & { return h[row[c] + col[s]]; }, in, n, ck);
        return;
    }
    // a long chain: one table over the pair of bytes as they lie in the input
    // (context | symbol << 8), so a step looks its symbol up with one load
    std::vector<HSym> pair(65536);
    for (uint32_t s = 0; s < 256; s++)
        for (uint32_t c = 0; c < 256; c++) pair[c | s << 8] = hsym(tab[row[c] + col[s]]);
    const HSym *h = pair.data();
    enc_chain_o1([&](uint32_t c, uint32_t s) -> const HSym & { return h[c | s << 8]; }, in, n, ck);
}

void rans_enc_tab_o1(const uint16_t *f1, int A, int bits, EncSym *tab) {
    for (int r = 0; r < A; r++) {
        uint32_t start = 0;
        for (int c = 0; c < A; c++) {
            const uint32_t f = f1[size_t(r) * A + c];
            tab[size_t(r) * A + c] = f ? make_encsym(start, f, bits) : EncSym{0, 0, 0, 0};
            start += f;
        }
    }
}

}  // namespace host
}  // namespace fqz5

// freq: order-0 the 256 frequencies (sum 4096); order-1 256 x 256, row =
// context byte, every row that occurs summing to 2^bits
extern "C" uint32_t *fqz5_rans_enc_chain_host(const unsigned char *in, size_t n, int order, int bits,
                                              const uint32_t *freq, size_t *ck_words) {
    using namespace fqz5;
    if (!in || !n || !freq || !ck_words || n > 0xffffffffu || (order != 0 && order != 1)) return nullptr;
    if (order == 0 ? bits != 12 : (bits != 10 && bits != 12)) return nullptr;
    const uint32_t M = 1u << bits;
    std::vector<EncSym> tab;
    uint8_t remap[256] = {0};
    int A = 0;
    if (order == 0) {
        tab.assign(256, EncSym{0, 0, 0, 0});
        uint32_t x = 0;
        for (int s = 0; s < 256; s++) {
            if (freq[s] > M - x) return nullptr;
            if (freq[s]) tab[s] = make_encsym(x, freq[s], bits);
            x += freq[s];
        }
        if (x != M) return nullptr;
        for (size_t i = 0; i < n; i++)
            if (!freq[in[i]]) return nullptr;
    } else {
        // the alphabet as the compressor makes it: 0 and every byte of the input
        bool present[256] = {true};
        for (size_t i = 0; i < n; i++) present[in[i]] = true;
        for (int s = 0; s < 256; s++)
            if (present[s]) remap[s] = uint8_t(A++);
        std::vector<uint16_t> f1(size_t(A) * A, 0);
        for (int r = 0; r < 256; r++) {
            uint32_t x = 0;
            for (int s = 0; s < 256; s++) {
                const uint32_t f = freq[r * 256 + s];
                if (!f) continue;
                if (!present[r] || !present[s] || f > M - x) return nullptr;
                f1[size_t(remap[r]) * A + remap[s]] = uint16_t(f);
                x += f;
            }
            if (x && x != M) return nullptr;
        }
        // every (context, symbol) pair of the input needs a frequency
        const size_t isz = n / 4;
        for (size_t i = 0; i < n; i++) {
            const bool first = i == 0 || (isz && i % isz == 0 && i / isz < 4);
            const int c = first ? 0 : in[i - 1];
            if (!f1[size_t(remap[c]) * A + remap[in[i]]]) return nullptr;
        }
        tab.resize(size_t(A) * A);
        host::rans_enc_tab_o1(f1.data(), A, bits, tab.data());
    }
    const size_t words = host::rans_enc_ck_words(n, order == 1);
    uint32_t *ck = static_cast<uint32_t *>(std::malloc(words * sizeof(uint32_t)));
    if (!ck) return nullptr;
    if (order == 0) host::rans_enc_chain_o0(tab.data(), in, n, ck);
    else host::rans_enc_chain_o1(tab.data(), remap, A, in, n, ck);
    *ck_words = words;
    return ck;
}

extern "C" int fqz5_rans_dec_host(const unsigned char *in, size_t in_size, unsigned char *out,
                                  size_t out_cap, size_t *out_size) {
    return fqz5::host::rans_dec_stream(in, in_size, out, out_cap, out_size);
}
