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

#include <cstring>

#include "rans_format.hpp"

namespace fqz5 {
namespace host {

bool rans_parse_o0(const uint8_t *p, const uint8_t *end, std::vector<uint32_t> &Fv, uint32_t *used) {
    uint32_t F[256] = {0}, tot = 0;
    const int k = get_freq0(p, end, F, &tot);
    if (!k) return false;
    scale_pow2(F, tot, 4096);
    uint32_t x = 0;
    for (int s = 0; s < 256; s++) x += F[s];
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

}  // namespace host
}  // namespace fqz5

extern "C" int fqz5_rans_dec_host(const unsigned char *in, size_t in_size, unsigned char *out,
                                  size_t out_cap, size_t *out_size) {
    return fqz5::host::rans_dec_stream(in, in_size, out, out_cap, out_size);
}
