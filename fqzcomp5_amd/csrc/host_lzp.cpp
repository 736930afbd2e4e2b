// host_lzp.cpp — unlzp (lzp16e.c:166-214) on a host core, token by token as
// k_lzp_dec (lzp.hip) decodes it:
//
//   * every output position P enters the table under the hash of the 4 bytes
//     before it (positions 0..3: of the bytes there are, from 0); position 0
//     is the table's "empty", so it never counts as a prediction;
//   * a byte other than 233 / 234 is a literal whatever the table holds;
//   * 233 / 234 with an empty table entry is a literal itself; otherwise it
//     carries a 1-byte / 2-byte length, 0 meaning that an escaped literal
//     follows;
//   * a match copies from the predicted position forward, so an overlapping
//     one repeats with period op - pred.
//
// The hash is rolled here: one update shifts the state by 4 bits, so after 4
// updates of a 16-bit state nothing older is left, which is the kernel's hash
// of the last 4 bytes.
#include <cstring>
#include <vector>

#include "host_lzp.hpp"

namespace fqz5 {
namespace host {

namespace {
constexpr uint32_t HASH_BITS = 16, MARK = 233;        // lzp16e.c:43-45, :54

inline uint32_t upd(uint32_t h, uint32_t c) {         // lzp16e.c:102
    return ((((h * 0x8ca6b53u) << 4) + (h << 5) * 17u) ^ c) & ((1u << HASH_BITS) - 1);
}
}  // namespace

bool unlzp(const uint8_t *in, size_t in_len, uint8_t *out, size_t cap, size_t *out_len) {
    *out_len = 0;
    if (in_len > 0xffffffffull) return false;         // positions are 32-bit, as the kernel's
    if (cap > 0xffffffffull) cap = 0xffffffffull;
    std::vector<uint32_t> ht(size_t(1) << HASH_BITS, 0);
    size_t ip = 0, op = 0;
    uint32_t h = 0;
    bool ok = true;
    while (ip < in_len) {
        const uint32_t b = in[ip];
        uint32_t ml = 0, lit = b;
        size_t adv = 1;
        const uint32_t p = b == MARK || b == MARK + 1 ? ht[h] : 0;
        if (p) {
            if (b == MARK) {
                if (ip + 1 >= in_len) { ok = false; break; }
                ml = in[ip + 1];
                adv = 2;
            } else {
                if (ip + 2 >= in_len) { ok = false; break; }
                ml = uint32_t(in[ip + 1]) << 8 | in[ip + 2];
                adv = 3;
            }
            if (!ml) {                                 // an escaped literal
                if (ip + adv >= in_len) { ok = false; break; }
                lit = in[ip + adv];
                adv++;
            }
        }
        if (!ml) {
            if (op >= cap) { ok = false; break; }
            out[op] = uint8_t(lit);
            ht[h] = uint32_t(op);
            h = upd(h, lit);
            op++;
            ip += adv;
            continue;
        }
        if (ml > cap - op) { ok = false; break; }
        // p < op: the table only holds positions already written
        const uint8_t *src = out + p;
        uint8_t *dst = out + op;
        if (op - p >= ml) std::memcpy(dst, src, ml);
        else for (uint32_t k = 0; k < ml; k++) dst[k] = src[k];
        for (uint32_t k = 0; k < ml; k++) {
            ht[h] = uint32_t(op + k);
            h = upd(h, dst[k]);
        }
        op += ml;
        ip += adv;
    }
    *out_len = op;
    return ok;
}

}  // namespace host
}  // namespace fqz5
