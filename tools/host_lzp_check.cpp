// host_lzp_check.cpp — a stand-alone checker of the host unlzp
// (fqzcomp5_amd/csrc/host_lzp.cpp), meant for sanitizer builds: no HIP, no
// Python, its own main.
//
//   c++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/host_lzp_check.cpp fqzcomp5_amd/csrc/host_lzp.cpp -o check
//   check CASES [--time]
//
// CASES (tests/test_host_lzp.py writes it) is a run of records
//   u32 in_len, u32 cap, u32 exp_len (0xffffffff: a failure is expected),
//   u32 damage, the stream, the expected bytes
// Each stream is decoded into a heap buffer of exactly `cap` bytes from a heap
// copy of exactly in_len bytes (so that any overrun is a sanitizer report)
// and compared.  With damage != 0 the stream is then cut at every prefix
// length, decoded into every capacity below `cap` (all of them for a small
// cap, else the last 64 and 64 spread ones), and decoded with a byte changed
// at `damage` seeded positions: any result within the capacity is fine, a
// sanitizer report is not.  --time prints the decode time of each undamaged
// case per output byte.  Exit 0: everything as expected.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../fqzcomp5_amd/csrc/host_lzp.hpp"

static int decode(const uint8_t *z, size_t len, size_t cap, std::vector<uint8_t> *got) {
    // exact-size heap copies: the sanitizer sees the first byte out of bounds
    std::unique_ptr<uint8_t[]> in(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(in.get(), z, len);
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap ? cap : 1]);
    size_t n = 0;
    const bool ok = fqz5::host::unlzp(in.get(), len, out.get(), cap, &n);
    if (n > cap) return -2;
    if (ok && got) got->assign(out.get(), out.get() + n);
    return ok ? 0 : -1;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const bool timing = argc > 2 && !std::strcmp(argv[2], "--time");
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int bad = 0, cases = 0;
    long damaged = 0;
    uint32_t h[4];
    while (std::fread(h, 4, 4, f) == 4) {
        std::vector<uint8_t> z(h[0]), exp(h[2] == 0xffffffffu ? 0 : h[2]);
        if (std::fread(z.data(), 1, z.size(), f) != z.size() ||
            std::fread(exp.data(), 1, exp.size(), f) != exp.size())
            return 2;
        std::vector<uint8_t> got;
        const int rc = decode(z.data(), z.size(), h[1], &got);
        const bool want_fail = h[2] == 0xffffffffu;
        if (rc == -2 || want_fail != (rc != 0) || (!want_fail && got != exp)) {
            std::fprintf(stderr, "case %d: rc %d, %zu bytes (expected %s%zu)\n", cases, rc, got.size(),
                         want_fail ? "a failure, " : "", exp.size());
            bad++;
        }
        if (timing && !want_fail && !exp.empty()) {
            // the decoder alone, into memory already touched
            size_t n = 0;
            const auto b = std::chrono::steady_clock::now();
            fqz5::host::unlzp(z.data(), z.size(), got.data(), got.size(), &n);
            const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - b).count();
            std::printf("case %d: %zu bytes in, %zu out, %.2f ns per output byte\n", cases, z.size(),
                        exp.size(), ns / double(exp.size()));
        }
        if (h[3]) {
            for (size_t cut = 0; cut < z.size(); cut++, damaged++)
                if (decode(z.data(), cut, h[1], nullptr) == -2) bad++;
            // a capacity below the decoded size must fail (the stream decodes to exp.size())
            const size_t full = exp.size();
            for (size_t c = 0; c < full; c++) {
                if (full > 256 && c + 64 < full && c % (full / 64 + 1)) continue;
                if (decode(z.data(), z.size(), c, nullptr) != -1) bad++;
                damaged++;
            }
            uint64_t s = 0x9e3779b97f4a7c15ull + uint64_t(cases);
            for (uint32_t k = 0; k < h[3] && !z.empty(); k++, damaged++) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                std::vector<uint8_t> c2 = z;
                // towards markers and lengths: a changed byte becomes 233, 234 or any value
                const uint32_t pick = uint32_t(s >> 20) % 4u;
                c2[size_t(s >> 33) % c2.size()] = pick == 0 ? 233 : pick == 1 ? 234 : uint8_t(s >> 12);
                if (decode(c2.data(), c2.size(), h[1], nullptr) == -2) bad++;
            }
        }
        cases++;
    }
    std::fclose(f);
    std::printf("%d cases, %ld damaged streams, %d bad\n", cases, damaged, bad);
    return bad || !cases ? 1 : 0;
}
