// host_rans_check.cpp — a stand-alone checker of the host rANS 4x16 decoders
// (fqzcomp5_amd/csrc/host_rans.cpp), meant for sanitizer builds: no HIP, no
// Python, its own main.
//
//   c++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/host_rans_check.cpp fqzcomp5_amd/csrc/host_rans.cpp -o check
//   check CASES [--time]
//
// CASES (tests/test_host_rans.py writes it) is a run of records
//   u32 comp_len, u32 cap, u32 exp_len (0xffffffff: a failure is expected),
//   u32 damage, comp bytes, expected bytes
// Each stream is decoded into a heap buffer of exactly `cap` bytes from a heap
// copy of exactly comp_len bytes (so that any overrun is a sanitizer report)
// and compared.  With damage != 0 the stream is then cut at every prefix
// length and decoded with a byte flipped at `damage` seeded positions: any
// result is fine, a sanitizer report is not.  --time prints the decode time
// of each undamaged case per symbol.  Exit 0: everything as expected.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../fqzcomp5_amd/csrc/host_rans.hpp"

static int decode(const uint8_t *comp, size_t len, size_t cap, std::vector<uint8_t> *got) {
    // exact-size heap copies: the sanitizer sees the first byte out of bounds
    std::unique_ptr<uint8_t[]> in(new uint8_t[len ? len : 1]);
    std::memcpy(in.get(), comp, len);
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap ? cap : 1]);
    size_t n = 0;
    const int rc = fqz5::host::rans_dec_stream(in.get(), len, out.get(), cap, &n);
    if (rc == 0 && n > cap) return -2;
    if (rc == 0 && got) got->assign(out.get(), out.get() + n);
    return rc;
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
        std::vector<uint8_t> comp(h[0]), exp(h[2] == 0xffffffffu ? 0 : h[2]);
        if (std::fread(comp.data(), 1, comp.size(), f) != comp.size() ||
            std::fread(exp.data(), 1, exp.size(), f) != exp.size())
            return 2;
        std::vector<uint8_t> got;
        const int rc = decode(comp.data(), comp.size(), h[1], &got);
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
            fqz5::host::rans_dec_stream(comp.data(), comp.size(), got.data(), got.size(), &n);
            const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - b).count();
            std::printf("case %d: %zu symbols, order %d, %.2f ns per symbol\n", cases, exp.size(),
                        comp[0] & 1, ns / double(exp.size()));
        }
        if (h[3]) {
            for (size_t cut = 0; cut < comp.size(); cut++, damaged++)
                if (decode(comp.data(), cut, h[1], nullptr) == -2) bad++;
            uint64_t s = 0x9e3779b97f4a7c15ull + uint64_t(cases);
            for (uint32_t k = 0; k < h[3]; k++, damaged++) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                std::vector<uint8_t> c2 = comp;
                c2[size_t(s >> 33) % c2.size()] ^= uint8_t(1u + (s >> 20) % 255u);
                if (decode(c2.data(), c2.size(), h[1], nullptr) == -2) bad++;
            }
        }
        cases++;
    }
    std::fclose(f);
    std::printf("%d cases, %ld damaged streams, %d bad\n", cases, damaged, bad);
    return bad || !cases ? 1 : 0;
}
