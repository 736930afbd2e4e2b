// host_rans_enc_check.cpp — a stand-alone checker of the encoder's bare rANS
// 4x16 chains on a host core (fqzcomp5_amd/csrc/host_rans.cpp
// rans_enc_chain_o0 / _o1), meant for sanitizer builds: no HIP, no Python, its
// own main.
//
//   c++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/host_rans_enc_check.cpp fqzcomp5_amd/csrc/host_rans.cpp -o check
//   check CASES [--time]
//
// CASES (tests/test_host_rans_enc.py writes it) is a run of records
//   u32 n, u32 order, u32 bits, u32 nfreq, u32 nwords,
//   n input bytes, nfreq x {u32 index, u32 frequency}, nwords x u32
// index = the symbol (order 0) or context * 256 + symbol (order 1); the words
// are the expected checkpoints (nwords = 0: none to compare, a timing case).
// The chain runs from a heap copy of exactly n input bytes into a heap array of
// exactly rans_enc_ck_words() words, so that any overrun is a sanitizer
// report.  --time prints each case's chain time per symbol (the chain alone,
// the second of two runs).  Exit 0: everything as expected.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../fqzcomp5_amd/csrc/host_rans.hpp"
#include "../fqzcomp5_amd/csrc/rans_format.hpp"

using fqz5::EncSym;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const bool timing = argc > 2 && !std::strcmp(argv[2], "--time");
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int bad = 0, cases = 0;
    uint32_t h[5];
    while (std::fread(h, 4, 5, f) == 5) {
        const size_t n = h[0];
        const bool o1 = h[1] != 0;
        const int bits = int(h[2]);
        std::vector<uint32_t> fr(size_t(h[3]) * 2), exp(h[4]);
        // exact-size heap copy: the sanitizer sees the first byte out of bounds
        std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
        if (!n || std::fread(in.get(), 1, n, f) != n ||
            std::fread(fr.data(), 4, fr.size(), f) != fr.size() ||
            std::fread(exp.data(), 4, exp.size(), f) != exp.size())
            return 2;
        // the job's tables as the compressor makes them: order 0 the 256
        // symbols; order 1 the alphabet (0 and every byte of the input), its
        // A x A frequencies, and from those the encoder symbols
        std::vector<EncSym> tab;
        uint8_t remap[256] = {0};
        int A = 0;
        if (!o1) {
            std::vector<uint32_t> F(256, 0);
            for (size_t k = 0; k < fr.size(); k += 2) F[fr[k] & 255u] = fr[k + 1];
            tab.assign(256, EncSym{0, 0, 0, 0});
            for (uint32_t s = 0, x = 0; s < 256; s++)
                if (F[s]) { tab[s] = fqz5::make_encsym(x, F[s], bits); x += F[s]; }
        } else {
            bool present[256] = {true};
            for (size_t i = 0; i < n; i++) present[in[i]] = true;
            for (int s = 0; s < 256; s++)
                if (present[s]) remap[s] = uint8_t(A++);
            std::vector<uint16_t> f1(size_t(A) * A, 0);
            for (size_t k = 0; k < fr.size(); k += 2) {
                const uint32_t c = (fr[k] >> 8) & 255u, s = fr[k] & 255u;
                if (present[c] && present[s]) f1[size_t(remap[c]) * A + remap[s]] = uint16_t(fr[k + 1]);
            }
            tab.resize(size_t(A) * A);
            fqz5::host::rans_enc_tab_o1(f1.data(), A, bits, tab.data());
        }
        const size_t words = fqz5::host::rans_enc_ck_words(n, o1);
        std::unique_ptr<uint32_t[]> ck(new uint32_t[words]);
        double ns = 0;
        for (int run = 0; run < (timing ? 2 : 1); run++) {
            std::memset(ck.get(), 0xa5, words * 4);
            const auto b = std::chrono::steady_clock::now();
            if (o1) fqz5::host::rans_enc_chain_o1(tab.data(), remap, A, in.get(), n, ck.get());
            else fqz5::host::rans_enc_chain_o0(tab.data(), in.get(), n, ck.get());
            ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - b).count();
        }
        if (!exp.empty() &&
            (exp.size() != words || std::memcmp(exp.data(), ck.get(), words * 4) != 0)) {
            std::fprintf(stderr, "case %d (n %zu, order %d, bits %d): %zu words, expected %zu%s\n", cases, n,
                         int(o1), bits, words, exp.size(), exp.size() == words ? ", contents differ" : "");
            bad++;
        }
        if (timing)
            std::printf("case %d: %zu symbols, order %d, alphabet %d, %.2f ns per symbol\n", cases, n, int(o1),
                        o1 ? A : int(fr.size() / 2), ns / double(n));
        cases++;
    }
    std::fclose(f);
    std::printf("%d cases, %d bad\n", cases, bad);
    return bad || !cases ? 1 : 0;
}
