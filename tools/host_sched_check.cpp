// host_sched_check.cpp — a stand-alone checker of the host scheduling module
// (fqzcomp5_amd/csrc/host_sched.cpp), meant for sanitizer builds: no HIP, no
// Python, its own main.
//
//   c++ -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/host_sched_check.cpp fqzcomp5_amd/csrc/host_sched.cpp -o check
//   c++ -O1 -g -pthread -fsanitize=thread (the same two files)
//   FQZ5_HOST_THREADS=4 check
//
// It checks place() against its rule and against plan(), measured() against
// chain_ns(), the two front ends of the worker loop (parallel_for, Jobs):
// every index once, the thread caps, and what a throwing item does; and Task:
// when it starts a thread, where its function's exception goes, and that a
// scope never leaves one running.  Exit 0
// and nothing on stderr: everything as expected (tests/test_host_sched.py).
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../fqzcomp5_amd/csrc/host_sched.hpp"

using namespace fqz5::host;

static int g_bad = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);              \
            g_bad++;                                                             \
        }                                                                        \
    } while (0)

static std::string str(const std::vector<char> &v) {
    std::string s;
    for (char c : v) s += c ? '1' : '0';
    return s;
}

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint64_t rnd(uint64_t below) {           // a seeded xorshift: the same inputs everywhere
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return g_seed % below;
}

// the mode switch on the untouched priors (host 1.0 ns, GPU 13.6 ns a symbol:
// every long chain finishes sooner on one of 16 idle cores)
static void check_place_rule() {
    const std::vector<uint64_t> n = {3u << 20, 100, 2u << 20, 5u << 20, 7};
    const std::vector<int> kind(n.size(), CK_RANS_O0);
    const std::vector<double> idle(16, 0.0), none;
    const char *want[4] = {"00000", "11111", "10110", "10101"};
    for (int mode = 0; mode < 4; mode++) {
        CHECK(str(place(mode, n, kind, CHAIN_MIN, &idle)) == want[mode]);
        CHECK(str(place(mode, n, kind, CHAIN_MIN, &none)) == "00000");
    }
}

static void check_place_against_plan() {
    for (int round = 0; round < 50; round++) {
        const size_t count = 1 + rnd(40), ncore = 1 + rnd(16);
        std::vector<uint64_t> n(count);
        std::vector<int> kind(count);
        for (size_t i = 0; i < count; i++) {
            n[i] = 1 + rnd(rnd(2) ? 8u << 20 : 2u << 20);     // on both sides of CHAIN_MIN
            kind[i] = int(rnd(CK_N));
        }
        std::vector<double> cores(ncore);
        for (double &c : cores) c = rnd(3) ? double(rnd(50000000)) : 0.0;
        // every length: plan on the same arguments
        std::vector<double> c0, c1;
        const std::vector<char> p0 = plan(n, kind, int(ncore), &cores, &c0);
        CHECK(place(2, n, kind, 0, &cores, &c1) == p0);
        CHECK(c0 == c1);
        // the long ones: plan on the filtered list, scattered back
        std::vector<uint64_t> ln;
        std::vector<int> lk;
        std::vector<size_t> at;
        for (size_t i = 0; i < count; i++)
            if (n[i] >= CHAIN_MIN) { ln.push_back(n[i]); lk.push_back(kind[i]); at.push_back(i); }
        const std::vector<char> pl = plan(ln, lk, int(ncore), &cores, &c0);
        std::vector<char> want(count, 0);
        for (size_t k = 0; k < at.size(); k++) want[at[k]] = pl[k];
        CHECK(place(2, n, kind, CHAIN_MIN, &cores, &c1) == want);
        CHECK(c0 == c1);
        // the other modes leave committed alone
        std::vector<double> keep = {1.0, 2.0};
        for (int mode : {0, 1, 3}) {
            place(mode, n, kind, CHAIN_MIN, &cores, &keep);
            CHECK(keep.size() == 2 && keep[0] == 1.0 && keep[1] == 2.0);
        }
    }
}

static void check_measured() {
    const double was = chain_ns(CK_RANS_O1, true);
    measured(CK_RANS_O1, true, CHAIN_MIN - 1, 1e9);
    CHECK(chain_ns(CK_RANS_O1, true) == was);
    measured(CK_RANS_O1, true, CHAIN_MIN, 0.0);
    measured(CK_RANS_O1, true, CHAIN_MIN, -5.0);
    CHECK(chain_ns(CK_RANS_O1, true) == was);
    const double ns = 40.0 * double(CHAIN_MIN);
    measured(CK_RANS_O1, true, CHAIN_MIN, ns);
    CHECK(chain_ns(CK_RANS_O1, true) == 0.5 * was + 0.5 * (ns / double(CHAIN_MIN)));
    CHECK(chain_ns(CK_RANS_O1, false) == 1.4);             // the other side untouched
    std::vector<double> all;
    for (int k = 0; k < CK_N; k++) { all.push_back(chain_ns(k, false)); all.push_back(chain_ns(k, true)); }
    measured(-1, false, CHAIN_MIN, ns);
    measured(CK_N, true, CHAIN_MIN, ns);
    for (int k = 0; k < CK_N; k++)
        CHECK(chain_ns(k, false) == all[size_t(2 * k)] && chain_ns(k, true) == all[size_t(2 * k + 1)]);
}

struct Boom : std::runtime_error {
    Boom() : std::runtime_error("boom") {}
};

static void check_parallel_for() {
    const size_t sizes[] = {0, 1, 63, 64, 1000};
    const size_t setting[2][2] = {{16, 64}, {1, 2}};
    for (size_t n : sizes)
        for (const auto &s : setting) {
            std::vector<std::atomic<int>> seen(n);
            for (auto &a : seen) a = 0;
            parallel_for(n, [&](size_t i) { seen[i]++; }, s[0], s[1]);
            for (size_t i = 0; i < n; i++) CHECK(seen[i] == 1);
            if (!n) continue;
            // item n / 2 throws: the call throws that, once no thread is inside fn
            std::atomic<int> inside{0}, calls{0};
            bool thrown = false;
            try {
                parallel_for(n, [&](size_t i) {
                    inside++;
                    calls++;
                    if (i == n / 2) { inside--; throw Boom(); }
                    inside--;
                }, s[0], s[1]);
            } catch (const Boom &) {
                thrown = true;
            }
            CHECK(thrown);
            CHECK(inside == 0);
            CHECK(calls >= 1 && size_t(calls) <= n);
        }
}

static void check_jobs() {
    const size_t hw = size_t(threads());
    Jobs jobs;
    for (size_t cap : {size_t(0), size_t(1), size_t(2)}) {       // (a second start after join, too)
        const size_t n = 200;
        std::vector<std::atomic<int>> seen(n);
        for (auto &a : seen) a = 0;
        std::atomic<int> inside{0}, most{0};
        jobs.start(n, [&](size_t i) {
            const int now = ++inside;
            int m = most.load();
            while (now > m && !most.compare_exchange_weak(m, now)) {}
            seen[i]++;
            inside--;
        }, cap);
        const size_t limit = cap ? std::min(cap, hw) : hw;
        CHECK(jobs.running() >= 1 && jobs.running() <= limit);
        jobs.join();
        CHECK(jobs.running() == 0);
        CHECK(size_t(most) <= limit);
        for (size_t i = 0; i < n; i++) CHECK(seen[i] == 1);
    }
    jobs.start(0, [](size_t) {});
    CHECK(jobs.running() == 0);
    jobs.join();
    // a throwing task: the others still run, join() throws once
    {
        const size_t n = 50;
        std::vector<std::atomic<int>> seen(n);
        for (auto &a : seen) a = 0;
        jobs.start(n, [&](size_t i) {
            seen[i]++;
            if (i == 7 || i == 30) throw Boom();
        });
        int thrown = 0;
        try { jobs.join(); } catch (const Boom &) { thrown++; }
        try { jobs.join(); } catch (const Boom &) { thrown++; }
        CHECK(thrown == 1);
        for (size_t i = 0; i < n; i++) CHECK(seen[i] == 1);
        // and the list is clean for the next start
        jobs.start(n, [&](size_t i) { seen[i]++; });
        jobs.join();
        for (size_t i = 0; i < n; i++) CHECK(seen[i] == 2);
    }
    // the destructor waits and stays quiet
    std::atomic<int> ran{0};
    {
        Jobs quiet;
        quiet.start(20, [&](size_t i) {
            ran++;
            if (i % 5 == 0) throw Boom();
        });
    }
    CHECK(ran == 20);
}

// one function on a thread of its own
static void check_task() {
    std::atomic<int> ran{0};
    {
        Task t([&] { ran++; });
        CHECK(t.running());
        t.join();
        CHECK(!t.running());
        t.join();                                 // (nothing left to wait for)
    }
    CHECK(ran == 1);
    // an empty function starts no thread
    Task none{std::function<void()>()};
    CHECK(!none.running());
    none.join();
    CHECK(!Task().running());
    // an exception comes out of join() exactly once
    {
        Task t([] { throw Boom(); });
        int thrown = 0;
        try { t.join(); } catch (const Boom &) { thrown++; }
        try { t.join(); } catch (const Boom &) { thrown++; }
        CHECK(thrown == 1);
    }
    // the destructor after an unjoined failure waits and stays quiet
    {
        Task quiet([&] { ran++; throw Boom(); });
    }
    CHECK(ran == 2);
    // a moved task keeps its function's exception; assignment waits for the old one
    {
        Task a([&] { ran++; });
        a = Task([] { throw Boom(); });
        CHECK(ran == 3);
        Task b(std::move(a));
        CHECK(!a.running() && b.running());
        bool thrown = false;
        try { b.join(); } catch (const Boom &) { thrown = true; }
        CHECK(thrown);
        a.join();
    }
    // a scope that unwinds from an exception of its own while two helpers
    // still run: both have finished (the flag is the last thing each sets)
    // before the catch block runs
    std::atomic<int> go{0}, done_a{0}, done_b{0};
    bool caught = false;
    try {
        Task a([&] { while (!go) std::this_thread::yield(); done_a = 1; });
        Task b([&] { while (!go) std::this_thread::yield(); done_b = 1; throw Boom(); });
        CHECK(done_a == 0 && done_b == 0);        // (both wait for `go`)
        go = 1;
        throw std::runtime_error("the scope's own");
    } catch (const std::runtime_error &e) {
        caught = std::string(e.what()) == "the scope's own";
        CHECK(done_a == 1 && done_b == 1);
    }
    CHECK(caught);
}

int main() {
    check_place_rule();                 // (first: it reads the priors)
    check_place_against_plan();
    check_measured();
    check_parallel_for();
    check_jobs();
    check_task();
    if (g_bad) return 1;
    std::printf("host_sched_check: ok (%d host threads)\n", threads());
    return 0;
}
