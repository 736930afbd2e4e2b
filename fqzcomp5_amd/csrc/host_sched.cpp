// host_sched.cpp — see host_sched.hpp
#include <sched.h>
#include <algorithm>
#include <cstdlib>

#include "../../include/fqz5_mi355x.h"
#include "host_sched.hpp"

namespace fqz5 {
namespace host {

namespace {
// the plain rANS decoders of host_rans.cpp on one host core, ns per symbol:
// measured on the MI355X box's cores with 16 chains at once, the -3 bench's
// 44.5 M-symbol sequence chains and 22 M-symbol packed qualities
// (profiles/hostrans_step_trace.txt: 0.92-0.98 and 1.36-1.39)
constexpr double HOST_RANS_O0_NS = 1.0, HOST_RANS_O1_NS = 1.4;
// the encoder's bare chains (host_rans.cpp rans_enc_chain_o0 / _o1) on one core
// of the same box, ns per symbol: tools/host_rans_enc_check --time over 44.5 M
// symbols of the -3 bench's alphabets, alone and with 16 at once 0.64 and
// 0.83-0.84 ("Encode long rANS chains on host cores")
constexpr double HOST_RANS_ENC_O0_NS = 0.65, HOST_RANS_ENC_O1_NS = 0.85;
// ns per symbol [kind][gpu]: priors from r04 on MI355X boxes (host: the
// decoders of host_dec.cpp on one core of the box, the -5 Illumina hybrid
// step; GPU: k_fqz_dec_small 170-190, the general decoder with sequence
// contexts 350-470, k_seq_dec 290-380).  The plain rANS 4x16 chains: GPU
// 54.4 ns a step of 4 symbols for order-0 and 73.4 for order-1 (DESIGN.md
// section 4); host: HOST_RANS_O0_NS / _O1_NS above.  The encoder's bare
// chains: GPU 18.3 ns a step of 4 symbols for both orders (k_enc_chain2w,
// DESIGN.md section 4); host: HOST_RANS_ENC_O0_NS / _O1_NS above
std::atomic<double> g_ns[CK_N][2] = {{{30.0}, {330.0}}, {{16.0}, {180.0}}, {{24.0}, {400.0}},
                                     {{HOST_RANS_O0_NS}, {13.6}}, {{HOST_RANS_O1_NS}, {18.4}},
                                     {{HOST_RANS_ENC_O0_NS}, {4.6}}, {{HOST_RANS_ENC_O1_NS}, {4.6}}};
}  // namespace

double chain_ns(int kind, bool gpu) { return g_ns[kind][gpu ? 1 : 0].load(std::memory_order_relaxed); }

void chain_measured(int kind, bool gpu, double ns) {
    if (!(ns > 0.0) || kind < 0 || kind >= CK_N) return;
    std::atomic<double> &a = g_ns[kind][gpu ? 1 : 0];
    double cur = a.load(std::memory_order_relaxed);
    // an exponential average: a chain's cost moves with its data
    while (!a.compare_exchange_weak(cur, 0.5 * cur + 0.5 * ns, std::memory_order_relaxed)) {}
}

void measured(int kind, bool gpu, uint64_t n, double ns) {
    if (n >= CHAIN_MIN && ns > 0.0) chain_measured(kind, gpu, ns / double(n));
}

std::vector<char> plan(const std::vector<uint64_t> &n, const std::vector<int> &kind, int threads,
                       const std::vector<double> *core_ns, std::vector<double> *committed) {
    std::vector<char> host(n.size(), 0);
    std::vector<size_t> ord(n.size());
    for (size_t i = 0; i < ord.size(); i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
        return double(n[a]) * chain_ns(kind[a], false) > double(n[b]) * chain_ns(kind[b], false);
    });
    std::vector<double> core(size_t(std::max(threads, 1)), 0.0);   // each core's finish time
    if (core_ns) core = *core_ns;
    if (core.empty()) {                      // no core to give: every chain on the GPU
        if (committed) committed->clear();
        return host;
    }
    double gpu_t = 0.0;
    for (size_t i : ord) {
        auto lo = std::min_element(core.begin(), core.end());
        const double th = *lo + double(n[i]) * chain_ns(kind[i], false);
        const double tg = double(n[i]) * chain_ns(kind[i], true);
        double cmax = 0.0;
        for (double c : core) cmax = std::max(cmax, c);
        const double on_host = std::max({cmax, th, gpu_t});
        const double on_gpu = std::max({cmax, gpu_t, tg});
        if (on_host <= on_gpu) {
            *lo = th;
            host[i] = 1;
        } else {
            gpu_t = std::max(gpu_t, tg);
        }
    }
    if (committed) *committed = core;
    return host;
}

std::vector<char> place(int mode, const std::vector<uint64_t> &n, const std::vector<int> &kind,
                        uint64_t min_n, const std::vector<double> *core_ns, std::vector<double> *committed) {
    std::vector<char> on(n.size(), 0);
    if (mode == 0 || (core_ns && core_ns->empty())) return on;
    if (mode != 2) {
        for (size_t i = 0; i < on.size(); i++) on[i] = mode == 1 || i % 2 == 0;
        return on;
    }
    std::vector<size_t> at;                  // the chains long enough for the plan
    std::vector<uint64_t> ln;
    std::vector<int> lk;
    for (size_t i = 0; i < n.size(); i++)
        if (n[i] >= min_n) { at.push_back(i); ln.push_back(n[i]); lk.push_back(kind[i]); }
    const std::vector<char> p = plan(ln, lk, core_ns ? int(core_ns->size()) : threads(), core_ns, committed);
    for (size_t k = 0; k < at.size(); k++) on[at[k]] = p[k];
    return on;
}

int cores_of_rank() {
    // the cores this process may run on (its affinity mask, which
    // hardware_concurrency() ignores: a cgroup or taskset share), split
    // evenly among the ranks of this node that share it
    // ($LOCAL_WORLD_SIZE, set by torch.distributed.run), and no more than
    // the per-GPU CPU share the box states ($OMP_NUM_THREADS)
    int n = 0;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = int(std::max(1u, std::thread::hardware_concurrency()));
    if (const char *e = std::getenv("LOCAL_WORLD_SIZE")) {
        const int w = std::atoi(e);
        if (w > 1) n /= w;
    }
    if (const char *e = std::getenv("OMP_NUM_THREADS")) {
        const int o = std::atoi(e);
        if (o > 0) n = std::min(n, o);
    }
    return std::max(1, n);
}

int threads() {
    static const int n = [] {
        if (const char *e = std::getenv("FQZ5_HOST_THREADS")) return std::max(1, std::atoi(e));
        return std::min(16, cores_of_rank());
    }();
    return n;
}

bool step_trace() {
    static const bool on = std::getenv("FQZ5_STEP_TRACE") != nullptr;
    return on;
}

void Jobs::start(size_t n, std::function<void(size_t)> fn, size_t max_threads, size_t grain, size_t callers) {
    fn_ = std::move(fn);
    n_ = n;
    grain_ = std::max<size_t>(grain, 1);
    next_ = 0;
    size_t t = std::min((n + grain_ - 1) / grain_, size_t(threads()));
    if (max_threads) t = std::min(t, max_threads);
    for (size_t k = callers; k < t; k++) th_.emplace_back([this] { work(); });
}

void Jobs::work() noexcept {
    for (size_t i; (i = next_.fetch_add(grain_)) < n_;) {
        try {
            for (size_t k = i; k < std::min(n_, i + grain_); k++) fn_(k);
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu_);
            if (!err_) err_ = std::current_exception();
        }
    }
}

void Jobs::join() {
    for (auto &t : th_) t.join();
    th_.clear();
    std::exception_ptr e;
    std::swap(e, err_);
    if (e) std::rethrow_exception(e);
}

Jobs::~Jobs() {
    for (auto &t : th_) t.join();
}

void parallel_for(size_t n, const std::function<void(size_t)> &fn, size_t grain, size_t serial_below) {
    if (n < serial_below || threads() == 1) {
        for (size_t i = 0; i < n; i++) fn(i);
        return;
    }
    Jobs j;
    j.start(n, fn, 0, grain, 1);
    j.work();
    j.join();
}

}  // namespace host
}  // namespace fqz5

extern "C" void fqz5_host_plan(const uint64_t *n, const int *kind, int count, int threads,
                               const double *core_ns, char *on_host) {
    using namespace fqz5;
    const std::vector<uint64_t> nv(n, n + count);
    const std::vector<int> kv(kind, kind + count);
    std::vector<double> cores;
    if (core_ns) cores.assign(core_ns, core_ns + threads);
    const std::vector<char> on = host::plan(nv, kv, threads, core_ns ? &cores : nullptr);
    std::copy(on.begin(), on.end(), on_host);
}
