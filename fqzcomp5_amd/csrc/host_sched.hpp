// host_sched.hpp — the host cores beside the GPU: how many threads the
// library's pools use, which serial chains run on a core and which on the GPU
// (the cost model, plan, place), the pools' one worker loop (Jobs,
// parallel_for), one function on a thread of its own (Task) and the clocks of
// the step trace.  No HIP.
#pragma once
#include <time.h>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace fqz5 {
namespace host {

// Host threads of the library's pools (the decode chains, the name
// tokenisers, the table builders): $FQZ5_HOST_THREADS, else this rank's
// share of the cores: the process's affinity mask divided by
// $LOCAL_WORLD_SIZE, capped by $OMP_NUM_THREADS and at 16 (the CPU share of
// one GPU on the MI355X boxes).
int threads();
// the cores share above without the cap of 16
int cores_of_rank();

// Which chains run on host cores and which on the GPU (host_decode_mode() /
// host_encode_mode() 2, the default): the adaptive-model chains of a
// fqz5_decode_sections call (CK_SEQ, CK_FQZ, CK_FQZ_SEQ), and the plain rANS
// 4x16 order-0 / order-1 chains of every decompress_batch (CK_RANS_O0,
// CK_RANS_O1; rans_decompress.cpp run_djs).  A chain is serial whichever
// side runs it: on a host core it costs n x host_ns, and a host core takes
// one chain at a time; on the GPU each chain has a wave of its own (the
// launch lasts as long as its longest chain, n x gpu_ns).  The per-symbol
// costs start at committed measurements (profiles/r04_fqz_dec_bench.txt,
// DESIGN.md section 4) and follow what this process measures: every host
// chain's time, and every GPU batch's time over its longest chain (chains of
// CHAIN_MIN symbols and more only: measured()).  plan() places the chains
// longest first, each where the call's finish time (the later of the host
// cores' and the GPU's) grows least; ties go to the host.  core_ns: the
// cores' finish times (ns) before these chains, i.e. what an earlier plan of
// the same call committed (nullptr: `threads` idle cores); committed, when
// given, receives the cores' finish times after them.
// CK_RANS_ENC_O0 / _O1: the encoder's bare NX = 4 chains (host_rans.hpp
// rans_enc_chain_*), placed by Compressor::stage_encode (rans_compress.cpp).
enum ChainKind { CK_SEQ = 0, CK_FQZ = 1, CK_FQZ_SEQ = 2, CK_RANS_O0 = 3, CK_RANS_O1 = 4,
                 CK_RANS_ENC_O0 = 5, CK_RANS_ENC_O1 = 6, CK_N };
double chain_ns(int kind, bool gpu);
void chain_measured(int kind, bool gpu, double ns_per_symbol);
std::vector<char> plan(const std::vector<uint64_t> &n, const std::vector<int> &kind, int threads,
                       const std::vector<double> *core_ns = nullptr,
                       std::vector<double> *committed = nullptr);

// Under 2^20 symbols a rANS chain is not worth a core (it costs the launch
// under ~20 ms beside the others), nor does any chain's time tell a symbol's cost.
constexpr uint64_t CHAIN_MIN = 1u << 20;
// A host chain of n symbols, or a GPU launch whose longest chain has n, took
// ns: chain_measured() of ns / n, unless n < CHAIN_MIN or ns is not positive.
void measured(int kind, bool gpu, uint64_t n, double ns);

// 1 for every chain that runs on a host core, by the host mode of the caller
// (host_decode_mode() / host_encode_mode()): 0 none, 1 every chain, 2 by
// plan() among the chains of min_n symbols and more (in their given order;
// the shorter ones stay on the GPU), 3 every other chain of the given order
// (tests).  core_ns as for plan() (nullptr: threads() idle cores); no core
// to give (an empty core_ns) leaves every chain on the GPU.  Only mode 2
// writes committed.
std::vector<char> place(int mode, const std::vector<uint64_t> &n, const std::vector<int> &kind,
                        uint64_t min_n, const std::vector<double> *core_ns = nullptr,
                        std::vector<double> *committed = nullptr);

// The host cores a decompress_batch may give its rANS chains within a
// fqz5_decode_sections call: the cores not running that call's
// adaptive-model chains, with their finish times (ns; all zero: idle).  A
// call without one plans against threads() idle cores.
struct CoreBudget {
    std::vector<double> core_ns;
};

// fn(i) for i in [0, n) on up to threads() host threads (max_threads, when
// given, lowers that), started by start() and waited for by join() (or the
// destructor).  The indices come `grain` at a time off a shared counter, so
// long and short items balance.  An exception of fn ends its grain only: the
// other indices still run, join() rethrows the first one (once), and the
// destructor only waits.
class Jobs {
  public:
    void start(size_t n, std::function<void(size_t)> fn, size_t max_threads = 0, size_t grain = 1,
               size_t callers = 0);             // callers: threads that will call work() themselves
    void work() noexcept;                       // the worker loop: until no index is left
    void join();
    size_t running() const { return th_.size(); }
    ~Jobs();

  private:
    std::function<void(size_t)> fn_;
    size_t n_ = 0, grain_ = 1;
    std::atomic<size_t> next_{0};
    std::mutex mu_;
    std::exception_ptr err_;
    std::vector<std::thread> th_;
};

// Jobs' counterpart for a single function: fn() on a thread of its own, started
// by the constructor; an empty fn starts none.  An exception of fn is kept:
// join() waits and rethrows it (once), the destructor only waits, so a scope
// that unwinds leaves no thread of its own behind.  What fn refers to must be
// declared before the Task.
class Task {
  public:
    Task() = default;
    explicit Task(std::function<void()> fn) {
        if (!fn) return;
        err_ = std::make_unique<std::exception_ptr>();
        th_ = std::thread([fn = std::move(fn), e = err_.get()] {
            try {
                fn();
            } catch (...) {
                *e = std::current_exception();
            }
        });
    }
    Task(Task &&) = default;
    Task &operator=(Task &&o) {                 // (waits for its own function first)
        wait();
        err_ = std::move(o.err_);
        th_ = std::move(o.th_);
        return *this;
    }
    bool running() const { return th_.joinable(); }   // started and not waited for yet
    void join() {
        wait();
        if (err_ && *err_) std::rethrow_exception(std::exchange(*err_, nullptr));
    }
    ~Task() { wait(); }

  private:
    void wait() { if (th_.joinable()) th_.join(); }
    std::unique_ptr<std::exception_ptr> err_;
    std::thread th_;
};

// Jobs, blocking: the caller works too and gets the first exception of fn;
// fn(i) must touch item i only.  Fewer than serial_below items, or one host
// thread, run on the caller alone.
void parallel_for(size_t n, const std::function<void(size_t)> &fn, size_t grain, size_t serial_below);

// $FQZ5_STEP_TRACE: host wall times of the phases on stderr
bool step_trace();
// the steady clock
inline double now_ns() {
    return std::chrono::duration<double, std::nano>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline double now_ms() { return now_ns() * 1e-6; }
// the calling thread's CPU time (0 when the clock is refused)
inline double thread_cpu_ns() {
    timespec t;
    if (clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t)) return 0;
    return double(t.tv_sec) * 1e9 + double(t.tv_nsec);
}

}  // namespace host
}  // namespace fqz5
