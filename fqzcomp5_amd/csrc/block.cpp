// block.cpp — fqzcomp5's per-block section coder for the sequence and
// quality sections (fqzcomp5.c:1899-2280), driving the batched GPU rANS
// codec.
//
// The reference encodes one block at a time per worker thread, trying every
// method of the section's mask while the codec trial is running
// (metrics_method / compress_with_methods, fqzcomp5.c:1899-2144).  Here a
// whole run of blocks is handed over at once: the candidates of every block
// are compressed in one try session (every method of the trial blocks; for
// the others every rANS method, or with a staged try only the trial's pick,
// predicted from the trial blocks' sizes: the long chains run on host cores,
// one core each, so a candidate nobody reads is not free), then the trial
// state machine is replayed on the host in block order, which gives exactly
// the choices of a single-threaded (-t1) reference run.
//
// The try and the commit share their machinery: a Candidates holds the
// requests of every coder family with one [section][method] table of where
// each candidate lives, collect() is the one place that maps a method to its
// family, size() / layout() read a candidate back, and run_candidates() codes
// a Candidates: spread over the thread's helper contexts (the try), or with
// only the fqz candidates on helpers (the commit's late encodes, and a try of
// rANS candidates only).  Every helper thread is a host::Task started through
// on_ctx(): joined, at the latest, when its scope unwinds.
#include <atomic>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <thread>
#include <deque>
#include <memory>
#include <vector>

#include "../../include/fqz5_block.h"
#include "rans_codec.hpp"
#include "fqz_codec.hpp"
#include "seq_codec.hpp"
#include "seq_cm.h"
#include "lzp_codec.hpp"
#include "names.hpp"
#include "host_dec.hpp"
#include "rans_format.hpp"

namespace fqz5 {

GpuCtx &gpu();
void fqz5_set_error(const char *msg);

namespace {

// fqzcomp5.c:185-208
enum Method {
    RANS0 = 1, RANS1, RANS64, RANS65, RANS128, RANS129, RANS192, RANS193,
    RANSXN1, LZP3, SEQ10 = 20, SEQ12, SEQ12B, SEQ13B, SEQ14B, SEQ_CUSTOM,
    FQZ0 = 26, FQZ1, FQZ2, FQZ3, FQZ4, M_LAST = 31
};
constexpr uint32_t RANS_MASK =
    (1u << RANS0) | (1u << RANS1) | (1u << RANS64) | (1u << RANS65) |
    (1u << RANS128) | (1u << RANS129) | (1u << RANS192) | (1u << RANS193) |
    (1u << RANSXN1);
constexpr uint32_t FQZ_MASK =
    (1u << FQZ0) | (1u << FQZ1) | (1u << FQZ2) | (1u << FQZ3) | (1u << FQZ4);

constexpr uint32_t SEQ_MASK =
    (1u << SEQ10) | (1u << SEQ12) | (1u << SEQ12B) | (1u << SEQ13B) | (1u << SEQ14B);
constexpr uint32_t NAME_MASK = ((1u << (M_TOK3_9_LZP + 1)) - 1) & ~((1u << M_TLZP3) - 1);

bool is_fqz(int m) { return m >= FQZ0 && m <= FQZ4; }
bool is_seqcm(int m) { return m >= SEQ10 && m <= SEQ14B; }

// encode_seq's parameters per method and the section strat byte
// (k << 4) | (both << 3) | 1 (fqzcomp5.c:2047-2062)
SeqEncReq seq_req(const fqz5_section &S, int m) {
    static const int slevel[] = {10, 12, 12, 13, 14}, both[] = {0, 0, 1, 1, 1};
    SeqEncReq r;
    r.d_in = S.in;
    r.n = S.in_size;
    r.lens = S.rec_len;
    r.nrec = S.nrec;
    r.k = slevel[m - SEQ10];
    r.both = both[m - SEQ10];
    return r;
}
int seq_strat(int m) {
    static const int slevel[] = {10, 12, 12, 13, 14}, both[] = {0, 0, 1, 1, 1};
    return (slevel[m - SEQ10] << 4) | (both[m - SEQ10] << 3) | 1;
}

// order word per rANS method (fqzcomp5.c:1992-2010)
int method_order(int m, uint32_t fixed_len) {
    static const int ord[] = {0, 1, 64, 65, 128, 129, 192, 193};
    if (m >= RANS0 && m <= RANS193) return ord[m - RANS0];
    return int((fixed_len << 8) + 9);   // RANSXN1, incl. the >=256 aliasing
}

// The trial's pick among the methods of `among` (fqzcomp5.c:1913-1924): the
// smallest (csize + 1) / usize, the first one on a tie; 0 if none was tried.
int pick_method(const fqz5_section_stats &s, uint32_t among) {
    int best_m = 0;
    double best = 1e30;
    for (int m = 0; m < FQZ5_M_LAST; m++) {
        if (!(among & (1u << m))) continue;
        if (s.usize[m] && best > (s.csize[m] + 1.0) / s.usize[m]) {
            best = (s.csize[m] + 1.0) / s.usize[m];
            best_m = m;
        }
    }
    return best_m;
}

// metrics_method (fqzcomp5.c:1899-1946)
uint32_t metrics_method(fqz5_trial_state &st, int sec, uint32_t avail) {
    fqz5_section_stats &s = st.sec[sec];
    if (s.review <= 0) {
        s.review = FQZ5_METRICS_REVIEW;
        s.trial = FQZ5_METRICS_TRIAL;
        std::memset(s.usize, 0, sizeof s.usize);
        std::memset(s.csize, 0, sizeof s.csize);
        std::memset(s.count, 0, sizeof s.count);
    }
    if (s.trial > 0) return avail;
    if (s.trial > -99999) {
        s.method_used = pick_method(s, ~0u);
        s.trial = -99999;
        return 1u << s.method_used;
    }
    s.review--;
    return 1u << s.method_used;
}

// metrics_method's counters without the sizes: what the next section of a
// kind does.  Which sections try every method (trial and re-trial blocks)
// does not depend on the outcomes.
enum TrialStep { STEP_TRIAL, STEP_DECIDE, STEP_KEEP };
TrialStep trial_step(fqz5_section_stats &ss, bool *fresh = nullptr) {
    if (ss.review <= 0) {
        ss.review = FQZ5_METRICS_REVIEW;
        ss.trial = FQZ5_METRICS_TRIAL;
        if (fresh) *fresh = true;
    }
    if (ss.trial > 0) {
        ss.trial--;
        return STEP_TRIAL;
    }
    if (ss.trial > -99999) {
        ss.trial = -99999;
        return STEP_DECIDE;
    }
    ss.review--;
    return STEP_KEEP;
}

// One decision of a staged try (fqz5_sections_try_staged): a trial window of
// a kind whose remaining sections lie in the call, and the sections after it
// that take its pick.
struct Decision {
    int kind = 0;
    bool fresh = false;            // the window began in the call: its sums start at zero
    std::vector<int> rows;         // the window's sections in the call
    std::vector<int> follow;       // the sections coded with its pick
};

// The role of every section of a call (file order) from the trial state
// before its first section; see fqz5_staged_plan.
void staged_walk(const int32_t *sec_ids, int nsec, const uint32_t *avail,
                 const fqz5_trial_state *st, int32_t *roles, uint32_t *masks, int32_t *window,
                 std::vector<Decision> *decs) {
    fqz5_trial_state s = *st;
    int cur[FQZ5_SEC_LAST], nwin[FQZ5_SEC_LAST], settled[FQZ5_SEC_LAST];
    bool open[FQZ5_SEC_LAST];      // the kind's last window still takes trial sections
    for (int k = 0; k < FQZ5_SEC_LAST; k++) {
        cur[k] = -1;               // index in *decs of the decision that governs, -1: the state
        nwin[k] = 0;
        settled[k] = s.sec[k].method_used;
        open[k] = false;
    }
    std::vector<Decision> local;
    std::vector<Decision> &D = decs ? *decs : local;
    for (int i = 0; i < nsec; i++) {
        const int k = sec_ids[i];
        fqz5_section_stats &ss = s.sec[k];
        const bool staged = k == FQZ5_SEC_SEQ || k == FQZ5_SEC_QUAL;
        bool fresh = false;
        const TrialStep step = trial_step(ss, &fresh);
        window[i] = -1;
        if (step == STEP_TRIAL) {
            roles[i] = staged ? FQZ5_ROLE_TRIAL : FQZ5_ROLE_OTHER;
            masks[i] = avail[k];
            if (!staged) continue;
            if (!open[k]) {
                Decision d;
                d.kind = k;
                d.fresh = fresh;
                cur[k] = int(D.size());
                D.push_back(d);
                open[k] = true;
                nwin[k]++;
            }
            D[size_t(cur[k])].rows.push_back(i);
            window[i] = nwin[k] - 1;
            continue;
        }
        if (!staged) {
            roles[i] = FQZ5_ROLE_OTHER;
            masks[i] = 0;
            continue;
        }
        if (step == STEP_DECIDE && !open[k]) {
            // the window ended before the call: its sums are in the state
            settled[k] = pick_method(st->sec[k], ~0u);
            cur[k] = -1;
        }
        open[k] = false;
        if (cur[k] >= 0) {
            roles[i] = FQZ5_ROLE_FOLLOW;
            masks[i] = 0;
            window[i] = nwin[k] - 1;
            D[size_t(cur[k])].follow.push_back(i);
        } else {
            roles[i] = FQZ5_ROLE_SETTLED;
            masks[i] = 1u << settled[k];
        }
    }
}

}  // namespace

using host::now_ms;
using host::now_ns;
using host::step_trace;

// compress_with_methods' rANS call of method m (fqzcomp5.c:1992-2010)
CompressReq rans_req(const fqz5_section &S, int m) {
    CompressReq r;
    r.d_in = S.in;
    r.n = S.in_size;
    r.order = method_order(m, S.fixed_len);
    r.cap = compress_bound(r.n, r.order);
    return r;
}

// An fqz or sequence-model candidate whose range chain was skipped (pruned, or
// a bounds-only try): no bytes yet, its size as the interval [lb, ub].
struct Bound {
    bool skip = false;
    uint64_t lb = 0, ub = 0;
};

// The candidates of a run of sections, by coder family, and where the
// candidate of (section, method) lives.
enum Family { FAM_NONE = 0, FAM_RANS, FAM_FQZ, FAM_SEQ, FAM_NAME };
struct Candidates {
    struct Slot { int fam = FAM_NONE, idx = -1; };
    int nsec = 0;
    std::vector<Slot> slots;                      // [nsec][FQZ5_M_LAST]
    std::vector<CompressReq> rans;                // every rANS stream, once it ran LZP3's and the stripes' too
    std::vector<CompressReq> stripes;             // RANSXN1 (stripe) candidates until join_stripes()
    std::vector<int> stripe_sec;
    std::vector<int> lzp_sec;                     // sections trying LZP3 until join_lzp()
    std::vector<FqzEncReq> fqz;                   // FQZ candidates
    std::vector<SeqEncReq> seq;                   // sequence CM candidates
    std::vector<Bound> fqz_b, seq_b;              // one each
    std::deque<std::vector<uint32_t>> recs;       // their (rewritable) lengths / flags
    std::vector<int> name_sec, name_meth;         // name-section candidates
    std::vector<NameEnc> names;                   // ... and their host bytes

    explicit Candidates(int n = 0) : nsec(n), slots(size_t(std::max(n, 0)) * FQZ5_M_LAST) {}
    Slot &at(int i, int m) { return slots[size_t(i) * FQZ5_M_LAST + size_t(m)]; }
    Slot get(int i, int m) const {
        return m > 0 && m < FQZ5_M_LAST ? slots[size_t(i) * FQZ5_M_LAST + size_t(m)] : Slot();
    }
    // the index of (i, m) in family fam's vector, -1 if it is no such candidate
    int find(int i, int m, int fam) const {
        const Slot s = get(i, m);
        return s.fam == fam ? s.idx : -1;
    }
    void put_rans(int i, int m, CompressReq &&r) {
        at(i, m) = {FAM_RANS, int(rans.size())};
        rans.push_back(std::move(r));
    }
    void join_stripes() {                          // the stripe candidates join the batch
        for (size_t k = 0; k < stripes.size(); k++) put_rans(stripe_sec[k], RANSXN1, std::move(stripes[k]));
        stripes.clear();
        stripe_sec.clear();
    }
    void join_lzp(std::vector<CompressReq> &&lzr) {   // the LZP3 streams (one per lzp_sec) join the batch
        for (size_t k = 0; k < lzp_sec.size(); k++) put_rans(lzp_sec[k], LZP3, std::move(lzr[k]));
        lzp_sec.clear();
    }
    // candidates whose cost grows with their work, or whose host work is worth
    // a thread: those the try runs on helper contexts
    bool wants_helpers() const {
        return !fqz.empty() || !seq.empty() || !lzp_sec.empty() || !stripes.empty() || !name_sec.empty();
    }
    // the coder of (i, m) ran, whatever came of it: not a candidate whose
    // range chain was skipped (those have no bytes)
    bool coded(int i, int m) const {
        const Slot s = get(i, m);
        if (s.fam == FAM_FQZ) return !fqz_b[size_t(s.idx)].skip;
        if (s.fam == FAM_SEQ) return !seq_b[size_t(s.idx)].skip;
        return s.fam != FAM_NONE;
    }
    // The size of (i, m) as compress_with_methods sees it: UINT_MAX when not
    // run, 0 when the codec returned NULL (out_len = *out_size = 0); a
    // skipped candidate's lower bound, with its upper bound in *upper (else
    // the size again).  *stale is the section's last good name size, for
    // m = 0, 1, ... in turn: encode_names returns NULL without writing
    // *out_size, so a failing name candidate is seen with the size the
    // previous name candidate of this section wrote (fqzcomp5.c:2036-2044,
    // :1433-1440); never strictly the best, but it enters the trial's totals
    // (metrics_update) and can win the later blocks
    uint32_t size(int i, int m, uint32_t *upper = nullptr, uint32_t *stale = nullptr) const {
        auto clip = [](uint64_t v) { return uint32_t(std::min<uint64_t>(v, UINT32_MAX - 1)); };
        const Slot s = get(i, m);
        uint32_t sz = UINT32_MAX, up = 0;
        if (s.fam == FAM_RANS) sz = rans[size_t(s.idx)].ok ? layout_size(rans[size_t(s.idx)].out) : 0;
        // a name candidate's size is its whole section (encode_names' *out_size)
        if (s.fam == FAM_NAME) {
            const NameEnc &E = names[size_t(s.idx)];
            sz = E.ok ? uint32_t(E.out.size()) : stale ? *stale : UINT32_MAX;
            if (E.ok && stale) *stale = sz;
        }
        if (s.fam == FAM_FQZ || s.fam == FAM_SEQ) {
            const Bound &b = s.fam == FAM_FQZ ? fqz_b[size_t(s.idx)] : seq_b[size_t(s.idx)];
            const Layout *l = layout(i, m);
            sz = l ? layout_size(*l) : b.lb ? clip(b.lb) : 0;
            if (!l && b.ub) up = clip(b.ub);
        }
        if (upper) *upper = up ? up : sz;
        return sz;
    }
    // the bytes of (i, m) if it was coded, else null (a name candidate's are in name())
    const Layout *layout(int i, int m) const {
        const Slot s = get(i, m);
        if (s.fam == FAM_RANS && rans[size_t(s.idx)].ok) return &rans[size_t(s.idx)].out;
        if (s.fam == FAM_FQZ && fqz[size_t(s.idx)].ok) return &fqz[size_t(s.idx)].out;
        if (s.fam == FAM_SEQ && seq[size_t(s.idx)].ok) return &seq[size_t(s.idx)].out;
        return nullptr;
    }
    const NameEnc *name(int i, int m) const {
        const Slot s = get(i, m);
        return s.fam == FAM_NAME ? &names[size_t(s.idx)] : nullptr;
    }
};

// Speculative candidates of the last fqz5_sections_try on this thread; they
// live in the thread's GPU arenas until fqz5_sections_commit.
struct TrySession {
    Candidates c;
    std::vector<uint32_t> upper;                  // the sizes matrix with upper bounds
    bool open = false;
    bool aux = false;                             // candidates live in the helper contexts
    std::vector<int> predicted;                   // staged try: a follow section's provisional method (else -1)
};

// fqz_compress(4, slice, in, size, &len, m - FQZ0, NULL) for a section
// (compress_with_methods, fqzcomp5.c:2071-2092)
FqzEncReq fqz_req(const fqz5_section &S, int m, std::deque<std::vector<uint32_t>> &keep) {
    FqzEncReq r;
    r.d_in = S.in;
    r.n = S.in_size;
    r.nrec = S.nrec;
    keep.emplace_back(S.rec_len, S.rec_len + std::max(S.nrec, 0));
    r.lens = keep.back().data();
    if (S.rec_flags)
        keep.emplace_back(S.rec_flags, S.rec_flags + std::max(S.nrec, 0));
    else
        keep.emplace_back(size_t(std::max(S.nrec, 0)), 0u);
    r.flags = keep.back().data();
    r.d_seq = S.seq;
    r.vers = 4;
    r.strat = m - FQZ0;
    return r;
}
thread_local TrySession t_sess;

// Name-section candidates (encode_names, fqzcomp5.c:1408-1586) of sections
// `which` x methods `meth`, on context g: the names come down once per
// section, are split / tokenised on host threads, and every lzp pass and
// rANS stream of all candidates runs as one batch each.
void encode_name_jobs(GpuCtx &g, const fqz5_section *secs, const std::vector<int> &which,
                      const std::vector<int> &meth, std::vector<NameEnc> &out) {
    out.assign(which.size(), NameEnc());
    if (which.empty()) return;
    // into the pinned staging arena (kept until the context's reset): a
    // pageable copy of a -5 run's 38 name blocks (570 MB) took ~0.5 s
    // Each block's tokenising starts when its own download is done (an
    // event per block), not after all of them.
    std::vector<const uint8_t *> host;
    std::vector<hipEvent_t> evs;
    std::vector<int> host_of(which.size());
    std::vector<int> seen;
    struct Events {
        std::vector<hipEvent_t> &e;
        ~Events() { for (auto x : e) (void)hipEventDestroy(x); }
    } keep_{evs};
    for (size_t k = 0; k < which.size(); k++) {
        auto it = std::find(seen.begin(), seen.end(), which[k]);
        if (it != seen.end()) { host_of[k] = int(it - seen.begin()); continue; }
        host_of[k] = int(seen.size());
        seen.push_back(which[k]);
        const fqz5_section &S = secs[which[k]];
        uint8_t *hb = g.staging.alloc(S.in_size + 1);
        g.download(hb, S.in, S.in_size);
        hipEvent_t e;
        FQZ5_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        evs.push_back(e);
        FQZ5_HIP(hipEventRecord(e, g.stream));
        host.push_back(hb);
    }
    std::vector<const uint8_t *> h(which.size()), d(which.size());
    std::vector<uint32_t> lens(which.size());
    std::vector<hipEvent_t> ready(which.size());
    for (size_t k = 0; k < which.size(); k++) {
        h[k] = host[size_t(host_of[k])];
        ready[k] = evs[size_t(host_of[k])];
        d[k] = secs[which[k]].in;
        lens[k] = secs[which[k]].in_size;
    }
    names_encode_batch(g, out, h, d, lens, meth, &ready);
    g.sync();
}

// Trial pruning (fqz5_set_trial_prune): an fqz or sequence-model candidate
// whose size is provably not below the best rANS candidate's, in every trial
// section and summed over the trial window, cannot be chosen (rANS methods
// come first, so they win ties); its range chain and bytes are skipped and
// its lower bound stands in for its size.  The caller enables it only when
// the sections of this call that try such methods form one whole trial
// window per section kind.
std::atomic<int> g_prune{0};
// Bounds-only tries (fqz5_set_trial_bounds): every fqz and sequence-model
// candidate skips its range chain and reports its size as the interval
// [lower, upper] (entropy, entropy plus the coder's slack): the caller
// decides the trial from the intervals when they separate the candidates,
// and codes the winners at commit (encode_run_bounded).
std::atomic<int> g_bounds{0};
std::atomic<uint64_t> g_fqz_tried{0}, g_fqz_pruned{0};
// Staged tries (fqz5_set_staged_try, $FQZ5_STAGED_TRY; -1 = not read yet)
std::atomic<int> g_staged{-1};
std::atomic<uint64_t> g_staged_n[4];               // fqz5_staged_counts
std::atomic<uint64_t> g_staged_dec[FQZ5_SEC_LAST]; // fqz5_staged_decisions
bool staged_on() {
    int v = g_staged.load();
    if (v < 0) {
        const char *e = std::getenv("FQZ5_STAGED_TRY");
        v = !(e && e[0] == '0');
        int want = -1;
        if (!g_staged.compare_exchange_strong(want, v)) v = want;
    }
    return v != 0;
}
std::atomic<uint64_t> g_chains_host{0}, g_chains_gpu{0};   // fqz5_decode_chain_counts

// Which candidates of one family of work candidates (fam: fqz methods
// FQZ0..FQZ4 on quality sections, or the sequence models SEQ10..SEQ14B) to
// skip, from the exact sizes of the earlier (rANS) methods and the family's
// lower bounds: sets bounds[k].skip.  lb(k): candidate k's size lower bound
// (0 if unknown).
template <class LB>
void prune_plan(const Candidates &C, int fam, int mlo, int mhi, std::vector<Bound> &bounds, LB lb) {
    std::vector<int> F;                                 // sections trying the family
    for (int i = 0; i < C.nsec; i++)
        for (int m = mlo; m <= mhi; m++)
            if (C.find(i, m, fam) >= 0) { F.push_back(i); break; }
    // one whole trial window: every method's usize is then the same, and the
    // window's pick (min (csize + 1) / usize) compares plain sums
    if (F.size() != size_t(FQZ5_METRICS_TRIAL)) return;
    auto rsize = [&](int i, int m) -> int64_t {          // exact rANS size, -1 if none
        const Layout *l = C.find(i, m, FAM_RANS) >= 0 ? C.layout(i, m) : nullptr;
        return l ? int64_t(layout_size(*l)) : -1;
    };
    std::vector<int64_t> best(F.size(), -1);            // per section: min earlier size
    for (size_t k = 0; k < F.size(); k++)
        for (int m = 1; m < mlo; m++) {
            const int64_t z = rsize(F[k], m);
            if (z >= 0 && (best[k] < 0 || z < best[k])) best[k] = z;
        }
    int64_t best_sum = -1;                              // min over methods tried everywhere
    for (int m = 1; m < mlo; m++) {
        int64_t sum = 0;
        bool all = true;
        for (int i : F) {
            const int64_t z = rsize(i, m);
            if (z < 0) { all = false; break; }
            sum += z;
        }
        if (all && (best_sum < 0 || sum < best_sum)) best_sum = sum;
    }
    for (int m = mlo; m <= mhi; m++) {
        bool ok = true;
        int64_t lbsum = 0;
        for (size_t k = 0; k < F.size() && ok; k++) {
            const int fi = C.find(F[k], m, fam);
            if (fi < 0) { ok = false; break; }            // must be tried in the whole window
            const int64_t b = int64_t(lb(size_t(fi)));
            ok = b > 0 && best[k] >= 0 && b >= best[k];
            lbsum += b;
        }
        if (!ok || !(best_sum >= 0 && lbsum >= best_sum)) continue;
        for (int i : F)
            if (C.find(i, m, fam) >= 0) bounds[size_t(C.find(i, m, fam))].skip = true;
    }
}

// Adds the candidates of masks[i] for every section: the one place that maps
// a method to its coder family.  A method that does not fit its section adds
// nothing (fqz5_sections_try refuses such masks first; fqz5_sections_commit
// leaves the section without bytes).  The stripe and LZP3 candidates get
// their place in the table when they join the batch.
void collect(Candidates &C, const fqz5_section *secs, const uint32_t *masks) {
    for (int i = 0; i < C.nsec; i++) {
        const fqz5_section &S = secs[i];
        for (int m = 1; m < FQZ5_M_LAST; m++) {
            if (!(masks[i] & (1u << m))) continue;
            if (is_name_method(m) != (S.sec == FQZ5_SEC_NAME)) continue;
            if (is_name_method(m)) {
                C.at(i, m) = {FAM_NAME, int(C.name_sec.size())};
                C.name_sec.push_back(i);
                C.name_meth.push_back(m);
            } else if (is_fqz(m)) {
                if (S.sec != FQZ5_SEC_QUAL || !S.rec_len) continue;
                C.at(i, m) = {FAM_FQZ, int(C.fqz.size())};
                C.fqz.push_back(fqz_req(S, m, C.recs));
                C.fqz_b.emplace_back();
            } else if (is_seqcm(m)) {
                if (S.sec != FQZ5_SEC_SEQ || !S.rec_len) continue;
                C.at(i, m) = {FAM_SEQ, int(C.seq.size())};
                C.seq.push_back(seq_req(S, m));
                C.seq_b.emplace_back();
            } else if (m == LZP3) {                            // after the lzp pass
                C.lzp_sec.push_back(i);
            } else if (m == RANSXN1) {                         // thousands of short stripe chains
                if (!S.fixed_len) continue;                    // out = NULL (:2004-2007)
                C.stripe_sec.push_back(i);
                C.stripes.push_back(rans_req(S, m));
            } else if (RANS_MASK & (1u << m)) {
                C.put_rans(i, m, rans_req(S, m));
            }
        }
    }
}

// The LZP3 candidates of sections `which` (fqzcomp5.c:2013-2021): the lzp pass
// on context g; its output (device, g's arena) as one order-5 rANS request
// each.
std::vector<CompressReq> lzp_reqs(GpuCtx &g, const fqz5_section *secs, const std::vector<int> &which) {
    std::vector<CompressReq> out(which.size());
    if (which.empty()) return out;
    std::vector<LzpEncReq> lz(which.size());
    for (size_t k = 0; k < which.size(); k++) {
        lz[k].d_in = secs[which[k]].in;
        lz[k].n = secs[which[k]].in_size;
    }
    lzp_encode_batch(g, lz);
    for (size_t k = 0; k < which.size(); k++) {
        CompressReq &r = out[k];
        r.d_in = lz[k].d_out;
        r.n = lz[k].out_len;
        r.order = 5;
        r.cap = compress_bound(r.n, r.order);
    }
    return out;
}

// fn() on a thread of its own for context c (an empty fn: none).  The caller
// takes c: gpu_aux() gives the calling thread's contexts.  A new thread
// starts on device 0, and c's arena may grow (hipMalloc on the current
// device), so c's device comes first.  Joined by join() or by leaving the
// scope, so before any reset() of c.
host::Task on_ctx(GpuCtx &c, const char *who, double t0, std::function<void()> fn) {
    if (!fn) return host::Task();
    return host::Task([&c, who, t0, fn = std::move(fn)] {
        FQZ5_HIP(hipSetDevice(c.device));
        fn();
        if (step_trace())
            std::fprintf(stderr, "%s: helper context %p done at %.1f ms\n", who,
                         static_cast<void *>(&c), now_ms() - t0);
    });
}

// Requests dealt round-robin into ng groups (one helper context each), and
// their work back in request order.
template <class R>
std::vector<std::vector<R>> deal(std::vector<R> &v, size_t ng) {
    std::vector<std::vector<R>> grp(ng);
    for (size_t k = 0; k < v.size(); k++) grp[k % ng].push_back(std::move(v[k]));
    return grp;
}
template <class R>
void deal_back(std::vector<R> &v, std::vector<std::vector<R>> &grp) {
    for (size_t k = 0; k < v.size(); k++) v[k] = std::move(grp[k % grp.size()][k / grp.size()]);
}

// A batch of rANS requests on g.  With a plain_ctx, the plain O0/O1 requests
// (RANS0/RANS1: the longest chains, one step per 4 input bytes) of 2^20 B and
// more need no PACK / RLE pass: they run as a batch of their own on that
// helper context, so that their chains start while this thread packs and
// run-length codes the others' inputs (the packed chains are half as long or
// less); unless the batch holds one kind only.
void rans_batch(GpuCtx &g, GpuCtx *plain_ctx, std::vector<CompressReq> &reqs, const char *who,
                double t0) {
    if (reqs.empty()) return;
    std::vector<char> is_plain(reqs.size(), 0);
    size_t np = 0;
    for (size_t k = 0; k < reqs.size(); k++)
        np += is_plain[k] = plain_ctx && (reqs[k].order & ~1) == 0 && reqs[k].n >= (1u << 20);
    if (np == 0 || np == reqs.size()) {
        compress_batch(g, reqs);
        return;
    }
    std::vector<CompressReq> plain, rest;
    for (size_t k = 0; k < reqs.size(); k++) (is_plain[k] ? plain : rest).push_back(std::move(reqs[k]));
    plain_ctx->prof.on = g.prof.on;
    host::Task tp = on_ctx(*plain_ctx, who, t0, [&] { compress_batch(*plain_ctx, plain); });
    compress_batch(g, rest);
    const double tc = step_trace() ? now_ms() : 0;
    tp.join();
    if (step_trace())
        std::fprintf(stderr, "%s: %zu plain rANS candidates on a helper, done %.1f ms after the "
                     "others\n", who, plain.size(), now_ms() - tc);
    size_t qp = 0, qr = 0;                               // back in request order
    for (size_t k = 0; k < reqs.size(); k++) reqs[k] = std::move(is_plain[k] ? plain[qp++] : rest[qr++]);
    g.prof.enc_ms += plain_ctx->prof.enc_ms;
    g.prof.enc_launches += plain_ctx->prof.enc_launches;
    g.prof.enc_bytes += plain_ctx->prof.enc_bytes;
    plain_ctx->prof = KernelProfile();
}

// What fqz5_sections_try adds to run_candidates.
struct RunHooks {
    // the second stage of a staged try: once every rANS batch (the stripes'
    // too) has sizes, while the other helpers are still at work; plain_ctx as
    // for rans_batch
    std::function<void(GpuCtx *plain_ctx)> after_rans;
    // trial pruning / a bounds-only try: sets Bound::skip of the fqz and
    // sequence-model candidates, after their model passes, before their chains
    std::function<void()> before_chains;
};

// Codes every candidate of C.  spread (fqz5_sections_try, when a candidate
// wants a helper): the candidates whose cost grows with their work (trial
// blocks only) run on the thread's helper contexts from helper threads,
// beside the rANS candidates on g (a few long chains that leave most of the
// GPU idle): LZP3 (the lzp pass, then rANS order 5 of its output), the fqz
// and the sequence-model model passes, the stripes, the names.  Then
// hk.before_chains marks the fqz / sequence-model candidates to skip, and the
// others' range chains run.  Otherwise (fqz5_sections_commit's late encodes,
// a try of rANS candidates only) everything runs on g but the fqz candidates.
// Returns whether helper contexts hold bytes of C now.
bool run_candidates(Candidates &C, const fqz5_section *secs, GpuCtx &g, bool spread,
                    const RunHooks &hk, const char *who, double t0) {
    // fn(context k) on a thread of its own, if `need`
    auto helper = [&](int k, bool need, auto fn) {
        if (!need) return host::Task();
        GpuCtx &c = gpu_aux(k);
        return on_ctx(c, who, t0, [&c, fn] { fn(c); });
    };
    if (!spread || !C.wants_helpers()) {
        // The late fqz encodes (-5 Illumina: every block's quality section;
        // their range chains, ~1.2 s for a 100 MB block, are the commit's
        // long pole) start first, in groups on the helper contexts (the
        // sequence models' ones, idle now), so that each group's chains start
        // when its own model pass is done, and the other late encodes run
        // beside them on this thread.
        std::vector<std::vector<FqzEncReq>> fgrp = deal(C.fqz, std::min(C.fqz.size(), size_t(AUX_NSEQ)));
        std::vector<host::Task> tf;
        for (size_t q = 0; q < fgrp.size(); q++)
            tf.push_back(helper(int(AUX_SEQ0 + q), true,
                                [&grp = fgrp[q]](GpuCtx &c) { fqz_encode_batch(c, grp); }));
        C.join_lzp(lzp_reqs(g, secs, C.lzp_sec));
        C.join_stripes();
        rans_batch(g, nullptr, C.rans, who, t0);
        if (hk.after_rans) hk.after_rans(nullptr);
        if (!C.seq.empty()) seq_encode_batch(g, C.seq);
        encode_name_jobs(g, secs, C.name_sec, C.name_meth, C.names);
        for (host::Task &t : tf) t.join();
        if (!fgrp.empty()) deal_back(C.fqz, fgrp);
        return !fgrp.empty();
    }
    // sequence-model candidates: one helper context each (their passes are
    // latency-bound and overlap well), up to AUX_NSEQ (each runs one block at
    // a time with ~120 B of device memory per base while it prepares: as many
    // side by side as fit a quarter of HBM; -9's 1 GB blocks take them one
    // after another)
    size_t nsq = std::min<size_t>(C.seq.size(), size_t(AUX_NSEQ));
    if (nsq) {
        uint64_t mx = 1;
        for (const SeqEncReq &q : C.seq) mx = std::max<uint64_t>(mx, q.n);
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess || !tot) tot = size_t(64) << 30;
        const uint64_t fit = (uint64_t(tot) / 4) / (120 * mx);
        nsq = std::max<size_t>(1, std::min<size_t>(nsq, size_t(fit)));
    }
    std::vector<std::vector<SeqEncReq>> sqg = deal(C.seq, nsq);
    std::vector<CompressReq> lzr;
    std::vector<char> skip_f(C.fqz.size(), 0), skip_s(C.seq.size(), 0);
    GpuCtx &gp = gpu_aux(AUX_PLAIN);
    host::Task t_lzp = helper(AUX_LZP, !C.lzp_sec.empty(), [&](GpuCtx &c) {
        lzr = lzp_reqs(c, secs, C.lzp_sec);
        compress_batch(c, lzr);
    });
    host::Task t_fqz = helper(AUX_FQZ, !C.fqz.empty(), [&](GpuCtx &c) { fqz_encode_prepare(c, C.fqz); });
    // The RANSXN1 candidates (150 stripes x 4 orders per quality section:
    // most of a batch's jobs, and most of its host work on tables) run as
    // their own batch on a helper context, so that their host work overlaps
    // the long chains of the other rANS candidates on the GPU.
    host::Task t_stripes = helper(AUX_STRIPES, !C.stripes.empty(),
                                  [&](GpuCtx &c) { compress_batch(c, C.stripes); });
    // the name candidates: host tokenising, then their own batches
    host::Task t_names = helper(AUX_NAMES, !C.name_sec.empty(), [&](GpuCtx &c) {
        encode_name_jobs(c, secs, C.name_sec, C.name_meth, C.names);
    });
    std::vector<host::Task> t_seq;
    for (size_t k = 0; k < nsq; k++)
        t_seq.push_back(helper(int(AUX_SEQ0 + k), true,
                               [&grp = sqg[k]](GpuCtx &c) { seq_encode_prepare(c, grp); }));
    rans_batch(g, &gp, C.rans, who, t0);
    // the three rANS batches first (the stripes' too): their sizes decide the
    // second stage, which runs beside the other helpers
    t_stripes.join();
    C.join_stripes();
    if (hk.after_rans) hk.after_rans(&gp);
    const double tc = step_trace() ? now_ms() : 0;
    t_lzp.join();
    t_fqz.join();
    for (host::Task &t : t_seq) t.join();
    t_names.join();
    if (step_trace())
        std::fprintf(stderr, "%s: rANS candidates %.1f ms, helpers waited %.1f ms more\n", who,
                     tc - t0, now_ms() - tc);
    if (nsq) deal_back(C.seq, sqg);
    C.join_lzp(std::move(lzr));
    if (hk.before_chains) hk.before_chains();
    for (size_t k = 0; k < C.fqz.size(); k++) skip_f[k] = C.fqz_b[k].skip;
    for (size_t k = 0; k < C.seq.size(); k++) skip_s[k] = C.seq_b[k].skip;
    // the fqz chains on their helper beside the sequence models' on this thread
    host::Task t_chains = helper(AUX_FQZ, !C.fqz.empty(),
                                 [&](GpuCtx &c) { fqz_encode_finish(c, C.fqz, &skip_f); });
    if (!C.seq.empty()) {
        GpuCtx &gb = gpu_aux(AUX_SEQ0);
        FQZ5_HIP(hipSetDevice(gb.device));
        seq_encode_finish(gb, C.seq, &skip_s);
    }
    t_chains.join();
    for (size_t k = 0; k < C.fqz.size(); k++)
        if (skip_f[k]) {
            C.fqz_b[k].lb = fqz_size_lower_bound(C.fqz[k]);
            C.fqz_b[k].ub = fqz_size_upper_bound(C.fqz[k]);
        }
    for (size_t k = 0; k < C.seq.size(); k++)
        if (skip_s[k]) {
            C.seq_b[k].lb = seq_size_lower_bound(C.seq[k]);
            C.seq_b[k].ub = seq_size_upper_bound(C.seq[k]);
        }
    return true;
}

}  // namespace fqz5

using namespace fqz5;

extern "C" {

void fqz5_trial_init(fqz5_trial_state *st) { std::memset(st, 0, sizeof *st); }

int fqz5_set_trial_prune(int on) { return g_prune.exchange(on ? 1 : 0); }

int fqz5_set_trial_bounds(int on) { return g_bounds.exchange(on ? 1 : 0); }

int fqz5_arenas_release(void) {
    try {
        t_sess = TrySession();
        gpu_release_all();
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        return -1;
    }
}

int fqz5_sections_try_upper(uint32_t *upper, int nsec) {
    if (nsec < 0 || size_t(nsec) * FQZ5_M_LAST != t_sess.upper.size()) {
        fqz5_set_error("fqz5_sections_try_upper: no try of that many sections on this thread");
        return -1;
    }
    std::memcpy(upper, t_sess.upper.data(), t_sess.upper.size() * sizeof(uint32_t));
    return 0;
}

void fqz5_decode_chain_counts(uint64_t *out2) {
    out2[0] = g_chains_host.load();
    out2[1] = g_chains_gpu.load();
}

void fqz5_rans_chain_counts(uint64_t *out2) { rans_chain_counts(out2); }
void fqz5_rans_enc_chain_counts(uint64_t *out2) { rans_enc_chain_counts(out2); }

void fqz5_rans_variant_counts(uint64_t *dec, uint64_t *dec_hedged, uint64_t *enc, int *ndec,
                              int *nenc) {
    rans_variant_counts(dec, dec_hedged, enc, ndec, nenc);
}
const char *fqz5_rans_variant_name(int dir, int i) { return rans_variant_name(dir, i); }

int fqz5_seq_path_counts(uint64_t *out, int n) { return seq_path_counts(out, n); }

void fqz5_trial_counts(uint64_t *out2) {
    out2[0] = g_fqz_tried.load();
    out2[1] = g_fqz_pruned.load();
}

void fqz5_trial_schedule(const int32_t *sec_ids, int nsec, const uint32_t *avail,
                         const fqz5_trial_state *st, uint32_t *masks_out) {
    fqz5_trial_state s = *st;
    for (int i = 0; i < nsec; i++)
        masks_out[i] = trial_step(s.sec[sec_ids[i]]) == STEP_TRIAL ? avail[sec_ids[i]] : 0;
}

void fqz5_staged_plan(const int32_t *sec_ids, int nsec, const uint32_t *avail,
                      const fqz5_trial_state *st, int32_t *roles_out, uint32_t *masks_out,
                      int32_t *window_out) {
    staged_walk(sec_ids, nsec, avail, st, roles_out, masks_out, window_out, nullptr);
}

int fqz5_set_staged_try(int on) {
    const int prev = staged_on();
    g_staged.store(on ? 1 : 0);
    return prev;
}

void fqz5_staged_counts(uint64_t out[4]) {
    for (int k = 0; k < 4; k++) out[k] = g_staged_n[k].load();
}

void fqz5_staged_decisions(uint64_t out[FQZ5_SEC_LAST]) {
    for (int k = 0; k < FQZ5_SEC_LAST; k++) out[k] = g_staged_dec[k].load();
}

}  // extern "C"

// fqz5_sections_try, and with `avail` and `st` (and staged tries on)
// fqz5_sections_try_staged: the sequence and quality sections outside a trial
// window code one method, the trial's pick.  A section whose pick is in the
// state (settled) codes it beside the trial sections; a section whose trial
// window lies in this call (follow) waits until the window's rANS candidates
// have sizes, and is then coded with the pick over those sizes, while the
// other helpers are still at work.  The pick is provisional: the replay
// decides, and the commit codes late whatever the session lacks.
static int sections_try_impl(const fqz5_section *secs, int nsec, const uint32_t *masks_in,
                             uint32_t *sizes, const uint32_t *avail,
                             const fqz5_trial_state *st) {
    const double t0 = step_trace() ? now_ms() : 0;
    try {
        GpuCtx &g = gpu();
        if (t_sess.open) {
            g.reset();
            gpu_aux_reset_all();
        }
        t_sess = TrySession();
        t_sess.predicted.assign(size_t(std::max(nsec, 0)), -1);
        // the first stage's masks: a settled section keeps its one method, a
        // follow section none
        std::vector<uint32_t> stage1(masks_in, masks_in + std::max(nsec, 0));
        std::vector<Decision> decs;
        const bool staged = avail && st && staged_on() && nsec > 0;
        if (staged) {
            std::vector<int32_t> ids(nsec), roles(nsec), win(nsec);
            std::vector<uint32_t> pm(nsec);
            for (int i = 0; i < nsec; i++) ids[i] = secs[i].sec;
            staged_walk(ids.data(), nsec, avail, st, roles.data(), pm.data(), win.data(), &decs);
            uint64_t skipped = 0;
            for (int i = 0; i < nsec; i++) {
                if (roles[i] == FQZ5_ROLE_SETTLED) stage1[i] &= pm[i];
                if (roles[i] == FQZ5_ROLE_FOLLOW) stage1[i] = 0;
                uint32_t gone = masks_in[i] & ~stage1[i];
                if (!secs[i].fixed_len) gone &= ~(1u << RANSXN1);
                skipped += uint64_t(__builtin_popcount(gone));
            }
            g_staged_n[3] += skipped;        // (a follow section's coded pick comes off below)
        }
        const uint32_t *masks = stage1.data();
        for (int i = 0; i < nsec; i++) {
            if (masks[i] & ~(RANS_MASK | FQZ_MASK | SEQ_MASK | NAME_MASK | (1u << LZP3)))
                throw GpuError("fqz5_sections_try: method mask has SEQ_CUSTOM (not in this build)");
            if ((masks[i] & NAME_MASK) && secs[i].sec != FQZ5_SEC_NAME)
                throw GpuError("fqz5_sections_try: name methods need a name section");
            if (secs[i].sec == FQZ5_SEC_NAME && (masks[i] & ~NAME_MASK))
                throw GpuError("fqz5_sections_try: a name section takes name methods only");
            if ((masks[i] & SEQ_MASK) && (secs[i].sec != FQZ5_SEC_SEQ || !secs[i].rec_len))
                throw GpuError("fqz5_sections_try: SEQ methods need a sequence section with records");
            if ((masks[i] & FQZ_MASK) && (secs[i].sec != FQZ5_SEC_QUAL || !secs[i].rec_len))
                throw GpuError("fqz5_sections_try: FQZ methods need a quality section with records");
        }
        // (t_sess is thread_local: the helper threads get the caller's
        // candidates by reference)
        Candidates &C = t_sess.c = Candidates(nsec);
        collect(C, secs, masks);
        if (staged)
            g_staged_n[0] += C.rans.size() + C.stripes.size() + C.lzp_sec.size() + C.fqz.size() + C.seq.size();
        RunHooks hk;
        // The second stage: each decision's pick over the sizes its window's
        // rANS candidates have now (the first smallest (csize + 1) / usize,
        // as metrics_method picks), and the follow sections coded with it; the
        // plain chains on `plain_ctx` beside the others when there is one.
        if (staged) hk.after_rans = [&](GpuCtx *plain_ctx) {
            std::vector<uint32_t> pick(size_t(nsec), 0);     // the follow sections' one-bit masks
            for (const Decision &d : decs) {
                fqz5_section_stats s = st->sec[d.kind];
                if (d.fresh) {
                    std::memset(s.usize, 0, sizeof s.usize);
                    std::memset(s.csize, 0, sizeof s.csize);
                }
                if (d.follow.empty()) continue;     // nothing in the call takes its pick
                for (int i : d.rows)
                    for (int m = 1; m < FQZ5_M_LAST; m++) {
                        if (!(masks_in[i] & RANS_MASK & (1u << m))) continue;
                        s.usize[m] += secs[i].in_size;
                        s.csize[m] += C.size(i, m);
                    }
                const int w = pick_method(s, RANS_MASK);
                g_staged_dec[d.kind]++;
                if (step_trace())
                    std::fprintf(stderr, "sections_try: staged: kind %d decided at %.1f ms: method %d "
                                 "for %zu sections\n", d.kind, now_ms() - t0, w, d.follow.size());
                if (!w) continue;
                for (int i : d.follow) pick[size_t(i)] = masks_in[i] & (1u << w);
            }
            Candidates s2(nsec);
            collect(s2, secs, pick.data());
            s2.join_stripes();
            if (s2.rans.empty()) return;
            rans_batch(g, plain_ctx, s2.rans, "sections_try", t0);
            const size_t n2 = s2.rans.size();
            for (int i = 0; i < nsec; i++) {
                const int m = pick[size_t(i)] ? __builtin_ctz(pick[size_t(i)]) : 0;
                const int k = s2.find(i, m, FAM_RANS);
                if (k < 0) continue;
                C.put_rans(i, m, std::move(s2.rans[size_t(k)]));
                t_sess.predicted[size_t(i)] = m;
            }
            g_staged_n[1] += n2;
            g_staged_n[3] -= n2;
            if (step_trace())
                std::fprintf(stderr, "sections_try: staged: stage 2 (%zu sections) done at %.1f ms\n",
                             n2, now_ms() - t0);
        };
        hk.before_chains = [&C] {
            if (g_bounds.load()) {
                for (size_t k = 0; k < C.fqz.size(); k++) C.fqz_b[k].skip = fqz_size_lower_bound(C.fqz[k]) > 0;
                for (size_t k = 0; k < C.seq.size(); k++) C.seq_b[k].skip = seq_size_upper_bound(C.seq[k]) > 0;
            } else if (g_prune.load()) {
                prune_plan(C, FAM_FQZ, FQZ0, FQZ4, C.fqz_b,
                           [&](size_t k) { return fqz_size_lower_bound(C.fqz[k]); });
                prune_plan(C, FAM_SEQ, SEQ10, SEQ14B, C.seq_b,
                           [&](size_t k) { return seq_size_lower_bound(C.seq[k]); });
            }
        };
        t_sess.aux = run_candidates(C, secs, g, true, hk, "sections_try", t0);
        g_fqz_tried += C.fqz.size() + C.seq.size();
        for (const Bound &b : C.fqz_b) g_fqz_pruned += b.skip ? 1 : 0;
        for (const Bound &b : C.seq_b) g_fqz_pruned += b.skip ? 1 : 0;
        t_sess.open = true;
        if (step_trace())
            std::fprintf(stderr, "sections_try: %.1f ms (device / pinned allocations so far %llu, "
                         "frees %llu)\n", now_ms() - t0,
                         (unsigned long long)ChunkPool::alloc_calls().load(),
                         (unsigned long long)ChunkPool::free_calls().load());
        // a skipped candidate's lower bound in `sizes`, its upper bound in `upper`
        t_sess.upper.assign(size_t(nsec) * FQZ5_M_LAST, 0);
        for (int i = 0; i < nsec; i++) {
            uint32_t stale = UINT32_MAX;
            for (int m = 0; m < FQZ5_M_LAST; m++)
                sizes[size_t(i) * FQZ5_M_LAST + m] =
                    C.size(i, m, &t_sess.upper[size_t(i) * FQZ5_M_LAST + m], &stale);
        }
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        t_sess = TrySession();
        try { gpu().reset(); } catch (...) {}
        try { gpu_aux_reset_all(); } catch (...) {}
        return -1;
    }
}

extern "C" {

int fqz5_sections_try(const fqz5_section *secs, int nsec, const uint32_t *masks,
                      uint32_t *sizes) {
    return sections_try_impl(secs, nsec, masks, sizes, nullptr, nullptr);
}

int fqz5_sections_try_staged(const fqz5_section *secs, int nsec, const uint32_t *masks,
                             uint32_t *sizes, const uint32_t *avail,
                             const fqz5_trial_state *st) {
    return sections_try_impl(secs, nsec, masks, sizes, avail, st);
}

void fqz5_trial_replay(const int32_t *sec_ids, const uint32_t *in_sizes,
                       const uint32_t *sizes, int nsec, const uint32_t *avail,
                       fqz5_trial_state *st, int32_t *methods_out,
                       uint32_t *tried_out) {
    for (int i = 0; i < nsec; i++) {
        const int sec = sec_ids[i];
        fqz5_section_stats &ss = st->sec[sec];
        const uint32_t methods = metrics_method(*st, sec, avail[sec]);
        const bool in_trial = ss.trial > 0;           // compress_with_methods
        uint32_t best_sz = UINT32_MAX;
        int best_m = 0;
        for (int m = 0; m < FQZ5_M_LAST; m++) {
            if (!(methods & (1u << m))) continue;
            const uint32_t out_len = sizes[size_t(i) * FQZ5_M_LAST + m];
            if (best_sz > out_len) { best_sz = out_len; best_m = m; }
        }
        // outside the trial the one method is run whatever its size (the
        // caller encodes it at commit: its size is not known here)
        if (!in_trial && __builtin_popcount(methods) == 1) best_m = __builtin_ctz(methods);
        if (in_trial) {                                 // metrics_update, :2121-2130
            for (int m = 0; m < FQZ5_M_LAST; m++) {
                if (!(methods & (1u << m)) || ss.trial <= 0) continue;
                ss.usize[m] += in_sizes[i];
                ss.csize[m] += sizes[size_t(i) * FQZ5_M_LAST + m];
                ss.count[m]++;
            }
            ss.trial--;
        }
        methods_out[i] = best_m;
        if (tried_out) tried_out[i] = methods;
    }
}

int fqz5_sections_commit(const fqz5_section *secs, int nsec, const int32_t *methods,
                         fqz5_section_result *res) {
    const double t0 = step_trace() ? now_ms() : 0;
    try {
        GpuCtx &g = gpu();
        if (!t_sess.open || t_sess.c.nsec != nsec)
            throw GpuError("fqz5_sections_commit: no matching fqz5_sections_try");
        const Candidates &C = t_sess.c;
        for (int i = 0; i < nsec; i++)                // a staged try's picks the replay overturned
            if (size_t(i) < t_sess.predicted.size() && t_sess.predicted[size_t(i)] >= 0 &&
                t_sess.predicted[size_t(i)] != methods[i])
                g_staged_n[2]++;
        // The late set: sections outside the trial, their one method encoded
        // now.  A candidate the session tried with its range chain skipped (a
        // bounds-only try or a pruned one) has no bytes: coded now, as a
        // method the session did not try.  A method that does not fit its
        // section is left out (status -1 below), LZP3 on anything but a
        // sequence section included (fqz5_decode_sections reads it only there).
        std::vector<uint32_t> late_mask(size_t(std::max(nsec, 0)), 0);
        for (int i = 0; i < nsec; i++) {
            const int m = methods[i];
            if (m <= 0 || m >= FQZ5_M_LAST || C.coded(i, m)) continue;
            if (m == LZP3 && secs[i].sec != FQZ5_SEC_SEQ) continue;
            late_mask[size_t(i)] = 1u << m;
        }
        Candidates late(nsec);
        collect(late, secs, late_mask.data());
        const bool late_aux = run_candidates(late, secs, g, false, RunHooks(), "sections_commit", t0);
        std::vector<const Layout *> ls;
        std::vector<uint8_t *> dsts;
        std::vector<Layout> framed(nsec);
        for (int i = 0; i < nsec; i++) {
            const fqz5_section &S = secs[i];
            fqz5_section_result &R = res[i];
            const int m = methods[i];
            // the session's bytes, else the late set's
            if (S.sec == FQZ5_SEC_NAME) {             // encode_names' bytes, unframed
                const NameEnc *E = C.name(i, m) ? C.name(i, m) : late.name(i, m);
                R.method = m;
                R.strat = is_name_method(m) ? name_strat(m) : 0;
                R.status = -1;
                R.clen = 0;
                R.usize = S.in_size;
                if (!E || !E->ok) continue;
                R.clen = uint32_t(E->out.size());
                if (E->out.size() > S.out_cap) continue;
                Piece p;
                p.host = E->out;
                framed[i].push_back(std::move(p));
                ls.push_back(&framed[i]);
                dsts.push_back(S.out);
                R.status = 0;
                continue;
            }
            const Layout *lay = C.layout(i, m) ? C.layout(i, m) : late.layout(i, m);
            R.method = m;
            // compress_with_methods' *strat (fqzcomp5.c:1994-2069)
            R.strat = is_fqz(m) ? 1 : is_seqcm(m) ? seq_strat(m) : m == LZP3 ? LZP3 : 0;
            R.status = -1;
            R.clen = 0;
            R.usize = S.in_size;
            if (!lay) continue;
            const uint32_t clen = layout_size(*lay);
            R.clen = clen;
            if (9ull + clen > S.out_cap) continue;
            // section framing [strat u8][u32 usize][u32 csize] (:2224-2229)
            Piece h;
            h.host.resize(9);
            h.host[0] = uint8_t(R.strat);
            std::memcpy(&h.host[1], &S.in_size, 4);
            std::memcpy(&h.host[5], &clen, 4);
            framed[i].push_back(std::move(h));
            for (auto &p : *lay) framed[i].push_back(p);
            ls.push_back(&framed[i]);
            dsts.push_back(S.out);
            R.status = 0;
        }
        const double t1 = step_trace() ? now_ms() : 0;
        write_layouts_dev(g, ls, dsts);
        const double t2 = step_trace() ? now_ms() : 0;
        g.reset();
        const double t3 = step_trace() ? now_ms() : 0;
        // the fqz candidates of the try live in the aux arena: rewind it too,
        // or every step's trial buffers take fresh chunks (the r01 bench OOM)
        if (t_sess.aux || late_aux) gpu_aux_reset_all();
        // the session's host buffers (candidate tables, layouts, the name
        // candidates' token streams: ~100 MB, mostly munmap) are freed by a
        // detached thread, off the caller's path; nothing refers to them now
        std::thread([old = std::make_unique<TrySession>(std::move(t_sess))]() mutable {
            old.reset();
        }).detach();
        t_sess = TrySession();
        if (step_trace())
            std::fprintf(stderr, "sections_commit: late encodes %.1f ms, write %.1f ms, sync "
                         "%.1f ms, release %.1f ms\n", t1 - t0, t2 - t1, t3 - t2, now_ms() - t3);
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        t_sess = TrySession();
        try { gpu().reset(); } catch (...) {}
        try { gpu_aux_reset_all(); } catch (...) {}   // (the late fqz groups' and the session's arenas)
        return -1;
    }
}

int fqz5_encode_sections(const fqz5_section *secs, int nsec, const uint32_t *avail,
                         fqz5_trial_state *st, fqz5_section_result *res) {
    std::vector<uint32_t> sizes(size_t(nsec) * FQZ5_M_LAST), masks(nsec);
    std::vector<int32_t> ids(nsec), meth(nsec);
    std::vector<uint32_t> ins(nsec);
    for (int i = 0; i < nsec; i++) { ids[i] = secs[i].sec; ins[i] = secs[i].in_size; }
    // every method of every trial section in one launch, the trial's pick
    // for the others (see sections.encode_run)
    for (int i = 0; i < nsec; i++) masks[i] = avail[secs[i].sec];
    if (fqz5_sections_try_staged(secs, nsec, masks.data(), sizes.data(), avail, st)) return -1;
    fqz5_trial_replay(ids.data(), ins.data(), sizes.data(), nsec, avail, st, meth.data(),
                      nullptr);
    return fqz5_sections_commit(secs, nsec, meth.data(), res);
}

int fqz5_decode_sections(const fqz5_section *secs, int nsec, fqz5_section_result *res) {
    // (trace) entry to exit, the locals' destructors included
    struct ExitTrace {
        double t;
        ~ExitTrace() {
            if (t) std::fprintf(stderr, "decode_sections: entry to exit %.1f ms\n", now_ms() - t);
        }
    } exit_trace{step_trace() ? now_ms() : 0.0};
    try {
        GpuCtx &g = gpu();
        const bool trace = step_trace();
        const double t0 = now_ms();
        // section headers to the host, then the rANS payloads
        size_t tot = 0;
        for (int i = 0; i < nsec; i++) tot += secs[i].in_size;
        // into the pinned staging arena (kept until g.reset() below): a
        // pageable copy of a -5 run's 600 MB took 125 ms, this one ~5x less
        uint8_t *host = g.staging.alloc(tot + 1);
        size_t off = 0;
        for (int i = 0; i < nsec; i++) {
            g.download(host + off, secs[i].in, secs[i].in_size);
            off += secs[i].in_size;
        }
        g.sync();
        std::vector<DecompressReq> reqs;
        std::vector<FqzDecReq> fqz;
        std::vector<SeqDecReq> seqd;
        std::vector<int> who, who_fqz, who_seq;
        std::vector<LzpDecReq> lzd;
        std::vector<int> who_lzp;                     // section of each lzd entry
        std::vector<size_t> lzp_rans;                 // its rANS stage in reqs
        std::vector<NameDec> nd;                      // name sections (decode_names)
        std::vector<int> who_name;
        std::vector<const uint8_t *> seq_h;           // host stream of each seqd entry
        off = 0;
        for (int i = 0; i < nsec; i++) {
            const uint8_t *h = host + off;
            off += secs[i].in_size;
            res[i].status = -1;
            if (secs[i].in_size < 9) continue;
            if (secs[i].sec == FQZ5_SEC_NAME) {       // [u32 u_len][u8 strat][u32 c_len] (:2325-2327)
                NameDec D;
                std::memcpy(&D.u_len, h, 4);
                D.strat = h[4];
                std::memcpy(&D.c_len, h + 5, 4);
                res[i].strat = D.strat;
                res[i].clen = D.c_len;
                if (9ull + D.c_len > secs[i].in_size || D.u_len > secs[i].out_cap) continue;
                D.comp = h + 9;
                D.d_comp = secs[i].in + 9;
                nd.push_back(D);
                who_name.push_back(i);
                continue;
            }
            uint32_t ulen, clen;
            std::memcpy(&ulen, h + 1, 4);
            std::memcpy(&clen, h + 5, 4);
            res[i].strat = h[0];
            res[i].clen = clen;
            if (9ull + clen > secs[i].in_size || ulen > secs[i].out_cap) continue;
            if (h[0] == 1 && secs[i].sec == FQZ5_SEC_QUAL) {   // fqz_decompress (:2498-2530)
                FqzDecReq f;
                f.h_in = h + 9;
                f.d_in = secs[i].in + 9;
                f.in_size = clen;
                f.nrec = secs[i].rec_len ? secs[i].nrec : 0;
                f.lens = secs[i].rec_len;
                f.d_seq = secs[i].seq;
                f.d_out = secs[i].out;
                f.out_cap = secs[i].out_cap;
                fqz.push_back(f);
                who_fqz.push_back(i);
                continue;
            }
            if ((h[0] & 7) == 1 && secs[i].sec == FQZ5_SEC_SEQ) {   // decode_seq (:2421-2430)
                seq_h.push_back(h + 9);
                SeqDecReq q;
                q.d_in = secs[i].in + 9;
                q.in_size = clen;
                q.lens = secs[i].rec_len;
                q.nrec = secs[i].nrec;
                q.k = h[0] >> 4;
                q.both = (h[0] >> 3) & 1;
                q.d_out = secs[i].out;
                q.n = ulen;
                seqd.push_back(q);
                who_seq.push_back(i);
                continue;
            }
            if (h[0] == LZP3 && secs[i].sec == FQZ5_SEC_SEQ) {   // rANS, then unlzp (:2431-2445)
                const uint8_t *hs = h + 9;
                uint32_t rsz = 0;
                if (clen < 2 || (hs[0] & ORD_NOSZ) || !varint_get(hs + 1, hs + clen, &rsz)) continue;
                DecompressReq r;
                r.h_in = hs;
                r.d_in = secs[i].in + 9;
                r.in_size = clen;
                r.out_cap = rsz;
                r.d_out = g.arena.alloc_n<uint8_t>(size_t(rsz) + 1);
                LzpDecReq z;
                z.d_in = r.d_out;
                z.d_out = secs[i].out;
                z.cap = ulen;
                lzp_rans.push_back(reqs.size());
                reqs.push_back(r);
                who.push_back(-1);
                lzd.push_back(z);
                who_lzp.push_back(i);
                continue;
            }
            if (h[0] != 0) continue;
            DecompressReq r;
            r.h_in = h + 9;
            r.d_in = secs[i].in + 9;
            r.in_size = clen;
            r.out_cap = ulen;
            r.d_out = secs[i].out;
            reqs.push_back(r);
            who.push_back(i);
        }
        const double t1 = now_ms();
        // ---- where each adaptive-model chain decodes (host::place by
        // host_decode_mode(): the sequence chains, then the quality chains, of
        // any length).  A quality chain with a sequence context waits for
        // its block's bases; when those come from a host chain it runs on
        // the host too (its bases are there) ----------------------------------
        const int hmode = host_decode_mode();
        std::vector<int> fqz_kind(fqz.size(), host::CK_FQZ), fqz_src(fqz.size(), -1);
        for (size_t k = 0; k < fqz.size(); k++) {
            const FqzDecReq &f = fqz[k];
            uint32_t tl = 0;
            const int vk = varint_get(f.h_in, f.h_in + f.in_size, &tl);
            if (vk > 0 && size_t(vk) + 1 < f.in_size && (f.h_in[vk + 1] & 8u) && f.d_seq) {
                fqz_kind[k] = host::CK_FQZ_SEQ;
                for (size_t m = 0; m < seqd.size(); m++)
                    if (seqd[m].d_out == f.d_seq) fqz_src[k] = int(m);
            }
        }
        std::vector<uint64_t> chain_n;
        std::vector<int> chain_kind;
        for (const SeqDecReq &q : seqd) { chain_n.push_back(q.n); chain_kind.push_back(host::CK_SEQ); }
        for (size_t k = 0; k < fqz.size(); k++) { chain_n.push_back(fqz[k].out_cap); chain_kind.push_back(fqz_kind[k]); }
        const std::vector<char> on = host::place(hmode, chain_n, chain_kind, 0);
        std::vector<char> seq_on_host(on.begin(), on.begin() + seqd.size()),
                          fqz_on_host(on.begin() + seqd.size(), on.end());
        for (size_t k = 0; k < fqz.size(); k++)
            if (fqz_src[k] >= 0 && seq_on_host[size_t(fqz_src[k])]) fqz_on_host[k] = 1;
        g_chains_host += uint64_t(std::count(seq_on_host.begin(), seq_on_host.end(), 1) +
                                  std::count(fqz_on_host.begin(), fqz_on_host.end(), 1));
        g_chains_gpu += uint64_t(std::count(seq_on_host.begin(), seq_on_host.end(), 0) +
                                 std::count(fqz_on_host.begin(), fqz_on_host.end(), 0));
        // ---- the host chains: sequence-model sections and quality sections
        // without a sequence context start now, beside the GPU's rANS and
        // names; quality sections with one wait for their block's bases
        struct HostChain { uint8_t *buf = nullptr; size_t cap = 0, n = 0; int sec = -1; bool ok = false; };
        std::vector<HostChain> hc;
        std::vector<size_t> hc_idx;                   // seqd / fqz index of each host chain
        std::vector<int> hc_kind;                     // host::ChainKind
        for (size_t k = 0; k < seqd.size(); k++) {
            if (!seq_on_host[k]) continue;
            HostChain c;
            c.cap = c.n = seqd[k].n;
            c.buf = g.staging.alloc(c.cap + 1);
            c.sec = who_seq[k];
            hc.push_back(c);
            hc_idx.push_back(k);
            hc_kind.push_back(host::CK_SEQ);
        }
        for (size_t k = 0; k < fqz.size(); k++) {
            if (!fqz_on_host[k]) continue;
            HostChain c;
            c.cap = fqz[k].out_cap;
            c.buf = g.staging.alloc(c.cap + 1);
            c.sec = who_fqz[k];
            hc.push_back(c);
            hc_idx.push_back(k);
            hc_kind.push_back(fqz_kind[k]);
        }
        // fn() under the clock, for the cost model: a host chain of n symbols
        // that decoded, or (gpu) a GPU batch whose longest chain has n
        auto timed = [](int kind, bool gpu, uint64_t n, const std::function<bool()> &fn) {
            const double a = now_ns();
            const bool ok = fn();
            if (ok) host::measured(kind, gpu, n, now_ns() - a);
            return ok;
        };
        host::Jobs hjobs;
        std::vector<size_t> early_h;                  // host chains that start now
        for (size_t j = 0; j < hc.size(); j++)
            if (hc_kind[j] != host::CK_FQZ_SEQ) early_h.push_back(j);
        hjobs.start(early_h.size(), [&](size_t t) {
            const size_t j = early_h[t];
            HostChain &c = hc[j];
            if (hc_kind[j] == host::CK_SEQ) {
                const SeqDecReq &q = seqd[hc_idx[j]];
                c.ok = timed(host::CK_SEQ, false, q.n, [&] {
                    return host::seq_decode(seq_h[hc_idx[j]], q.in_size, q.lens, q.nrec, q.both, q.k,
                                            c.buf, q.n) == 0;
                });
            } else {
                const FqzDecReq &f = fqz[hc_idx[j]];
                c.ok = timed(host::CK_FQZ, false, c.cap, [&] {
                    return host::fqz_decode(f.h_in, f.in_size, c.buf, c.cap, &c.n, nullptr, 0, nullptr, 0) == 0;
                });
            }
        });
        // the name sections on their helper context, beside the chains: their
        // host rebuild overlaps the GPU's rANS / fqz / sequence decoding
        // The name sections decode on their helper context beside the chains.
        // Each hedged chain copy holds a CU (its LDS), so while the names run
        // they count as a second hedging caller: the chains' copies take half
        // the CUs and the names' short kernels find the rest free (their
        // host rebuild needs no CU at all).
        double t_names_up = 0;                        // (trace) the names' upload done
        GpuCtx *gn = nullptr;
        std::unique_ptr<HedgeShare> nshare;
        host::Task tn;                                // (the helpers: joined on every exit)
        if (!nd.empty()) {
            gn = &gpu_aux(AUX_NAMES);
            nshare = std::make_unique<HedgeShare>(size_t(g.cus));
            tn = on_ctx(*gn, "decode_sections", t0, [&] {
                // each block's names to their section as soon as that
                // block is rebuilt, on the names context, while the
                // chains (and the later blocks' rebuilds) still run (after
                // them, on the main stream, -5 NovaSeq's 590 MB of names
                // added ~50 ms)
                names_decode_batch(*gn, nd, [&](size_t k) {
                    if (nd[k].ok && nd[k].u_len)
                        FQZ5_HIP(hipMemcpyAsync(secs[who_name[k]].out, nd[k].names,
                                                nd[k].u_len, hipMemcpyHostToDevice, gn->stream));
                });
                gn->sync();                           // (nd's buffers are the sources)
                if (trace) t_names_up = now_ms();
            });
        }
        // GPU quality sections without a sequence context need nothing else
        // of this call: they decode on the fqz helper context from a thread
        // of their own, beside the rANS / LZP / sequence-model work, instead
        // of after it (a -5 Illumina step waited ~0.6 s for the rANS batch
        // before its 8 s fqz launch).  Those with one wait for the bases.
        std::vector<FqzDecReq> fqz_early;
        std::vector<size_t> early_of;                 // fqz index of each early request
        std::vector<char> is_early(fqz.size(), 0);
        uint64_t early_longest = 0;
        for (size_t k = 0; k < fqz.size(); k++) {
            if (fqz_on_host[k] || fqz_kind[k] == host::CK_FQZ_SEQ) continue;
            fqz_early.push_back(fqz[k]);
            early_of.push_back(k);
            is_early[k] = 1;
            early_longest = std::max<uint64_t>(early_longest, fqz[k].out_cap);
        }
        GpuCtx *gf = nullptr;
        host::Task tf;
        if (!fqz_early.empty()) {
            gf = &gpu_aux(AUX_FQZ);
            tf = on_ctx(*gf, "decode_sections", t0, [&] {
                timed(host::CK_FQZ, true, early_longest, [&] { fqz_decode_batch(*gf, fqz_early); return true; });
            });
        }
        // the GPU's sequence-model sections likewise (their own helper context)
        std::vector<SeqDecReq> seq_gpu;
        std::vector<size_t> seq_gpu_of;
        uint64_t seq_longest = 0;
        for (size_t m = 0; m < seqd.size(); m++)
            if (!seq_on_host[m]) {
                seq_gpu.push_back(seqd[m]);
                seq_gpu_of.push_back(m);
                seq_longest = std::max<uint64_t>(seq_longest, seqd[m].n);
            }
        GpuCtx *gs = nullptr;
        host::Task ts;
        if (!seq_gpu.empty()) {
            gs = &gpu_aux(AUX_SEQ0);
            ts = on_ctx(*gs, "decode_sections", t0, [&] {
                timed(host::CK_SEQ, true, seq_longest, [&] { seq_decode_batch(*gs, seq_gpu); return true; });
            });
        }
        // the rANS batch's long chains share the cores with the chains
        // started above: it gets the cores those leave idle (the late
        // quality chains run after it), so that no more than host::threads()
        // chain threads of this call run at once
        host::CoreBudget cores;
        cores.core_ns.assign(size_t(host::threads()) - std::min(size_t(host::threads()), hjobs.running()), 0.0);
        decompress_batch(g, reqs, &cores);
        const double t_rans = trace ? now_ms() : 0;
        if (trace)
            std::fprintf(stderr, "decode_sections: %zu bytes to host in %.1f ms, rANS %.1f ms\n", tot,
                         t1 - t0, now_ms() - t1);
        if (!lzd.empty()) {
            std::vector<LzpDecReq> run;
            std::vector<int> run_who;
            for (size_t k = 0; k < lzd.size(); k++) {
                const DecompressReq &r = reqs[lzp_rans[k]];
                if (!r.ok) continue;
                lzd[k].in_len = r.out_size;
                run.push_back(lzd[k]);
                run_who.push_back(who_lzp[k]);
            }
            lzp_decode_batch(g, run);
            for (size_t k = 0; k < run.size(); k++) {
                fqz5_section_result &R = res[run_who[k]];
                R.status = run[k].ok ? 0 : -1;
                R.usize = run[k].out_len;
            }
        }
        ts.join();
        for (size_t i = 0; i < seq_gpu.size(); i++) seqd[seq_gpu_of[i]] = seq_gpu[i];
        // after the rANS and sequence sections: a quality section's sequence
        // context may be the output of this call's sequence section (a GPU
        // one: host-decoded bases make their quality chain a host chain)
        {
            std::vector<FqzDecReq> late;
            std::vector<size_t> late_of;
            uint64_t longest = 0;
            for (size_t k = 0; k < fqz.size(); k++)
                if (!is_early[k] && !fqz_on_host[k]) {
                    late.push_back(fqz[k]);
                    late_of.push_back(k);
                    longest = std::max<uint64_t>(longest, fqz[k].out_cap);
                }
            if (!late.empty()) {
                timed(host::CK_FQZ_SEQ, true, longest, [&] { fqz_decode_batch(g, late); return true; });
                for (size_t k = 0; k < late.size(); k++) fqz[late_of[k]] = late[k];
            }
        }
        tf.join();
        for (size_t k = 0; k < fqz_early.size(); k++) fqz[early_of[k]] = fqz_early[k];
        if (!hc.empty()) {
            hjobs.join();
            // the quality chains with a sequence context: their block's bases
            // on the host (a host-decoded sequence section's buffer, or a copy
            // of the GPU's output), per record pointers as the reference's s->seq
            std::vector<std::vector<const uint8_t *>> recp(hc.size());
            for (size_t j = 0; j < hc.size(); j++) {
                if (hc_kind[j] != host::CK_FQZ_SEQ) continue;
                const FqzDecReq &f = fqz[hc_idx[j]];
                const uint8_t *bases = nullptr;
                bool host_src = false;
                for (size_t m = 0; m < hc.size(); m++)
                    if (hc_kind[m] == host::CK_SEQ && secs[hc[m].sec].out == f.d_seq) {
                        bases = hc[m].ok ? hc[m].buf : nullptr;
                        host_src = true;
                    }
                uint64_t nb = 0;
                for (int r = 0; r < f.nrec; r++) nb += f.lens[r];
                if (!bases) {
                    uint8_t *b = g.staging.alloc(nb + 1);
                    if (!host_src) g.download(b, f.d_seq, nb);
                    else std::memset(b, 0, nb + 1);   // (its sequence chain failed)
                    bases = b;
                }
                recp[j].resize(size_t(std::max(f.nrec, 1)));
                uint64_t o = 0;
                for (int r = 0; r < f.nrec; r++) {
                    recp[j][size_t(r)] = bases + o;
                    o += f.lens[r];
                }
            }
            g.sync();
            host::Jobs hb;
            std::vector<size_t> late;
            for (size_t j = 0; j < hc.size(); j++)
                if (hc_kind[j] == host::CK_FQZ_SEQ) late.push_back(j);
            hb.start(late.size(), [&](size_t t) {
                HostChain &c = hc[late[t]];
                const FqzDecReq &f = fqz[hc_idx[late[t]]];
                c.ok = timed(host::CK_FQZ_SEQ, false, c.cap, [&] {
                    return host::fqz_decode(f.h_in, f.in_size, c.buf, c.cap, &c.n, nullptr, 0,
                                            recp[late[t]].data(), f.nrec) == 0;
                });
            });
            hb.join();
            for (HostChain &c : hc) {
                fqz5_section_result &R = res[c.sec];
                R.status = c.ok ? 0 : -1;
                R.usize = uint32_t(c.n);
                if (c.ok && c.n)
                    FQZ5_HIP(hipMemcpyAsync(secs[c.sec].out, c.buf, c.n, hipMemcpyHostToDevice, g.stream));
            }
        }
        const double t_hc = trace ? now_ms() : 0;
        tn.join();
        nshare.reset();
        const double t_nj = trace ? now_ms() : 0;
        for (size_t k = 0; k < nd.size(); k++) {
            fqz5_section_result &R = res[who_name[k]];
            if (!nd[k].ok) continue;                    // (uploaded by the names thread)
            R.status = 0;
            R.usize = nd[k].u_len;
        }
        for (size_t k = 0; k < reqs.size(); k++) {
            if (who[k] < 0) continue;                   // an LZP3 section's rANS stage
            fqz5_section_result &R = res[who[k]];
            R.status = reqs[k].ok ? 0 : -1;
            R.usize = reqs[k].out_size;
        }
        for (size_t k = 0; k < seqd.size(); k++) {
            if (seq_on_host[k]) continue;
            fqz5_section_result &R = res[who_seq[k]];
            R.status = seqd[k].ok ? 0 : -1;
            R.usize = seqd[k].n;
        }
        for (size_t k = 0; k < fqz.size(); k++) {
            if (fqz_on_host[k]) continue;
            fqz5_section_result &R = res[who_fqz[k]];
            R.status = fqz[k].ok ? 0 : -1;
            R.usize = uint32_t(fqz[k].out_size);
        }
        g.reset();
        if (gn) gn->reset();
        if (gf) gf->reset();
        if (gs) gs->reset();
        if (trace) {
            std::fprintf(stderr, "decode_sections: from its start: rANS done %.1f, host chains joined "
                         "%.1f, names uploaded %.1f, names joined %.1f, reset %.1f ms\n", t_rans - t0,
                         t_hc - t0, t_names_up ? t_names_up - t0 : -1.0, t_nj - t0, now_ms() - t0);
        }
        return 0;
    } catch (const std::exception &e) {
        fqz5_set_error(e.what());
        try { gpu().reset(); } catch (...) {}
        try { gpu_aux_reset_all(); } catch (...) {}
        return -1;
    }
}

}  // extern "C"
