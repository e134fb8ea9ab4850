// tools/gmres_drive_check.cpp — dev tool: gmres_drive.hpp (the host loop of mi_gmres_solve_dev and mi_gmres_plan_solve, and the two
// batch rules) under the host address and undefined-behaviour sanitizers, with no GPU: the loop drives two fake backends over a
// scripted "device", a GmresRecord updated in plain C++ by the counting rules of gmres_cycle_begin and gmres_hess_step (a step counts
// unless the record holds a reason or its >= maxiter; a script says at which step of which cycle reason 1, 3 or 4 appears and which
// start meets rtol).  Work "runs" when it is enqueued, which stream order allows.  Grid: restart m in {1, 2, 5}, maxiter in
// {0, 1, m - 1, m, m + 1, 2 m + 2}, check_every = segment in {1, 2, m, m + 3}, both bases, and per m the scripts of scripts_for().
// For every case:
//   results   iterations, reason, history (all maxiter + 1 places), refused and the k of every cycle's end equal those of reference(),
//             a loop with no pipeline that looks at the record after every single step; the eager and the planned backend agree
//   slots     no read-back goes into a slot whose earlier read-back the host still has to wait for (one the host has walked away
//             from at a cycle's end is never looked at again, and stream order puts the next copy behind it); every wait is for a slot
//             that was enqueued; at every wait either a later batch is already enqueued or nothing more can be enqueued
//   enqueue   steps in order, none at k >= m, the eager backend none at its + k >= maxiter; the end exactly when k > 0, with the
//             record's k; every read-back carries the entries of the steps enqueued so far
//   bounds    include/mi355_spmv.h's, of the steps enqueued behind the one that froze the cycle (`wasted` also holds a step that found
//             reason 4 itself: it is not counted).  Eager: wasted <= 2 check_every - 1 per cycle, and per solve with the double basis; readbacks <=
//             ceil(its / check_every) + cycles + 1.  Planned: wasted <= 2 segment - 1 per cycle, and what tests/test_gpu_gmres_plan.py
//             asserts of wasted, readbacks and replays.  cycles: the starts (in that file's solves ceil(its / restart) is the same number)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Inavierstokes_amd/csrc -o /tmp/gmres_drive_check tools/gmres_drive_check.cpp && /tmp/gmres_drive_check
#include "gmres_drive.hpp"
#include <cstdio>
#include <string>
#include <vector>
using namespace mi355;

static int bad = 0, cases = 0;
static std::string g_case;

static void fail(const char* what)
{
    if (bad < 40) printf("%s: %s\n", g_case.c_str(), what);
    bad++;
}

struct CycleScript {
    bool meets = false;      // this cycle's start meets rtol
    int step = -1, reason = 0; // at this step this reason appears (4: the step is not counted)
};
typedef std::vector<CycleScript> Script; // cycles behind its end: nothing happens

struct Device {
    int m = 0, maxiter = 0;
    const Script* script = nullptr;
    GmresRecord rec{};
    std::vector<double> hcyc;
    int cycle = -1;
    CycleScript now() const { return cycle < (int)script->size() ? (*script)[(size_t)cycle] : CycleScript{}; }
    void begin(bool first)
    {
        cycle++;
        hcyc.assign((size_t)m, -1.0);
        if (first) rec.its = 0, rec.bnorm = 1.0;
        int reason = 0;
        if (now().meets) reason = rec.its == 0 ? kGmresMetAtStart : 1;
        else if (rec.its >= maxiter) reason = 2;
        rec.k = 0, rec.reason = reason, rec.beta = 100.0 + cycle, rec.rel0 = 0.5 + cycle;
        if (first) rec.last = rec.rel0;
    }
    void step(int k)
    {
        if (rec.reason != 0 || rec.its >= maxiter) return;
        if (k != rec.k) return fail("a step runs that is not the next one to count");
        const CycleScript c = now();
        if (c.step == k && c.reason == 4) {
            rec.reason = 4;
            return;
        }
        hcyc[(size_t)k] = rec.last = 1000.0 * cycle + k + 0.25;
        rec.its++, rec.k = k + 1;
        if (c.step == k) rec.reason = c.reason;
    }
};

struct Result {
    int its = 0, reason = 0, refused = 0;
    std::vector<double> history;
    std::vector<int> ends;
    bool operator==(const Result& o) const { return its == o.its && reason == o.reason && refused == o.refused && history == o.history && ends == o.ends; }
};

// the definition (include/mi355_spmv.h), one step at a time
static Result reference(int m, int maxiter, bool f32, const Script& script)
{
    Device D;
    D.m = m, D.maxiter = maxiter, D.script = &script;
    Result R;
    R.history.assign((size_t)maxiter + 1, -7.0);
    bool claimed = false;
    for (bool first = true;; first = false) {
        D.begin(first);
        if (first) R.history[0] = D.rec.rel0;
        const int its0 = D.rec.its;
        while (D.rec.reason == 0 && D.rec.k < m && D.rec.its < maxiter) D.step(D.rec.k);
        const int k = D.rec.k;
        for (int j = 0; j < k; j++) R.history[(size_t)(its0 + 1 + j)] = D.hcyc[(size_t)j];
        if (k > 0) R.ends.push_back(k);
        R.its = D.rec.its;
        R.reason = D.rec.reason == kGmresMetAtStart ? 0 : D.rec.reason;
        const bool confirmed = D.rec.reason == 1 && k == 0;
        if (claimed && !confirmed) R.refused++;
        claimed = f32 && D.rec.reason == 1 && k > 0;
        if (claimed) continue;
        if (D.rec.reason != 0) break;
        if (R.its >= maxiter) {
            R.reason = 2;
            break;
        }
    }
    return R;
}

// what both fake backends share: the device, the two slots, and the checks
struct Fake {
    Device D;
    bool eager = false;
    struct Slot {
        bool filled = false;
        GmresRecord rec{};
        std::vector<double> ent;
    } slot[2];
    int next = 0, outstanding = 0;
    int k_enq = 0, its0 = 0, starts = 0, waits = 0, wasted = 0, behind = 0, worst_cycle_behind = 0;
    bool in_cycle = false, ended = false;
    std::vector<int> ends;

    // the host has left the cycle's loop: a read-back it did not wait for is never looked at
    void abandon()
    {
        for (Slot& s : slot)
            if (s.filled) s.filled = false, s.ent.clear(), s.ent.shrink_to_fit();
        outstanding = 0;
    }
    void close_cycle()
    {
        if (!in_cycle) return;
        abandon();
        if ((D.rec.k > 0) != ended) fail("the end is not called exactly when k > 0");
        const int waste = k_enq - D.rec.k;
        wasted += waste;
        // what the bounds speak of: the steps BEHIND the one that froze the cycle.  A step that finds reason 4 is not counted, so
        // `wasted` holds it too, though it is the step that told
        const int after = waste - (D.rec.reason == 4 ? 1 : 0);
        behind += after;
        worst_cycle_behind = std::max(worst_cycle_behind, after);
        in_cycle = false;
    }
    int start(bool first)
    {
        close_cycle();
        D.begin(first);
        starts++, k_enq = 0, its0 = D.rec.its, ended = false, in_cycle = true;
        return 0;
    }
    void enqueue_step(int k)
    {
        if (k != k_enq) fail("steps are not enqueued in order");
        if (k >= D.m) return fail("a step k >= m is enqueued");
        if (eager && its0 + k >= D.maxiter) fail("the eager backend enqueues a step at its + k >= maxiter");
        D.step(k);
        k_enq++;
    }
    int readback(int entries, int* s)
    {
        Slot& S = slot[next];
        if (S.filled) fail("a read-back goes into a slot the host has not waited for");
        if (entries != k_enq || entries > D.m) {
            fail("a read-back does not carry the entries of the steps enqueued");
            return 1;
        }
        S.filled = true, S.rec = D.rec;
        S.ent.assign(D.hcyc.begin(), D.hcyc.begin() + entries);
        *s = next, next ^= 1, outstanding++;
        return 0;
    }
    int wait(int s, GmresRecord* rec, const double** entries)
    {
        if (s < 0 || s > 1 || !slot[s].filled) {
            fail("a wait for a slot that was not enqueued");
            return 1;
        }
        slot[s].filled = false, outstanding--, waits++;
        if (outstanding == 0 && std::min(D.m - k_enq, D.maxiter - its0 - k_enq) > 0) fail("the host waits with nothing enqueued behind and room for more");
        *rec = slot[s].rec, *entries = slot[s].ent.data();
        return 0;
    }
    int end(int k)
    {
        abandon();
        if (k <= 0 || k != D.rec.k || ended) fail("the end is called with k <= 0, not the record's k, or twice");
        ended = true;
        ends.push_back(k);
        return 0;
    }
};

struct FakeEager : Fake {
    int check_every = 1;
    int batch(int& k, int room, bool first_batch)
    {
        const int k1 = gmres_eager_batch(k, room, first_batch, check_every);
        for (int j = k; j < k1; j++) enqueue_step(j);
        k = k1;
        return 0;
    }
};

struct FakePlanned : Fake {
    int segment = 1, replays = 0; // (segment as mi_gmres_plan_create clamps it)
    int start(bool first) { return replays++, Fake::start(first); }
    int batch(int& k, int, bool first_batch)
    {
        int g;
        k = gmres_plan_batch(k, D.m, first_batch, segment, &g);
        if (g < 0) return 0;
        replays++; // the segment's graph: its steps whatever maxiter says
        for (int j = g * segment; j < std::min(D.m, (g + 1) * segment); j++) enqueue_step(j);
        if (k != k_enq) fail("the planned count is not the end of the segment replayed");
        return 0;
    }
    int end(int k) { return replays++, Fake::end(k); }
};

template <class B>
static Result drive(B& F, int m, int maxiter, bool f32, const Script& script, GmresOutcome& out)
{
    F.D.m = m, F.D.maxiter = maxiter, F.D.script = &script;
    Result R;
    R.history.assign((size_t)maxiter + 1, -7.0);
    if (gmres_drive(F, m, maxiter, f32, R.history.data(), out)) fail("the driver returned an error");
    F.close_cycle();
    R.its = out.its, R.reason = out.reason, R.refused = out.refused, R.ends = F.ends;
    if (out.last_k != F.D.rec.k || out.last_beta != F.D.rec.beta) fail("last_k / last_beta are not the last record's");
    if (out.wasted != F.wasted || out.readbacks != F.waits) fail("wasted / readbacks are not what was enqueued for nothing / waited for");
    return R;
}

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

static void check(int m, int maxiter, int v, bool f32, const Script& script, int script_no)
{
    cases++;
    g_case = "m " + std::to_string(m) + " maxiter " + std::to_string(maxiter) + " check_every/segment " + std::to_string(v) + (f32 ? " f32" : " f64") +
             " script " + std::to_string(script_no);
    const Result want = reference(m, maxiter, f32, script);
    GmresOutcome oe, op;
    FakeEager E;
    E.eager = true, E.check_every = v;
    if (!(drive(E, m, maxiter, f32, script, oe) == want)) fail("eager: iterations, reason, history, refused or the ends differ from the reference loop");
    FakePlanned P;
    P.segment = std::min(v, m);
    if (!(drive(P, m, maxiter, f32, script, op) == want)) fail("planned: iterations, reason, history, refused or the ends differ from the reference loop");
    // the header's bounds
    if (E.worst_cycle_behind > 2 * v - 1 || (!f32 && E.behind > 2 * v - 1)) fail("eager: wasted steps beyond 2 check_every - 1");
    if (oe.readbacks > ceil_div(oe.its, v) + E.starts + 1) fail("eager: read-backs beyond ceil(its / check_every) + cycles + 1");
    const int seg = P.segment, early = f32 ? 2 * (op.refused + 1) + 1 : 1;
    if (P.worst_cycle_behind > 2 * seg - 1 || P.behind > early * (2 * seg - 1)) fail("planned: wasted steps beyond 2 segment - 1 per cycle that ends early");
    if (op.readbacks > ceil_div(op.its, seg) + 2 * P.starts + 1) fail("planned: read-backs beyond ceil(its / segment) + 2 cycles + 1");
    if (P.replays > op.readbacks + 2 * P.starts + 1) fail("planned: replays beyond readbacks + 2 cycles + 1");
}

// no freeze; a freeze with reason 1, 3 and 4 at every step of the first and of the second cycle (with the float basis reason 1 is a
// claim that the next start refuses); rtol met at the first start and at a later one; a claim confirmed, refused once, refused twice
static std::vector<Script> scripts_for(int m)
{
    std::vector<Script> all(1);
    for (int c = 0; c < 2; c++)
        for (int s = 0; s < m; s++)
            for (int r : {1, 3, 4}) {
                Script sc((size_t)c + 1);
                sc[(size_t)c].step = s, sc[(size_t)c].reason = r;
                all.push_back(sc);
            }
    CycleScript none, meets, claim_first, claim_last;
    meets.meets = true;
    claim_first.step = 0, claim_first.reason = 1;
    claim_last.step = m - 1, claim_last.reason = 1;
    all.push_back({meets});
    all.push_back({none, meets});
    all.push_back({claim_last, meets});
    all.push_back({claim_first, claim_last, meets});
    all.push_back({claim_first, claim_first, claim_last, meets});
    return all;
}

int main()
{
    for (int m : {1, 2, 5}) {
        const std::vector<Script> scripts = scripts_for(m);
        for (int maxiter : {0, 1, m - 1, m, m + 1, 2 * m + 2})
            for (int v : {1, 2, m, m + 3})
                for (int f32 = 0; f32 < 2; f32++)
                    for (size_t i = 0; i < scripts.size(); i++) check(m, maxiter, v, f32 != 0, scripts[i], (int)i);
    }
    printf("gmres_drive cases %d\nbad %d\n", cases, bad);
    return bad != 0;
}
