// replay_plan.cpp -- how a call's steps are cut into batches (csrc/mph_kernels.h replay_plan; DESIGN.md
// section 3.1) for n = 1 ... 80 with and without the all-lean 8-step graph and the lean single step,
// and the key fold's two fields of a step's form (seq_step; section 3.2) over every combination of
// the step's place in its sequence, structures, monitors, a slab's set and the toggle.  The rules are
// written out below as this program's own and never taken from the code under test.  Built and run
// by tests/test_replay_plan.py with the host compiler; needs no GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../particlemethod_fsi_amd/csrc/mph_kernels.h"

using namespace mph;

namespace {

int failures = 0;

void expect(bool ok, const char* what, int a, int b, int c)
{
    if (ok) return;
    std::printf("FAILED %s (%d %d %d)\n", what, a, b, c);
    ++failures;
}

// ---- the plan ---------------------------------------------------------------------------------
// A plan as the steps it launches, in order: 1 where the step stores the output-only fields.
std::vector<int> steps_of(const ReplayPlan& p)
{
    std::vector<int> s;
    for (int k = 0; k < p.count[kSeq8t]; ++k) s.insert(s.end(), {0, 0, 0, 0, 0, 0, 0, 0});
    for (int k = 0; k < p.count[kSeq8]; ++k) s.insert(s.end(), {0, 0, 0, 0, 0, 0, 0, 1});
    for (int k = 0; k < p.count[kSeq1t]; ++k) s.push_back(0);
    for (int k = 0; k < p.count[kSeq1]; ++k) s.push_back(1);
    return s;
}

// the plan's four counts under the names of the rules below
struct Counts {
    int batch8t, batch8, single1t, single1;
};
Counts counts_of(const ReplayPlan& q) { return {q.count[kSeq8t], q.count[kSeq8], q.count[kSeq1t], q.count[kSeq1]}; }

// The rules.  The sequence before the lean batches: graph8 while 8 or more steps are left, then
// single steps -- all but the last without the stores where the context has the lean single step.
std::vector<int> before(int n, bool lean1)
{
    std::vector<int> s;
    for (; n >= 8; n -= 8) s.insert(s.end(), {0, 0, 0, 0, 0, 0, 0, 1});
    for (; n > 1; --n) s.push_back(lean1 ? 0 : 1);
    if (n == 1) s.push_back(1);
    return s;
}

void check_plan(int n, bool lean8, bool lean1)
{
    const ReplayPlan plan = replay_plan(n, lean8, lean1);
    const Counts p = counts_of(plan);
    const std::vector<int> s = steps_of(plan);
    expect((int)s.size() == n, "the step total", n, lean8, lean1);
    expect(!s.empty() && s.back() == 1, "the call's last step stores", n, lean8, lean1);
    expect(p.batch8t >= 0 && p.batch8 >= 0 && p.single1t >= 0 && p.single1 >= 0, "a negative count", n, lean8, lean1);
    expect(p.batch8t == (lean8 && n / 8 >= 2 ? n / 8 - 1 : 0), "the lean batches: max(0, n / 8 - 1)", n, lean8, lean1);
    expect(8 * (p.batch8t + p.batch8) == n - n % 8 && p.single1t + p.single1 == n % 8, "batches and remainder", n,
           lean8, lean1);
    expect(!lean8 || p.batch8 == (n >= 8 ? 1 : 0), "one storing batch, the last whole one", n, lean8, lean1);
    expect(p.single1t == (lean1 && n % 8 > 1 ? n % 8 - 1 : 0), "the remainder as before", n, lean8, lean1);
    // the storing steps: with both lean graphs the call's last step and, where a remainder follows
    // it, the last step of the last whole batch (mph_step(13) keeps its 7 + 4 lazy steps) -- one
    // storing step, the last, where n is a multiple of 8 or below 8
    int stores = 0;
    for (int v : s) stores += v;
    if (lean8 && lean1) {
        const int want = 1 + (n >= 8 && n % 8 ? 1 : 0);
        expect(stores == want, "the storing steps with both lean graphs", n, stores, want);
        if (n >= 8 && n % 8) expect(s[8 * (n / 8) - 1] == 1, "the last whole batch stores on its last step", n, 0, 0);
    }
    if (!lean8 || n < 16) expect(s == before(n, lean1), "the sequence before the lean batches", n, lean8, lean1);
    // a storing step never precedes a lean batch
    const int first_store = (int)(std::find(s.begin(), s.end(), 1) - s.begin());
    expect(first_store >= 8 * p.batch8t, "a store inside the lean batches", n, lean8, lean1);
}

// ---- the extended form ------------------------------------------------------------------------
struct FoldCase {
    bool toggle, structures, monitors, slab, lazy_walls;
};

// the rule: a step's keys come from the step before it in the same sequence, and only there; never
// with structure particles, monitors or a slab's set, or with the toggle off
bool fold_on(const FoldCase& c) { return c.toggle && !c.structures && !c.monitors && !c.slab; }

void check_fold(int bits)
{
    const FoldCase c{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0};
    DevParams P{};
    P.n_struct = c.structures ? 5 : 0;
    MonitorDev mon;
    int idx = 0;
    unsigned char map = 0;
    double4 force;
    Launch L;
    L.P = &P;
    L.force = &force;
    L.key_fold = c.toggle;
    L.mon = c.monitors ? &mon : nullptr;
    L.vsrc.idx = c.slab ? &idx : nullptr;
    L.cmap = c.lazy_walls ? &map : nullptr;
    expect(!L.form.keys_done && !L.form.keys_next && !L.cmap_next, "the context's own form", bits, 0, 0);
    // the sequences a context enqueues: a graph of 1 or 8 steps, storing on its last or not at all;
    // the profiler's batch of 9
    const int shapes[5][2] = {{1, 1}, {1, 0}, {8, 1}, {8, 0}, {9, 1}};
    for (const auto& sh : shapes) {
        const int steps = sh[0];
        const bool store_last = sh[1] != 0;
        bool prev_next = false;   // keys_next of the step before; false before a sequence's first
        for (int k = 0; k < steps; ++k) {
            const bool last = store_last && k == steps - 1, next_last = store_last && k + 1 == steps - 1;
            const Launch S = seq_step(L, StepSeq{steps, store_last}, k);
            expect(S.form.keys_done == prev_next, "keys_done of step k + 1 <=> keys_next of step k", bits, steps, k);
            expect(S.form.keys_next == (fold_on(c) && k + 1 < steps), "keys_next", bits, steps, k);
            expect(!(k == steps - 1 && S.form.keys_next), "keys_next across a sequence's end", bits, steps, k);
            expect(!(k == 0 && S.form.keys_done), "keys_done on a sequence's first step", bits, steps, k);
            expect(!(S.form.keys_next && last), "keys_next on a storing step", bits, steps, k);
            // the next step's coarse map: only where that step is lazy (not a storing one, the map
            // allocated, no monitors)
            const bool next_lazy = S.form.keys_next && !next_last && c.lazy_walls && !c.monitors;
            expect(S.cmap_next == (next_lazy ? &map : nullptr), "cmap_next", bits, steps, k);
            // nothing else of the step's Launch changes
            // the rest of the step's Launch is what the step alone would have: lazy unless it stores (the
            // map allocated, no monitors), never lean here (L.lean_ok is off), Force on the storing step
            expect(S.form.lazy == (!last && c.lazy_walls && !c.monitors) && !S.form.lean_search &&
                       !S.form.lean_pass_a && S.force == (last ? &force : nullptr) && S.cmap == L.cmap && S.P == L.P &&
                       S.mon == L.mon,
                   "the fold changed another field", bits, steps, k);
            prev_next = S.form.keys_next;
        }
    }
}

}  // namespace

int main()
{
    for (int n = 1; n <= 80; ++n)
        for (int g = 0; g < 4; ++g) check_plan(n, (g & 1) != 0, (g & 2) != 0);
    // the calls the GPU tests pin
    const Counts p40 = counts_of(replay_plan(40, true, true)), p16 = counts_of(replay_plan(16, true, true)),
                 p13 = counts_of(replay_plan(13, true, true));
    expect(p40.batch8t == 4 && p40.batch8 == 1 && p40.single1t == 0 && p40.single1 == 0, "mph_step(40)", 40, 0, 0);
    expect(p16.batch8t == 1 && p16.batch8 == 1 && p16.single1t == 0 && p16.single1 == 0, "mph_step(16)", 16, 0, 0);
    expect(p13.batch8t == 0 && p13.batch8 == 1 && p13.single1t == 4 && p13.single1 == 1, "mph_step(13)", 13, 0, 0);
    const Counts z = counts_of(replay_plan(0, true, true));
    expect(z.batch8t + z.batch8 + z.single1t + z.single1 == 0, "no step, no launch", 0, 0, 0);
    // the four kinds are the sequences steps_of writes out, in the plan's launch order
    const int kinds[4][2] = {{8, 0}, {8, 1}, {1, 0}, {1, 1}};
    for (int kind = 0; kind < 4; ++kind)
        expect(kSeqKinds == 4 && kSeqs[kind].steps == kinds[kind][0] && kSeqs[kind].store_last == (kinds[kind][1] != 0),
               "the four kinds", kind, 0, 0);
    for (int bits = 0; bits < 32; ++bits) check_fold(bits);
    if (failures) return 1;
    std::printf("replay_plan ok\n");
    return 0;
}
