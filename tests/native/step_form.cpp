// step_form.cpp -- a step's form and the outputs it stores (csrc/mph_kernels.h seq_step,
// trim_outputs) over all 64 combinations of: a sequence's storing last step or not,
// surface tension, the coarse map allocated, monitors on, MPH_LEAN_STEPS, the context's lean-search
// capability.  The rules are written out below as this program's own table and never taken from the
// code under test.  Built and run by tests/test_step_form.py with the host compiler; needs no GPU.
#include <cstdint>
#include <cstdio>

#include "../../particlemethod_fsi_amd/csrc/mph_kernels.h"

using namespace mph;

namespace {

struct Case {
    bool last, surface, cmap, mon, lean_ok, lean_search;
};

// ---- the rules -------------------------------------------------------------------------------
// the form
bool want_lazy(const Case& c) { return !c.last && c.cmap && !c.mon; }
bool want_lean_search(const Case& c) { return want_lazy(c) && c.lean_ok && c.lean_search; }
bool want_lean_pass_a(const Case& c) { return want_lazy(c) && c.lean_ok && !c.surface; }
// the nine trimmed outputs: null on a step that is not the last of its batch -- GravityCenter and
// PressureA only without surface tension (pass B reads them with it)
bool null_always(const Case& c) { return !c.last; }
bool null_without_surface(const Case& c) { return !c.last && !c.surface; }
struct Trimmed {
    const char* name;
    const void* (*get)(const Launch&);
    bool (*want_null)(const Case&);
};
const Trimmed kTrimmed[9] = {
    {"dens_a", [](const Launch& L) -> const void* { return L.dens_a; }, null_always},
    {"vstrain", [](const Launch& L) -> const void* { return L.vstrain; }, null_always},
    {"divp", [](const Launch& L) -> const void* { return L.divp; }, null_always},
    {"gx", [](const Launch& L) -> const void* { return L.gx; }, null_without_surface},
    {"gy", [](const Launch& L) -> const void* { return L.gy; }, null_without_surface},
    {"gz", [](const Launch& L) -> const void* { return L.gz; }, null_without_surface},
    {"pa", [](const Launch& L) -> const void* { return L.pa; }, null_without_surface},
    {"force", [](const Launch& L) -> const void* { return L.force; }, null_always},
    {"acc", [](const Launch& L) -> const void* { return L.acc; }, null_always},
};

// ---- a context's Launch with a distinct value in every field ----------------------------------
int next_tag = 0;
template <typename T>
void tag(T*& p) { p = reinterpret_cast<T*>(static_cast<std::uintptr_t>(0x1000 + 0x100 * ++next_tag)); }
void tag(Soa& s)
{
    tag(s.x); tag(s.y); tag(s.z); tag(s.vx); tag(s.vy); tag(s.vz); tag(s.type); tag(s.id); tag(s.p6); tag(s.f4);
}

Launch context_launch(const Case& c, const DevParams* P, const MonitorDev* mon)
{
    Launch L;
    L.P = P;
    tag(L.T); tag(L.st); tag(L.stream); tag(L.prof);
    tag(L.A); tag(L.B);
    tag(L.dst_of); tag(L.key); tag(L.slot); tag(L.tmp); tag(L.cnt); tag(L.start); tag(L.bsum);
    tag(L.nbr); tag(L.ncount); tag(L.nbcount); tag(L.lhdr); tag(L.lgap); tag(L.wface);
    tag(L.vsrc.idx); tag(L.vsrc.n); tag(L.vsrc.V);
    L.xcd_bal_min = 12345;
    if (c.cmap) tag(L.cmap);
    L.cmap_bytes = c.cmap ? 4096 : 0;
    L.lean_ok = c.lean_ok;
    L.lean_search = c.lean_search;
    tag(L.pres); tag(L.gx); tag(L.gy); tag(L.gz); tag(L.pa); tag(L.dens_a); tag(L.vstrain); tag(L.divp);
    tag(L.fpart); tag(L.rec); tag(L.force); tag(L.acc);
    tag(L.S);
    L.mon = c.mon ? mon : nullptr;
    return L;
}

bool same(const Soa& a, const Soa& b)
{
    return a.x == b.x && a.y == b.y && a.z == b.z && a.vx == b.vx && a.vy == b.vy && a.vz == b.vz &&
           a.type == b.type && a.id == b.id && a.p6 == b.p6 && a.f4 == b.f4;
}

// everything but the nine trimmed outputs and the form
bool untrimmed_same(const Launch& a, const Launch& b)
{
    return a.P == b.P && a.T == b.T && a.st == b.st && a.stream == b.stream && a.prof == b.prof && same(a.A, b.A) &&
           same(a.B, b.B) && a.dst_of == b.dst_of && a.key == b.key && a.slot == b.slot && a.tmp == b.tmp &&
           a.cnt == b.cnt && a.start == b.start && a.bsum == b.bsum && a.nbr == b.nbr && a.ncount == b.ncount &&
           a.nbcount == b.nbcount && a.lhdr == b.lhdr && a.lgap == b.lgap && a.wface == b.wface &&
           a.vsrc.idx == b.vsrc.idx && a.vsrc.n == b.vsrc.n && same(a.vsrc.V, b.vsrc.V) &&
           a.xcd_bal_min == b.xcd_bal_min && a.cmap == b.cmap && a.cmap_bytes == b.cmap_bytes &&
           a.lean_ok == b.lean_ok && a.lean_search == b.lean_search && a.pres == b.pres && a.fpart == b.fpart &&
           a.rec == b.rec && a.S == b.S && a.mon == b.mon;
}

int failures = 0;

void expect(bool ok, int bits, const char* what)
{
    if (ok) return;
    std::printf("case %d%d%d%d%d%d (last surface cmap mon lean_ok lean_search): FAILED %s\n", bits & 1, (bits >> 1) & 1,
                (bits >> 2) & 1, (bits >> 3) & 1, (bits >> 4) & 1, (bits >> 5) & 1, what);
    ++failures;
}

}  // namespace

int main()
{
    int lazy = 0, lean_s = 0, lean_a = 0;
    for (int bits = 0; bits < 64; ++bits) {
        const Case c{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0};
        DevParams P{};
        P.surface = c.surface ? 1 : 0;
        MonitorDev mon;
        next_tag = 0;
        const Launch L = context_launch(c, &P, &mon);
        expect(!L.form.lazy && !L.form.lean_search && !L.form.lean_pass_a, bits, "the context's own form is all false");

        // a sequence of one step, storing or not: the step alone, with nothing to fold
        const Launch S = seq_step(L, StepSeq{1, c.last}, 0);
        expect(S.form.lazy == want_lazy(c), bits, "form.lazy");
        expect(S.form.lean_search == want_lean_search(c), bits, "form.lean_search");
        expect(S.form.lean_pass_a == want_lean_pass_a(c), bits, "form.lean_pass_a");
        for (const Trimmed& t : kTrimmed) {
            const void* got = t.get(S);
            expect(t.want_null(c) ? got == nullptr : (got != nullptr && got == t.get(L)), bits, t.name);
        }
        expect(untrimmed_same(S, L), bits, "an untrimmed field changed");
        expect(!S.form.keys_done && !S.form.keys_next && !S.cmap_next, bits, "a single step folds nothing");
        // what the launchers read: the map on a lazy step alone, a stored Force on a storing step alone
        expect(lazy_cmap(S) == (want_lazy(c) ? L.cmap : nullptr), bits, "lazy_cmap");
        expect(stores_outputs(S) == c.last, bits, "stores_outputs");
        lazy += S.form.lazy;
        lean_s += S.form.lean_search;
        lean_a += S.form.lean_pass_a;

        // the first half alone (mph_profile_graphs): a non-last step's outputs, never a form
        const Launch T = trim_outputs(L);
        const Case not_last{false, c.surface, c.cmap, c.mon, c.lean_ok, c.lean_search};
        for (const Trimmed& t : kTrimmed) {
            const void* got = t.get(T);
            expect(t.want_null(not_last) ? got == nullptr : (got != nullptr && got == t.get(L)), bits, t.name);
        }
        expect(!T.form.lazy && !T.form.lean_search && !T.form.lean_pass_a, bits, "trim_outputs sets no form");
        expect(untrimmed_same(T, L), bits, "trim_outputs changed an untrimmed field");
    }
    // of the 64 combinations: lazy needs !last, cmap, !mon (8); lean_search also lean_ok and the
    // capability (2); lean_pass_a also lean_ok and no surface tension (2)
    std::printf("lazy %d, lean_search %d, lean_pass_a %d of 64\n", lazy, lean_s, lean_a);
    if (lazy != 8 || lean_s != 2 || lean_a != 2) {
        std::printf("FAILED the counts over the 64 combinations\n");
        ++failures;
    }
    if (failures) return 1;
    std::printf("step_form ok\n");
    return 0;
}
