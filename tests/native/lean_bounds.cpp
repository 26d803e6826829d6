// lean_bounds.cpp -- the radii of the lean search (csrc/mph_params.h set_uniforms, lean_search_ok)
// on the radii and domains of d1m, d16m, box3d and dam2d: the list radius lies below the FP32 band
// of the search radius, the lean trimming bound between the list radius and the full search's
// bound, and the guard turns the lean search off when the lists keep every pair.  Built and run by
// tests/test_lean_bounds.py; needs no GPU.
#include <cfloat>
#include <cstdio>

#include "../../particlemethod_fsi_amd/csrc/mph_params.h"

using namespace mph;

namespace {

struct Input {
    const char* name;
    double dx, ratio;        // ParticleSpacing, RadiusRatio (A = G = P = V)
    double lo[3], hi[3];     // the domain
};

// cases.py: dam2d, d1m, d16m, box3d (RadiusRatio 2.5; MARGIN = 0.1 dx, main.cpp:116)
const Input kInputs[] = {
    {"d1m", 0.001, 2.5, {-0.01, 0.0, -0.01}, {0.21, 0.40, 0.11}},
    {"d16m", 0.0004, 2.5, {-0.004, 0.0, -0.004}, {0.208, 0.40, 0.108}},
    {"box3d", 0.001, 2.5, {-0.01, 0.0, -0.01}, {0.04, 0.05, 0.025}},
    {"dam2d", 0.001, 2.5, {-0.01, 0.0, 0.0}, {0.21, 0.40, 0.001}},
};

int failures = 0;

void expect(bool ok, const char* name, const char* what)
{
    if (ok) return;
    std::printf("%s: FAILED %s\n", name, what);
    ++failures;
}

}  // namespace

int main()
{
    for (const Input& in : kInputs) {
        DevParams P{};
        const double r = in.ratio * in.dx, rc = r + 0.1 * in.dx;
        P.ra = P.rg = P.rp = P.rv = r;
        P.rc2 = rc * rc;
        P.r2g = 1.0;
        for (int d = 0; d < 3; ++d) {
            P.dmin[d] = in.lo[d];
            P.dw[d] = in.hi[d] - in.lo[d];
            P.hw[d] = 0.5 * P.dw[d];
            P.ginv[d] = 3.0 / rc;
        }
        set_uniforms(P);
        const double rl2 = r * r;
        std::printf("%s: rl2 %.9g rlf %.9g rl_trimf %.9g rc2f_lo %.9g rc2_trim %.9g lean %d\n", in.name, rl2,
                    (double)P.rlf, (double)P.rl_trimf, (double)P.rc2f_lo, P.rc2_trim, (int)lean_search_ok(P));
        expect(P.rlf <= P.rc2f_lo, in.name, "rlf <= rc2f_lo");
        expect(lean_search_ok(P), in.name, "lean_search_ok");
        expect(rl2 <= (double)P.rl_trimf, in.name, "list radius^2 <= lean trim bound");
        expect((double)P.rlf <= (double)P.rl_trimf, in.name, "rlf <= lean trim bound");
        expect((double)P.rl_trimf <= P.rc2_trim, in.name, "lean trim bound <= rc2_trim");
        // MPH_LIST_FULL=1 (ctx_fill_launch): the lists keep every pair
        P.rlf = FLT_MAX;
        expect(!lean_search_ok(P), in.name, "the guard is off with rlf = FLT_MAX");
        P.rlf = 3.0e38f;
        expect(!lean_search_ok(P), in.name, "the guard is off with rlf = 3e38");
    }
    if (failures) return 1;
    std::printf("lean_bounds ok\n");
    return 0;
}
