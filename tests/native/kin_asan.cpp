// kin_asan.cpp -- the host half of the kinematics (include/mph_gpu.h mph_kinematics_*; csrc/mph_host.cpp,
// the shared inlines of csrc/mph_params.h) under ASan + UBSan: a jittered block with a lone particle, a
// pair and a coplanar group beside it, in 2-D and 3-D, every radius rule, the text form, the layout, the
// lattice sum and the .vtu writer.  Prints one line per check and returns 0 when all hold.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mph_gpu.h"

static int g_bad = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++g_bad;                                                      \
        }                                                                 \
    } while (0)

static double jitter(unsigned& s)
{
    s = s * 1664525u + 1013904223u;
    return ((s >> 8) & 0xffff) / 65536.0 - 0.5;
}

static void run(int dim, const char* vtu)
{
    MphConfig cfg;
    CHECK(mph_config_default(&cfg, dim, MPH_MODULE_DAM) == MPH_OK);
    const double dx = 0.001;
    cfg.particle_spacing = dx;
    cfg.radius_ratio_a = cfg.radius_ratio_p = cfg.radius_ratio_v = 2.5;
    for (int d = 0; d < 3; ++d) {
        cfg.domain_min[d] = 0.0;
        cfg.domain_max[d] = d < dim ? 0.04 : dx;
    }
    std::vector<double> pos, vel;
    std::vector<int> prop;
    unsigned seed = 7u + dim;
    auto add = [&](double x, double y, double z, int t) {
        pos.insert(pos.end(), {x, y, dim == 3 ? z : 0.0});
        vel.insert(vel.end(), {0.7 * x - 1.3 * y, 2.1 * x - 0.5 * y + 0.2 * x * y, dim == 3 ? 0.3 * z - 0.8 * x : 0.0});
        prop.push_back(t);
    };
    const int m = dim == 3 ? 7 : 12;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j)
            for (int k = 0; k < (dim == 3 ? m : 1); ++k)
                add(0.004 + dx * (i + 0.3 * jitter(seed)), 0.004 + dx * (j + 0.3 * jitter(seed)),
                    0.004 + dx * (k + 0.3 * jitter(seed)), (i + j + k) % 6);
    const int block = (int)prop.size();
    add(0.03, 0.03, 0.03, 0);                                         // alone
    add(0.03, 0.02, 0.03, 0); add(0.03 + dx, 0.02, 0.03, 1);          // a pair
    for (int k = 0; k < 4; ++k) add(0.02 + 0.7 * dx * k, 0.03, 0.03, 0);   // collinear (3-D: also coplanar)
    const int n = (int)prop.size();
    std::vector<double> out((size_t)n * MPH_KIN_CHANNELS, -1.0);
    MphKinematics k;
    CHECK(mph_kinematics_parse("", &k) == MPH_OK);
    CHECK(mph_kinematics_arrays(&cfg, &k, n, prop.data(), pos.data(), vel.data(), out.data()) == MPH_OK);
    const double* lone = &out[(size_t)block * MPH_KIN_CHANNELS];
    CHECK(lone[MPH_KIN_COUNT] == 0.0 && lone[MPH_KIN_FLAGS] == 7.0 && lone[MPH_KIN_WSUM] == 0.0);
    for (int i = block + 1; i < n; ++i) {
        const double* r = &out[(size_t)i * MPH_KIN_CHANNELS];
        CHECK(r[MPH_KIN_COUNT] >= 1.0 && r[MPH_KIN_FLAGS] == 3.0);
        for (int c = MPH_KIN_L; c < MPH_KIN_FLAGS; ++c) CHECK(r[c] == 0.0);
    }
    int good = 0;
    for (int i = 0; i < block; ++i) {
        const double* r = &out[(size_t)i * MPH_KIN_CHANNELS];
        CHECK(r[MPH_KIN_COUNT] >= 3.0 && std::isfinite(r[MPH_KIN_SHEAR]) && r[MPH_KIN_RESERVED0] == 0.0);
        good += ((int)r[MPH_KIN_FLAGS] & 1) == 0;
    }
    CHECK(good > block / 2);
    // the class mask, every radius rule, the other members
    k.classes = 4;
    CHECK(mph_kinematics_arrays(&cfg, &k, n, prop.data(), pos.data(), vel.data(), out.data()) == MPH_OK);
    k.classes = 8;
    CHECK(mph_kinematics_arrays(&cfg, &k, n, prop.data(), pos.data(), vel.data(), out.data()) == MPH_ERR_ARG);
    k.classes = 0;
    k.radius = 2.5 * dx;
    CHECK(mph_kinematics_arrays(&cfg, &k, n, prop.data(), pos.data(), vel.data(), out.data()) == MPH_OK);
    k.radius = 2.6 * dx;
    CHECK(mph_kinematics_arrays(&cfg, &k, n, prop.data(), pos.data(), vel.data(), out.data()) == MPH_ERR_ARG);
    k.radius = -dx;
    CHECK(mph_kinematics_arrays(&cfg, &k, n, prop.data(), pos.data(), vel.data(), out.data()) == MPH_ERR_ARG);
    k.radius = 0.0;
    k.reserved = 1;
    CHECK(mph_kinematics_arrays(&cfg, &k, n, prop.data(), pos.data(), vel.data(), out.data()) == MPH_ERR_ARG);
    k.reserved = 0;
    CHECK(mph_kinematics_arrays(&cfg, &k, 0, nullptr, nullptr, nullptr, nullptr) == MPH_OK);
    CHECK(mph_kinematics_arrays(&cfg, &k, 65537, prop.data(), pos.data(), vel.data(), out.data()) == MPH_ERR_ARG);
    double n0 = 0.0;
    CHECK(mph_kinematics_n0(&cfg, 0.0, &n0) == MPH_OK && n0 > 1.0);
    CHECK(mph_kinematics_n0(&cfg, -1.0, &n0) == MPH_ERR_ARG && mph_kinematics_n0(&cfg, 0.0, nullptr) == MPH_ERR_ARG);
    CHECK(mph_kinematics_arrays(&cfg, &k, n, prop.data(), pos.data(), vel.data(), out.data()) == MPH_OK);
    CHECK(mph_write_vtu_kinematics_arrays(vtu, n, prop.data(), pos.data(), out.data()) == MPH_OK);
    CHECK(mph_write_vtu_kinematics_arrays(vtu, 0, nullptr, nullptr, nullptr) == MPH_OK);
    CHECK(mph_write_vtu_kinematics_arrays(nullptr, n, prop.data(), pos.data(), out.data()) == MPH_ERR_ARG);
    std::printf("dim %d: n %d, %d of the block's %d with a gradient, n0 %.17g\n", dim, n, good, block, n0);
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    int lay[6];
    CHECK(mph_kinematics_layout(lay) == MPH_OK && lay[0] == (int)sizeof(MphKinematics) && lay[5] == 28);
    MphKinematics k;
    CHECK(mph_kinematics_parse("radius=0.002;classes=3;beta=0.9;det=1e-5;", &k) == MPH_OK && k.classes == 3);
    for (const char* bad : {"radius", "=1", "radius=1;radius=2", "classes=9", "beta=x", "det=1e-5,2", ";;radius=;"})
        CHECK(mph_kinematics_parse(bad, &k) == MPH_ERR_ARG);
    CHECK(mph_kinematics_parse(nullptr, &k) == MPH_ERR_ARG && mph_kinematics_parse("", nullptr) == MPH_ERR_ARG);
    run(2, (dir + "/k2.vtu").c_str());
    run(3, (dir + "/k3.vtu").c_str());
    std::printf(g_bad ? "kin_asan: %d checks failed\n" : "kin_asan: ok\n", g_bad);
    return g_bad ? 1 : 0;
}
