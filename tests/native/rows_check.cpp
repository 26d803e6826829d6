// rows_check.cpp -- HostRows (csrc/mph_rows.h), the host reader of the neighbour lists' row jumps,
// against a brute-force model on hand-made waves.  Built with -fsanitize=address,undefined and run
// by tests/test_native_asan.py; needs no GPU.
#include <cstdio>
#include <vector>

#include "../../particlemethod_fsi_amd/csrc/mph_rows.h"

using namespace mph;

namespace {

struct Gap { int a, b; };   // rows [a, b)

int failures = 0;

// One wave: its jumps' destination rows (the gaps' ends, shared by the lanes) and, per lane, the
// gaps' starts and the lane's rows.
struct Wave {
    std::vector<int> ends;
    std::vector<std::vector<int>> starts;   // [lane][jump]
    std::vector<int> rows;                  // [lane]
};

void check(const char* name, const Wave& w)
{
    const int lanes = (int)w.rows.size(), J = (int)w.ends.size();
    HostRows R;
    R.rows = w.rows;
    R.hdr.assign(1, (unsigned long long)J << 56);
    for (int k = 0; k < J; ++k) R.hdr[0] |= (unsigned long long)w.ends[k] << (8 * k);
    R.gap.assign(kTile, 0);
    for (int s = 0; s < lanes; ++s)
        for (int k = 0; k < J; ++k) R.gap[s] |= (unsigned long long)w.starts[s][k] << (8 * k);
    for (int s = 0; s < lanes; ++s) {
        // the model: mark the rows [0, rows), then clear each gap
        std::vector<char> held(kTileRows + 64, 0);
        for (int r = 0; r < w.rows[s] && r < (int)held.size(); ++r) held[r] = 1;
        for (int k = 0; k < J; ++k)
            for (int r = w.starts[s][k]; r < w.ends[k]; ++r) held[r] = 0;
        int entries = 0;
        for (int r = 0; r < kTileRows; ++r) entries += held[r];   // a tile holds kTileRows rows
        for (int r = 0; r < (int)held.size(); ++r)
            if (R.ok(s, r) != (held[r] != 0)) {
                std::printf("%s: lane %d row %d: ok = %d, model %d\n", name, s, r, (int)R.ok(s, r), (int)held[r]);
                ++failures;
            }
        if (R.entries(s) != entries) {
            std::printf("%s: lane %d: entries = %d, model %d\n", name, s, R.entries(s), entries);
            ++failures;
        }
    }
}

}  // namespace

int main()
{
    static_assert(kAlignRows == 128 && kMaxJumps == 6, "the waves below are made for these");
    check("no jump", {{}, {{}, {}, {}}, {0, 7, 200}});
    check("one empty gap", {{9}, {{9}, {4}}, {12, 12}});
    check("gap ending at kAlignRows", {{kAlignRows}, {{100}, {127}, {128}}, {kAlignRows, 140, kAlignRows + 1}});
    // kMaxJumps gaps; lane 1 ends below its last gap's start, lane 2 inside a gap
    check("kMaxJumps gaps", {{10, 25, 40, 60, 90, 120},
                             {{8, 20, 33, 50, 70, 100}, {10, 25, 40, 60, 90, 110}, {3, 12, 30, 45, 61, 95}},
                             {130, 100, 50}});
    check("rows = 0", {{16, 32}, {{5, 20}, {16, 32}}, {0, 0}});
    check("rows above kTileRows", {{64}, {{40}, {64}}, {kTileRows + 5, kTileRows + 1}});
    if (failures) return 1;
    std::printf("rows_check ok\n");
    return 0;
}
