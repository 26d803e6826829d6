// list16_check.cpp -- the host-callable helpers of the 16-bit list rows (csrc/mph_params.h: entry16*,
// soff_*, row_group, GroupCursor; csrc/mph_rows.h: HostRows::entry) against plain models.  A stand-
// alone program built by tests/test_list16_format.py with -fsanitize=address,undefined; needs no GPU.
#include <cstdio>
#include <vector>

#include "../../particlemethod_fsi_amd/csrc/mph_rows.h"

using namespace mph;

namespace {

int failures = 0;

void fail(const char* what, long long a, long long b, long long c)
{
    if (++failures <= 20) std::printf("FAIL %s (%lld, %lld, %lld)\n", what, a, b, c);
}

// encode / decode over the whole offset range and every type the 3 bits hold
void check_entries()
{
    for (int t = 0; t < (1 << (16 - kOff16Bits)); ++t)
        for (int off = 0; off <= kOff16Mask; ++off) {
            const unsigned e = entry16(off, t);
            if (e > 0xffffu) fail("entry past 16 bits", off, t, e);
            const unsigned short stored = (unsigned short)e;
            if (entry16_off(stored) != off || entry16_type(stored) != t) fail("round trip", off, t, stored);
            // the search forms the entry as j | type << 13 in 32 bits and stores its low half
            if ((unsigned short)(off | (t << kOff16Bits)) != stored) fail("search's form", off, t, stored);
        }
    static_assert(MPH_TYPE_COUNT <= 8, "3 type bits");
    static_assert(kList16Span <= kOff16Mask, "a span's offsets fit the offset bits");
}

// the store counter of both formats against row * row bytes + lane * entry bytes
void check_store_offsets()
{
    for (int s16 = 0; s16 < 2; ++s16) {
        const int eb = s16 ? 2 : 4, rb = 64 * eb;
        for (int lane = 0; lane < 64; ++lane) {
            int soff = soff_first(s16, lane);
            int total = 0;
            for (int row = 0; row < 640; ++row) {
                if ((soff & kSoffMask) != row * rb + lane * eb) fail("store offset", s16, row, lane);
                if (soff_stored(s16, soff) != row) fail("stored rows", s16, row, lane);
                if (soff_total(soff) != total) fail("total", s16, row, lane);
                // every third neighbour is counted without being stored (the shell past the list radius)
                if (row % 3 == 0) {
                    soff += kListTotal;
                    ++total;
                    if ((soff & kSoffMask) != row * rb + lane * eb) fail("store offset after a count", s16, row, lane);
                }
                soff += soff_keep(s16);
                ++total;
            }
            // a row jump: the lane moves from its row to the wave's (group_end)
            for (int row = 0; row < kAlignRows; row += 7)
                for (int m = row; m < kAlignRows; m += 13) {
                    int so = soff_first(s16, lane) + row * soff_keep(s16);
                    so += (m - row) << soff_row_shift(s16);
                    if ((so & kSoffMask) != m * rb + lane * eb || soff_stored(s16, so) != m || soff_total(so) != row)
                        fail("jump", s16, row, m);
                }
        }
        // the last row a lane that keeps 512 entries behind kAlignRows of gaps can reach does not
        // carry into the total
        const int top = soff_first(s16, 63) + (kTileRows - 1) * soff_keep(s16);
        if (soff_stored(s16, top) != kTileRows - 1 || soff_total(top) != kTileRows - 1) fail("top row", s16, top, 0);
    }
}

unsigned long long header(const int (&starts)[kMaxJumps], unsigned flags)
{
    unsigned long long h = (unsigned long long)(kMaxJumps | flags) << 56;
    for (int g = 0; g < kMaxJumps; ++g) h |= (unsigned long long)starts[g] << (8 * g);
    return h;
}

// the group of row k: row_group and the ascending cursor against a linear search over the group starts
void check_groups()
{
    const int cases[][kMaxJumps] = {
        {9, 20, 33, 47, 60, 70},      // seven groups, none empty
        {0, 0, 12, 12, 12, 40},       // empty groups at the start and in the middle
        {5, 5, 5, 5, 5, 5},           // all but the first and the last empty
        {0, 0, 0, 0, 0, 0},           // every entry in the last group
        {127, 127, 127, 127, 127, 127},
        {1, 2, 3, 4, 5, 6},
        {10, 30, 30, 64, 100, 127},
    };
    for (const auto& st : cases) {
        const unsigned long long h = header(st, kHdrShort | kHdrNoGap);
        if (!hdr_short(h) || jump_count(h) != kMaxJumps || gap_count(h) != 0) fail("header flags", 0, 0, 0);
        if (gap_count(header(st, kHdrShort)) != kMaxJumps) fail("gap count", 0, 0, 0);
        GroupCursor c;
        c.init(h);
        int prev = 0;
        for (int k = 0; k < kTileRows; ++k) {
            int g = 0;   // the model: the last group whose first row is at or below k
            for (int q = 0; q < kMaxJumps; ++q)
                if (k >= st[q]) g = q + 1;
            if (row_group(h, k) != g) fail("row_group", k, g, row_group(h, k));
            const bool moved = c.seek(h, k);
            if (c.g != g || moved != (g != prev)) fail("cursor", k, g, c.g);
            prev = g;
        }
    }
}

// HostRows::entry on a hand-made short wave and a wide one
void check_host_entry()
{
    HostRows R;
    const int starts[kMaxJumps] = {2, 2, 5, 6, 6, 9};
    R.hdr = {header(starts, kHdrShort | kHdrNoGap), 0ull};
    R.base.assign(2 * kBaseInts, 0);
    for (int g = 0; g < 7; ++g) R.base[g] = 1000 * (g + 1);
    R.rows.assign(2 * kTile, 12);
    R.gap.assign(2 * kTile, 0);
    std::vector<int> tile(kTile * kTileRows, 0);
    unsigned short* t16 = reinterpret_cast<unsigned short*>(tile.data());
    for (int r = 0; r < 12; ++r)
        for (int lane = 0; lane < kTile; ++lane) t16[ell_slot(r, lane)] = (unsigned short)entry16(r * 64 + lane, (r + lane) % 6);
    for (int r = 0; r < 12; ++r)
        for (int lane = 0; lane < kTile; ++lane) {
            int type = -1;
            const int j = R.entry(lane, r, tile.data(), &type);
            if (j != r * 64 + lane + 1000 * (row_group(R.hdr[0], r) + 1) || type != (r + lane) % 6) fail("short entry", r, lane, j);
        }
    for (int r = 0; r < 12; ++r)
        for (int lane = 0; lane < kTile; ++lane) tile[ell_slot(r, lane)] = (123456 + r * 64 + lane) | ((lane % 6) << kTypeShift);
    for (int r = 0; r < 12; ++r)
        for (int lane = 0; lane < kTile; ++lane) {
            int type = -1;
            const int j = R.entry(kTile + lane, r, tile.data(), &type);
            if (j != 123456 + r * 64 + lane || type != lane % 6) fail("wide entry", r, lane, j);
        }
}

// a short wave's gap words: the jumps before its first real gap carry the empty gap [255, header byte)
void check_empty_gaps()
{
    HostRows R;
    const int starts[kMaxJumps] = {4, 9, 9, 15, 20, 26};
    R.hdr = {header(starts, kHdrShort)};   // (gaps: no kHdrNoGap)
    R.rows.assign(kTile, 30);
    R.gap.assign(kTile, 0);
    R.base.assign(kBaseInts, 0);
    for (int lane = 0; lane < kTile; ++lane) {
        // first real gap at jump 3: lanes' rows 12 + lane % 4 against the wave's 15; then agreeing jumps
        unsigned long long g = 0xffffffull | ((unsigned long long)(12 + lane % 4) << 24);
        g |= (unsigned long long)20 << 32 | (unsigned long long)26 << 40;
        R.gap[lane] = g;
        const int gap = 15 - (12 + lane % 4);
        if (R.entries(lane) != 30 - gap) fail("entries with empty gaps", lane, R.entries(lane), 30 - gap);
        for (int r = 0; r < 32; ++r) {
            const bool held = r < 30 && !(r >= 12 + lane % 4 && r < 15);
            if (R.ok(lane, r) != held) fail("ok with empty gaps", lane, r, held);
        }
    }
}

}  // namespace

int main()
{
    check_entries();
    check_store_offsets();
    check_groups();
    check_host_entry();
    check_empty_gaps();
    if (failures) {
        std::printf("list16_check: %d failures\n", failures);
        return 1;
    }
    std::printf("list16_check ok\n");
    return 0;
}
