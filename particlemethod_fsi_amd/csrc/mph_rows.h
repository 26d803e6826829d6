// mph_rows.h -- host view of the neighbour lists' rows (no HIP types: builds with plain g++).
#pragma once

#include <algorithm>
#include <vector>

#include "mph_params.h"

namespace mph {

// The lists' rows as the last search left them (mph_list.h RowMask): per particle (sorted
// order) its rows [0, rows[s]) and, per wave, the row jumps (jump_count / gap_begin / gap_end).
struct HostRows {
    std::vector<int> rows;
    std::vector<unsigned long long> hdr, gap;
    std::vector<int> base;   // kBaseInts per wave: the group bases of the waves with 16-bit rows
    // Entry of row r of particle s from its wave's tile as copied from the device (rows of 64 ints,
    // or of 64 uint16 in a short wave's): the neighbour's sorted index, its type in *type
    int entry(int s, int r, const int* tile, int* type = nullptr) const
    {
        const unsigned long long h = hdr[s >> 6];
        int j, t;
        if (hdr_short(h)) {
            const unsigned e = reinterpret_cast<const unsigned short*>(tile)[ell_slot(r, s & 63)];
            j = entry16_off(e) + base[(size_t)(s >> 6) * kBaseInts + row_group(h, r)];
            t = entry16_type(e);
        } else {
            const int e = tile[ell_slot(r, s & 63)];
            j = e & kIndexMask;
            t = (int)((unsigned)e >> kTypeShift);
        }
        if (type) *type = t;
        return j;
    }
    // whether row r of particle s holds one of its entries
    bool ok(int s, int r) const
    {
        const unsigned long long h = hdr[s >> 6];
        for (int k = 0; k < gap_count(h); ++k)
            if (r >= gap_begin(gap[s], k) && r < gap_end(h, k)) return false;
        return r < rows[s];
    }
    int entries(int s) const
    {
        const unsigned long long h = hdr[s >> 6];
        const int end = std::min(rows[s], kTileRows);
        // At a jump every lane's row counter moves on to the gap's end (scan_candidates_lds
        // group_end: soff += (m - row) << 8, in all lanes) and only grows after it, so the search
        // leaves rows[s] >= every gap end, and those are below kAlignRows < kTileRows: on its lists
        // the clamps change nothing.  Like the kernels' row_mask, a gap past the end takes nothing.
        int e = end;
        // (a short wave's jumps before its first real gap carry the empty gap [255, header byte))
        for (int k = 0; k < gap_count(h); ++k)
            if (gap_begin(gap[s], k) < gap_end(h, k)) e -= std::min(gap_end(h, k), end) - std::min(gap_begin(gap[s], k), end);
        return e;
    }
};

}  // namespace mph
