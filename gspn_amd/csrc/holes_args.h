// holes_args.h -- the host side of gspn_mask_hole_fill (components.hip) that needs no device: the argument checks the launcher runs before
// anything is launched, and the layout of its workspace.  Plain C++, no HIP header: tools/holes_args_check.cpp compiles it on its own.
#pragma once
#include "components_args.h"

// unsigned long long cand[v][words], then, each 16-byte aligned, unsigned long long set[v][words], int size[r][v] (the two high bits below
// the sign are the flags of a root), int bad[r], int box[r][6] (the keys of lo x, y, z and hi x, y, z), int points_in[r] and int parent[r][v].
// The parents are part of the workspace whether the caller brings a label or not: the size does not depend on a pointer.
struct HfLayout { size_t cand, set, size, bad, box, points, parent, bytes; int words; };
static inline HfLayout hf_layout(int r, int v) {
    const size_t cells = sizeof(int) * (size_t)r * (size_t)v, rows = sizeof(int) * (size_t)r;
    const size_t table = sizeof(unsigned long long) * (size_t)v * (size_t)((r + 63) / 64);
    HfLayout l;
    l.words = (r + 63) / 64;
    l.cand = 0;
    l.set = stage_up16(table);
    l.size = stage_up16(l.set + table);
    l.bad = stage_up16(l.size + cells);
    l.box = stage_up16(l.bad + rows);
    l.points = stage_up16(l.box + 6 * rows);
    l.parent = stage_up16(l.points + rows);
    l.bytes = l.parent + cells;
    return l;
}

// every decline of gspn_mask_hole_fill, in stage_check's order; faces may be null when there are none, label may always be null
static inline int hf_check(int r, int v, int f, const void* masks, const void* faces, const void* xyz, int max_vertices, double max_share,
                           const void* ws, const void* out, const void* mask_points, const void* nholes, const void* nfilled) {
    const bool parameters_ok = max_vertices >= 0 && max_share >= 0.0 && max_share <= 1.0;      // a NaN fails both compares
    return stage_check(stage_any_null(masks, xyz, ws, out, mask_points, nholes, nfilled) || (!faces && f > 0) || !parameters_ok,
                       mc_check_sizes(r, v, f), ws);
}

static inline long hf_ws_bytes(int r, int v, int f) {
    return stage_ws_bytes(mc_check_sizes(r, v, f), r == 0 || v == 0, [&] { return hf_layout(r, v); });
}
