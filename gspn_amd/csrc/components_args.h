// components_args.h -- the host side of components.hip that needs no device: the argument checks the two launchers run before anything is
// launched, and the layout of their workspaces.  Plain C++, no HIP header: tools/components_args_check.cpp compiles it on its own.
#pragma once
#include "stage_args.h"

#define MC_MAX_R 1024                    // scene_rank's limit: 16 words of the vertex-major table per vertex
#define MC_MAX_V (1 << 24)
#define MC_MAX_F (1 << 26)

// components: unsigned long long table[v][words], then, each 16-byte aligned, int size[r][v] and int bad[r].  The filter: the same, then
// int parent[r][v] and int largest[r] -- what gspn_mask_components writes to its caller's comp and largest
struct McLayout { size_t table, size, bad, parent, largest, bytes; int words; };
static inline McLayout mc_layout(int r, int v, bool filter) {
    const size_t cells = sizeof(int) * (size_t)r * (size_t)v, rows = sizeof(int) * (size_t)r;
    McLayout l;
    l.words = (r + 63) / 64;
    l.table = 0;
    l.size = stage_up16(sizeof(unsigned long long) * (size_t)v * (size_t)l.words);
    l.bad = stage_up16(l.size + cells);
    l.parent = stage_up16(l.bad + rows);
    l.largest = stage_up16(l.parent + cells);
    l.bytes = filter ? l.largest + rows : l.bad + rows;
    return l;
}

// the sizes alone: 0, GSPN_ERR_ARG or GSPN_ERR_UNSUPPORTED
static inline int mc_check_sizes(int r, int v, int f) {
    if (r < 0 || v < 0 || f < 0) return GSPN_ERR_ARG;
    if (r > MC_MAX_R || v > MC_MAX_V || f > MC_MAX_F) return GSPN_ERR_UNSUPPORTED;
    return 0;
}

// every decline of gspn_mask_components, in stage_check's order; faces may be null when there are none
static inline int mc_check(int r, int v, int f, const void* masks, const void* faces, const void* ws, const void* comp, const void* ncomp,
                           const void* largest) {
    return stage_check(stage_any_null(masks, ws, comp, ncomp, largest) || (!faces && f > 0), mc_check_sizes(r, v, f), ws);
}
// every decline of gspn_mask_component_filter
static inline int mf_check(int r, int v, int f, const void* masks, const void* faces, int min_vertices, double min_share, const void* ws,
                           const void* out, const void* mask_points, const void* ncomp, const void* nkept) {
    const bool parameters_ok = min_vertices >= 1 && min_share >= 0.0 && min_share <= 1.0;      // a NaN fails both compares
    return stage_check(stage_any_null(masks, ws, out, mask_points, ncomp, nkept) || (!faces && f > 0) || !parameters_ok, mc_check_sizes(r, v, f), ws);
}

static inline long mc_ws_bytes(int r, int v, int f) {
    return stage_ws_bytes(mc_check_sizes(r, v, f), r == 0 || v == 0, [&] { return mc_layout(r, v, false); });
}
static inline long mf_ws_bytes(int r, int v, int f) {
    return stage_ws_bytes(mc_check_sizes(r, v, f), r == 0 || v == 0, [&] { return mc_layout(r, v, true); });
}
