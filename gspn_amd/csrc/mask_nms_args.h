// mask_nms_args.h -- the host side of mask_nms.hip that needs no device: the argument checks the two launchers run before anything is
// launched, and the layout of their workspaces.  Plain C++, no HIP header: tools/mask_nms_args_check.cpp compiles it on its own.
#pragma once
#include "stage_args.h"

#define MN_MAX_R 1024                    // scene_rank's limit; the (r, r) overlap matrix of one scene is then 4 MB
#define MN_MAX_V (1 << 24)
#define MN_MAX_B 65535                   // the scenes are a grid dimension

// overlaps: unsigned long long packed[b][r][words].  NMS: the same, then, each 16-byte aligned, int sizes[b][r] and int inter[b][r][r]
struct MnLayout { size_t packed, sizes, inter, bytes; int words; };
static inline MnLayout mn_layout(int b, int r, int v, bool nms) {
    MnLayout l;
    l.words = (int)(((long)v + 63) / 64);
    l.packed = 0;
    l.sizes = stage_up16(sizeof(unsigned long long) * (size_t)b * (size_t)r * (size_t)l.words);
    l.inter = stage_up16(l.sizes + sizeof(int) * (size_t)b * (size_t)r);
    l.bytes = nms ? l.inter + sizeof(int) * (size_t)b * (size_t)r * (size_t)r : l.sizes;
    return l;
}

// the sizes alone: 0, GSPN_ERR_ARG or GSPN_ERR_UNSUPPORTED
static inline int mn_check_sizes(int b, int r, int v) {
    if (b < 0 || r < 0 || v < 0) return GSPN_ERR_ARG;
    if (r > MN_MAX_R || v > MN_MAX_V || b > MN_MAX_B) return GSPN_ERR_UNSUPPORTED;
    return 0;
}

// every decline of gspn_mask_overlaps, in stage_check's order
static inline int mo_check(int b, int r, int v, const void* masks, const void* ws, const void* sizes, const void* inter) {
    return stage_check(stage_any_null(masks, ws, sizes, inter), mn_check_sizes(b, r, v), ws);
}
// every decline of gspn_mask_nms; labels may be null
static inline int mn_check(int b, int r, int v, const void* masks, const void* count, double iou_th, const void* ws, const void* out,
                           const void* keep, const void* mask_points) {
    const bool th_ok = iou_th >= 0.0 && iou_th < 1.0;                        // a NaN fails both compares
    return stage_check(stage_any_null(masks, count, ws, out, keep, mask_points) || !th_ok, mn_check_sizes(b, r, v), ws);
}

static inline long mo_ws_bytes(int b, int r, int v) {
    return stage_ws_bytes(mn_check_sizes(b, r, v), b == 0 || r == 0 || v == 0, [&] { return mn_layout(b, r, v, false); });
}
static inline long mn_ws_bytes(int b, int r, int v) {
    return stage_ws_bytes(mn_check_sizes(b, r, v), b == 0 || r == 0 || v == 0, [&] { return mn_layout(b, r, v, true); });
}
