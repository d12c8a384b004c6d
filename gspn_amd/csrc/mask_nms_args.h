// mask_nms_args.h -- the host side of mask_nms.hip that needs no device: the argument checks the two launchers run before anything is
// launched, and the layout of their workspaces.  Plain C++, no HIP header: tools/mask_nms_args_check.cpp compiles it on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gspn_hip.h"

#define MN_MAX_R 1024                    // scene_rank's limit; the (r, r) overlap matrix of one scene is then 4 MB
#define MN_MAX_V (1 << 24)
#define MN_MAX_B 65535                   // the scenes are a grid dimension

// overlaps: unsigned long long packed[b][r][words].  NMS: the same, then, each 16-byte aligned, int sizes[b][r] and int inter[b][r][r]
struct MnLayout { size_t packed, sizes, inter, bytes; int words; };
static inline MnLayout mn_layout(int b, int r, int v, bool nms) {
    MnLayout l;
    l.words = (int)(((long)v + 63) / 64);
    l.packed = 0;
    l.sizes = sizeof(unsigned long long) * (size_t)b * (size_t)r * (size_t)l.words;        // a multiple of 8
    l.sizes = (l.sizes + 15) & ~(size_t)15;
    l.inter = (l.sizes + sizeof(int) * (size_t)b * (size_t)r + 15) & ~(size_t)15;
    l.bytes = nms ? l.inter + sizeof(int) * (size_t)b * (size_t)r * (size_t)r : l.sizes;
    return l;
}

// the sizes alone: 0, GSPN_ERR_ARG or GSPN_ERR_UNSUPPORTED
static inline int mn_check_sizes(int b, int r, int v) {
    if (b < 0 || r < 0 || v < 0) return GSPN_ERR_ARG;
    if (r > MN_MAX_R || v > MN_MAX_V || b > MN_MAX_B) return GSPN_ERR_UNSUPPORTED;
    return 0;
}

// every decline of gspn_mask_overlaps, argument errors first
static inline int mo_check(int b, int r, int v, const void* masks, const void* ws, const void* sizes, const void* inter) {
    if (b < 0 || r < 0 || v < 0 || !masks || !ws || !sizes || !inter) return GSPN_ERR_ARG;
    const int rc = mn_check_sizes(b, r, v);
    if (rc != 0) return rc;
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return GSPN_ERR_UNSUPPORTED;
    return 0;
}
// every decline of gspn_mask_nms; labels may be null
static inline int mn_check(int b, int r, int v, const void* masks, const void* count, double iou_th, const void* ws, const void* out,
                           const void* keep, const void* mask_points) {
    if (b < 0 || r < 0 || v < 0 || !masks || !count || !ws || !out || !keep || !mask_points) return GSPN_ERR_ARG;
    if (!(iou_th >= 0.0 && iou_th < 1.0)) return GSPN_ERR_ARG;               // a NaN fails both compares
    const int rc = mn_check_sizes(b, r, v);
    if (rc != 0) return rc;
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return GSPN_ERR_UNSUPPORTED;
    return 0;
}

static inline long mo_ws_bytes(int b, int r, int v) {
    if (mn_check_sizes(b, r, v) != 0 || b == 0 || r == 0 || v == 0) return 0;
    return (long)mn_layout(b, r, v, false).bytes;
}
static inline long mn_ws_bytes(int b, int r, int v) {
    if (mn_check_sizes(b, r, v) != 0 || b == 0 || r == 0 || v == 0) return 0;
    return (long)mn_layout(b, r, v, true).bytes;
}
