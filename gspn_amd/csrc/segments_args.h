// segments_args.h -- the host side of segments.hip that needs no device: the argument checks the two launchers run before anything is
// launched, and the layout of their workspaces.  Plain C++, no HIP header: tools/segments_args_check.cpp compiles it on its own.
#pragma once
#include "stage_args.h"

#define SV_MAX_V (1 << 24)
#define SV_MAX_S (1 << 24)
#define SV_MAX_R 65535
#define SV_MAX_COUNTERS (1L << 28)       // int32 counters of one call: 1 GiB

// mask vote: int cnt[r + 1][s] (row r: the sizes), then, 16-byte aligned, unsigned long long bits[r][words]
struct SvLayout { size_t cnt, bits, bytes; int words; };
static inline SvLayout sv_layout(int r, int v, int s) {
    (void)v;
    SvLayout l;
    l.words = (s + 63) / 64;
    l.cnt = 0;
    l.bits = stage_up16(sizeof(int) * ((size_t)r + 1) * (size_t)s);
    l.bytes = l.bits + sizeof(unsigned long long) * (size_t)r * (size_t)l.words;
    return l;
}
// label vote: int cnt[s][c], then int win[s]
struct SlLayout { size_t cnt, win, bytes; };
static inline SlLayout sl_layout(int v, int s, int c) {
    (void)v;
    SlLayout l;
    l.cnt = 0;
    l.win = sizeof(int) * (size_t)s * (size_t)c;
    l.bytes = l.win + sizeof(int) * (size_t)s;
    return l;
}

// the sizes alone: 0, GSPN_ERR_ARG or GSPN_ERR_UNSUPPORTED
static inline int sv_check_sizes(int r, int v, int s) {
    if (r < 0 || v < 0 || s < 0) return GSPN_ERR_ARG;
    if (v > SV_MAX_V || r > SV_MAX_R || s > SV_MAX_S || ((long)r + 1) * (long)s > SV_MAX_COUNTERS) return GSPN_ERR_UNSUPPORTED;
    return 0;
}
static inline int sl_check_sizes(int v, int s, int c) {
    if (v < 0 || s < 0 || c < 1) return GSPN_ERR_ARG;
    if (v > SV_MAX_V || s > SV_MAX_S || (long)s * (long)c > SV_MAX_COUNTERS) return GSPN_ERR_UNSUPPORTED;
    return 0;
}

// every decline of gspn_segment_vote, in stage_check's order
static inline int sv_check(int r, int v, int s, const void* masks, const void* seg, double vote_th, const void* ws, const void* out,
                           const void* mask_points) {
    const bool th_ok = vote_th >= 0.0 && vote_th < 1.0;                      // a NaN fails both compares
    return stage_check(stage_any_null(masks, seg, ws, out, mask_points) || !th_ok, sv_check_sizes(r, v, s), ws);
}
static inline int sl_check(int v, int s, int c, const void* labels, const void* seg, const void* ws, const void* out) {
    return stage_check(stage_any_null(labels, seg, ws, out), sl_check_sizes(v, s, c), ws);
}

static inline long sv_ws_bytes(int r, int v, int s) {
    return stage_ws_bytes(sv_check_sizes(r, v, s), r == 0 || v == 0, [&] { return sv_layout(r, v, s); });
}
static inline long sl_ws_bytes(int v, int s, int c) {
    return stage_ws_bytes(sl_check_sizes(v, s, c), v == 0, [&] { return sl_layout(v, s, c); });
}
