// stage_args.h -- what the host sides of the mask stages (segments_args.h, mask_nms_args.h, components_args.h) share: the parts of a workspace
// start at multiples of 16 bytes, and every launcher declines in one order.  Plain C++, no HIP header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gspn_hip.h"

// a workspace offset rounded up to 16 bytes
static inline size_t stage_up16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

static inline bool stage_ws_aligned(const void* ws) { return (reinterpret_cast<uintptr_t>(ws) & 15) == 0; }

template <class... P>
static inline bool stage_any_null(const P*... p) { return (... || !p); }

// Every decline of a launcher: an argument error (a null pointer, a parameter outside its range, a negative size: the last is sizes_rc's
// GSPN_ERR_ARG) goes first, then a size beyond a limit, then a ws that is not 16-byte aligned.
static inline int stage_check(bool bad_argument, int sizes_rc, const void* ws) {
    if (bad_argument || sizes_rc == GSPN_ERR_ARG) return GSPN_ERR_ARG;
    if (sizes_rc != 0) return sizes_rc;
    return stage_ws_aligned(ws) ? 0 : GSPN_ERR_UNSUPPORTED;
}

// The bytes of a workspace: 0 for sizes the launcher declines and for a call with nothing to do; the layout is not computed for them (it
// multiplies without looking).
template <class Layout>
static inline long stage_ws_bytes(int sizes_rc, bool empty, Layout layout) { return sizes_rc != 0 || empty ? 0 : (long)layout().bytes; }
