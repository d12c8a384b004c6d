// mask_rows.h -- rows of v mask bytes read and written 16 bytes at a time, shared by the per-vertex mask stages: segments.hip (sv_count_kernel
// reads), mask_nms.hip (mn_pack_kernel reads, mn_apply_kernel writes) and components.hip, whose kernels also take the wave walk below
// (mc_init_kernel, hf_box_kernel and hf_init_kernel read, mc_apply_kernel and hf_apply_kernel write).
//
// THE ADDRESS WALK.  v is arbitrary, so a row p = base + row * v starts at an arbitrary address and a vector grid laid over the row's
// VERTICES would be misaligned in most rows.  The grid is laid over the row's ADDRESS instead: with a0 = address of p modulo 16
// (mask_row_a0), chunk q covers the vertices [16 q - a0, 16 q - a0 + 16), so that p + i0 is 16-byte aligned for the first vertex i0 of every
// chunk, whatever v is.  A chunk that lies wholly inside [0, v) is ONE aligned 16-byte access; the chunks at the two ragged ends (i0 < 0 at
// the head, i0 + 16 > v at the tail; a short row has one chunk that is both) go byte by byte, and no byte outside [0, v) is ever read or
// written.  mask_row_chunks(v) chunks cover the row for every a0.  A kernel may start its walk anywhere in the row: mn_pack_kernel takes
// a0 of p + vb, the first vertex of its block, and the helpers take i0, not a chunk number.
//
// A chunk travels as 16 bits, bit k = "byte i0 + k is set" (any nonzero byte is set; a written byte is 0 or 1); the bits of vertices
// outside [0, v) are zero when read and ignored when written.  No LDS, no barrier; every function is inlined.
//
// THE WAVE WALK.  The 64 chunks of a wave are 1024 consecutive vertices.  A lane that went through its own 16 would touch every per-vertex
// array (parent, size, xyz) with 64 bytes between one lane's dword and the next: 454 us for mc_init_kernel's stores and 135 us for
// mc_apply_kernel's loads at 100 x 500 000, measured.  So in pass t of 16 the wave takes the 64 consecutive vertices 64 t .. 64 t + 63 of
// its chunks, lane l vertex 64 t + l, which is bit l % 16 of the chunk of lane 4 t + l / 16.  Shuffles and ballots carry the bits, so
// EVERY lane of the wave must reach every pass: between mask_row_load and the walk only a return that is uniform over the wave.
#pragma once
#include "common.h"

#define MASK_ROW_VEC 16                  // bytes per aligned vector

// the chunks that cover a row of v bytes whatever its misalignment: ceil((v + a0) / 16) for the largest a0
static inline int mask_row_chunks(int v) { return (v + 2 * (MASK_ROW_VEC - 1)) / MASK_ROW_VEC; }

__device__ __forceinline__ int mask_row_a0(const void* p) { return (int)(reinterpret_cast<uintptr_t>(p) & (MASK_ROW_VEC - 1)); }

// the 4 bits "byte k of x is not zero", bit k for byte k
__device__ __forceinline__ unsigned mask_row_nibble(unsigned x) {
    const unsigned y = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;      // the top bit of every nonzero byte
    return (((y >> 7) * 0x01020408u) >> 24) & 0xFu;                                  // no two partial products share a bit: no carries
}
// 4 bits -> 4 bytes of 0 or 1
__device__ __forceinline__ unsigned mask_row_spread(unsigned n) { return (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21); }

// The 16 bits of the chunk that starts at vertex i0 of row p; p + i0 is 16-byte aligned, i0 >= -15.  0 for a chunk at or beyond v.
__device__ __forceinline__ unsigned mask_row_load(const unsigned char* p, int i0, int v) {
    unsigned bits = 0u;
    if (i0 >= 0 && i0 + MASK_ROW_VEC <= v) {
        const uint4 x = *reinterpret_cast<const uint4*>(p + i0);
        bits = mask_row_nibble(x.x) | (mask_row_nibble(x.y) << 4) | (mask_row_nibble(x.z) << 8) | (mask_row_nibble(x.w) << 12);
    } else if (i0 < v) {                                             // a ragged end
        for (int k = 0; k < MASK_ROW_VEC; ++k) {
            const int i = i0 + k;
            if (i >= 0 && i < v && p[i] != 0) bits |= 1u << k;
        }
    }
    return bits;
}

// Writes the chunk that starts at vertex i0 of row p as bytes of 0 and 1; p + i0 is 16-byte aligned, i0 >= -15.  Nothing for a chunk at
// or beyond v.
__device__ __forceinline__ void mask_row_store(unsigned char* p, int i0, int v, unsigned bits) {
    if (i0 >= 0 && i0 + MASK_ROW_VEC <= v) {
        uint4 o;
        o.x = mask_row_spread(bits);
        o.y = mask_row_spread(bits >> 4);
        o.z = mask_row_spread(bits >> 8);
        o.w = mask_row_spread(bits >> 12);
        *reinterpret_cast<uint4*>(p + i0) = o;
    } else if (i0 < v) {                                             // a ragged end
        for (int k = 0; k < MASK_ROW_VEC; ++k) {
            const int i = i0 + k;
            if (i >= 0 && i < v) p[i] = (unsigned char)((bits >> k) & 1u);
        }
    }
}

// the vertex of this lane in pass t of the wave walk, i0 being the first vertex of the lane's own chunk; it may lie outside [0, v)
__device__ __forceinline__ int mask_wave_vertex(int i0, int t) { return i0 - lane_id() * MASK_ROW_VEC + GSPN_WAVE * t + lane_id(); }

// The wave walk, reading: body(i, set) for every vertex i in [0, v) of the wave's chunks, set being its bit; bits is what mask_row_load
// gave this lane for its chunk at i0.
template <class Body>
__device__ __forceinline__ void mask_wave_read(unsigned bits, int i0, int v, Body body) {
    const int lane = lane_id();
#pragma unroll
    for (int t = 0; t < MASK_ROW_VEC; ++t) {
        const unsigned theirs = (unsigned)__shfl((int)bits, 4 * t + (lane >> 4), GSPN_WAVE);
        const int i = mask_wave_vertex(i0, t);
        if (i >= 0 && i < v) body(i, ((theirs >> (lane & 15)) & 1u) != 0u);
    }
}

// The wave walk, writing, pass t: on is the bit of mask_wave_vertex(i0, t), false outside [0, v).  The ballot holds the bits of four chunks
// and the lane whose chunk is among them keeps its 16: after the 16 passes bits is the lane's chunk, for mask_row_store.  (The pass loop
// is the kernel's: with a lambda for a body that also counts, the apply kernels compile to other code, profiles/components_fold.txt.)
__device__ __forceinline__ void mask_wave_write(bool on, int t, unsigned& bits) {
    const unsigned long long word = __ballot(on);
    if ((lane_id() >> 2) == t) bits = (unsigned)(word >> (16 * (lane_id() & 3))) & 0xFFFFu;
}
