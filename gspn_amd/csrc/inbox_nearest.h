// inbox_nearest.h -- the tile that gspn_nearest_in_sets (detect.hip) and gspn_lift_masks (lift.hip) share: for the THREADS * QB points of
// a workgroup's tile that lie inside one box, the nearest of a set of p points, the first among equal distances (tf.argmin).  The inside
// test first; the inside points are compacted into LDS by wave ballot, so that a tile without one stages nothing.  The set sits in LDS as
// three planes and every lane walks them for QB compacted entries held in registers (one broadcast LDS read of four points serves 4 x QB
// distances).  A tile with few inside points -- the usual case, a detection holds about a hundredth of the cloud -- gives each entry to
// 2..64 lanes that split the set and meet by shuffles.
//
// Both users are pinned bit for bit to the reference, through what is written here once: the distance (dx*dx + dy*dy) + dz*dz, unfused
// (their translation units are compiled with -ffp-contract=off); strict <, so the smallest position wins among equal distances; the
// (distance, position) rule where lanes meet; NaN in the slots past p, which is smaller than nothing and never wins.
//
// The kernel declares the LDS and says what happens with the nearest position:
//   extern __shared__ __align__(16) float planes[];   [3][p4], p4 = p rounded up to 4
//   __shared__ int list[THREADS * QB];                the tile offsets of the inside points, ascending
//   __shared__ int wcnt[QB][THREADS / GSPN_WAVE];
// A tile offset is u * THREADS + tid for slot u of lane tid; the tile starts at point i0.
#pragma once
#include "box_common.h"

// Points per lane of a launch over `rows` (scene, box) pairs of n points each: four once that still gives every CU two workgroups, one
// per lane below (small clouds, few boxes).  gspn_amd/lift.py::lift_tile restates it.
template <int THREADS>
static inline int inbox_points_per_lane(long rows, int n) {
    return rows * ((n + THREADS * 4 - 1) / (THREADS * 4)) >= 512 ? 4 : 1;
}

// in[u]: slot u of this lane lies in the box (a slot past the end holds NaN, which is inside no box).  list[0 .. total): the tile offsets
// of the inside points in (u, wave, lane) order, which is ascending.  Returns total, uniform.  One barrier, which every lane reaches.
template <int THREADS, int QB>
__device__ __forceinline__ int inbox_compact(const float* pts, int i0, int n, const float (&lo)[3], const float (&hi)[3],
                                             bool (&in)[QB], int* list, int (*wcnt)[THREADS / GSPN_WAVE]) {
    const int tid = threadIdx.x, lane = tid % GSPN_WAVE, wave = tid / GSPN_WAVE;
    int before[QB];
#pragma unroll
    for (int u = 0; u < QB; ++u) {
        const int i = i0 + u * THREADS + tid;
        const float* g = pts + 3 * (long)min(i, n - 1);
        const float x = i < n ? g[0] : NAN, y = g[1], z = g[2];      // a slot past n holds NaN, which is inside no box
        in[u] = point_in_box(x, y, z, lo, hi);
        const unsigned long long ballot = __ballot(in[u]);
        before[u] = mbcnt64(ballot);
        if (lane == 0) wcnt[u][wave] = __popcll(ballot);
    }
    __syncthreads();
    int total = 0;                                                   // before[u]: the inside points ahead of this one, in (u, wave, lane) order
#pragma unroll
    for (int u = 0; u < QB; ++u) {
#pragma unroll
        for (int w = 0; w < THREADS / GSPN_WAVE; ++w) {
            if (in[u] && w == wave) before[u] += total;
            total += wcnt[u][w];
        }
    }
#pragma unroll
    for (int u = 0; u < QB; ++u)
        if (total > 0 && in[u]) list[before[u]] = u * THREADS + tid; // before[u] < total <= THREADS * QB
    return total;
}

// The set of p points at s into the three planes, the slots past p NaN.  The caller's barrier follows.
template <int THREADS>
__device__ __forceinline__ void inbox_stage(const float* s, int p, int p4, float* planes) {
    for (int j = threadIdx.x; j < p4; j += THREADS) {
        const float* g = s + 3 * (long)min(j, p - 1);
        planes[j] = j < p ? g[0] : NAN;
        planes[p4 + j] = g[1];
        planes[2 * p4 + j] = g[2];
    }
}

// For entry e < total of the tile, at tile offset list[e] (gated) or e itself (not gated: every point of the tile, list is not read):
// emit(tile offset, position of the nearest of the p staged points), from one lane.  pts: the coordinates the tile's points were loaded
// from, point i0 + offset.  No barrier and no return inside: a wave without an entry falls through.
template <int THREADS, int QB, typename Emit>
__device__ __forceinline__ void inbox_walk(const float* pts, int i0, const float* planes, int p, int p4, const int* list,
                                           bool gated, int total, Emit emit) {
    const int tid = threadIdx.x, wave = tid / GSPN_WAVE;
    // Few inside points (a detection holds about a hundredth of the cloud): s lanes share one entry, lane g of them walks the points
    // g, g + s, ... (neighbouring lanes read neighbouring words of a plane), and the s results meet by shuffles.  The smaller distance
    // wins, the smaller position among equal ones: the first minimum, as in the walk of one lane.
    int s_lanes = 1;
    if (gated)
        while (s_lanes < GSPN_WAVE && 2 * s_lanes * total <= THREADS) s_lanes <<= 1;
    if (s_lanes > 1) {                                               // uniform
        if (wave * GSPN_WAVE < total * s_lanes) {                    // uniform over the wave: it has an entry
            const int e = tid / s_lanes, g = tid % s_lanes;
            const int at = e < total ? list[e] : -1;
            const float* q = pts + 3 * (long)(i0 + max(at, 0));      // list[e] names a point before the end
            const float qx = q[0], qy = q[1], qz = q[2];
            float best = INFINITY;
            int arg = 0;
            for (int j = g; j < p; j += s_lanes) {
                const float dx = qx - planes[j], dy = qy - planes[p4 + j], dz = qz - planes[2 * p4 + j];
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (d < best) {
                    best = d;
                    arg = j;
                }
            }
            for (int w = s_lanes >> 1; w > 0; w >>= 1) {
                const float ob = __shfl_xor(best, w, GSPN_WAVE);
                const int oa = __shfl_xor(arg, w, GSPN_WAVE);
                if (ob < best || (ob == best && oa < arg)) {
                    best = ob;
                    arg = oa;
                }
            }
            if (g == 0 && at >= 0) emit(at, arg);                    // arg < p: a slot past p never wins
        }
    } else if (wave * GSPN_WAVE < total) {                           // entry u * THREADS + tid: none for the waves behind
        const float4* X = (const float4*)planes;
        const float4* Y = (const float4*)(planes + p4);
        const float4* Z = (const float4*)(planes + 2 * p4);
        int at[QB];
        float qx[QB], qy[QB], qz[QB], best[QB];
        int arg[QB];
#pragma unroll
        for (int u = 0; u < QB; ++u) {
            const int e = u * THREADS + tid;                         // e < THREADS * QB, the size of list
            at[u] = -1;
            if (e < total) at[u] = gated ? list[e] : e;
            const float* q = pts + 3 * (long)(i0 + max(at[u], 0));
            qx[u] = q[0];
            qy[u] = q[1];
            qz[u] = q[2];
            best[u] = INFINITY;
            arg[u] = 0;
        }
        for (int j4 = 0; j4 < p4 / 4; ++j4) {
            const float4 sx = X[j4], sy = Y[j4], sz = Z[j4];
            const float px[4] = {sx.x, sx.y, sx.z, sx.w}, py[4] = {sy.x, sy.y, sy.z, sy.w}, pz[4] = {sz.x, sz.y, sz.z, sz.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int u = 0; u < QB; ++u) {
                    const float dx = qx[u] - px[t], dy = qy[u] - py[t], dz = qz[u] - pz[t];
                    const float d = (dx * dx + dy * dy) + dz * dz;
                    if (d < best[u]) {                               // strict: the smallest position among equal distances (tf.argmin)
                        best[u] = d;
                        arg[u] = 4 * j4 + t;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < QB; ++u)
            if (at[u] >= 0) emit(at[u], arg[u]);
    }
}
