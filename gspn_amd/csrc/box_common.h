// box_common.h -- device helpers shared by the box stages (spn_boxes.hip, roi.hip, detect.hip, nms3d.hip), whose translation units are
// compiled with -ffp-contract=off: everything here is evaluated as the reference (models/model_rpointnet.py) writes it.  A box is
// (centre[3], size[3]).
#pragma once
#include "common.h"

// the shape of the point scans of gspn_box_shrink and gspn_box_point_count: lanes per workgroup, points per lane and trip
#define BOX_SCAN_THREADS 256
#define BOX_SCAN_WAVES (BOX_SCAN_THREADS / GSPN_WAVE)
#define BOX_SCAN_UNROLL 4

// lo = c - s/2, hi = c + s/2 (:529-551, :673-674, :1042) ...
__device__ __forceinline__ void box_bounds(const float* __restrict__ q, float (&lo)[3], float (&hi)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float h = q[3 + a] / 2.0f;
        lo[a] = q[a] - h;
        hi[a] = q[a] + h;
    }
}
// ... and widened by a margin applied after the half size (:764-765 with 1e-3)
__device__ __forceinline__ void box_bounds(const float* __restrict__ q, float margin, float (&lo)[3], float (&hi)[3]) {
    box_bounds(q, lo, hi);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = lo[a] - margin;
        hi[a] = hi[a] + margin;
    }
}
// bounds included; a NaN coordinate is inside nothing
__device__ __forceinline__ bool point_in_box(float x, float y, float z, const float (&lo)[3], const float (&hi)[3]) {
    return x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] && z >= lo[2] && z <= hi[2];
}

// IoU of two boxes (:617-623, :683-689), in the reference's order of operations
__device__ __forceinline__ float box_iou(const float* __restrict__ p, const float* __restrict__ q) {
    const float vp = p[3] * p[4] * p[5], vq = q[3] * q[4] * q[5];
    float cube[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float va = fmaxf(p[a] - p[3 + a] / 2.0f, q[a] - q[3 + a] / 2.0f);
        const float vb = fminf(p[a] + p[3 + a] / 2.0f, q[a] + q[3 + a] / 2.0f);
        cube[a] = fmaxf(vb - va, 0.0f);
    }
    const float inter = cube[0] * cube[1] * cube[2];
    return inter / (vp + vq - inter + 1e-8f);
}

// the padding row of a box list
__device__ __forceinline__ bool zero_row6(const float* __restrict__ q) {
    return q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f && q[4] == 0.0f && q[5] == 0.0f;
}
