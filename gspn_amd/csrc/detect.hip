// detect.hip -- the detection output stage of R-PointNet (models/model_rpointnet.py) behind the two heads, ABI 14, without its per-class NMS
// (gspn_class_nms3d of nms3d.hip).
//   gspn_nearest_in_sets   the argmin of unmold_segmentation (:1032-1033) behind the box test of :1042, without the (B, R, N, P) distance
//                          tensor: a workgroup per (scene, ROI, query tile) over the in-box nearest-point tile of inbox_nearest.h (the
//                          inside test, the compacted list, the ROI's points as three LDS planes, the two walks), which lift.hip shares.
//                          The kernel adds what is its own: -1 for a query outside the box, a tile without an inside query leaves before
//                          anything is staged, the nearest position itself is the output, and the form without boxes searches for every
//                          query of the tile.
//
// fp32 throughout, no atomics, no host synchronisation, no allocation.  Compiled with -ffp-contract=off: every bound, volume, IoU and distance
// below and in inbox_nearest.h is evaluated exactly as the reference writes it.
#include "inbox_nearest.h"

#define NN_THREADS 256
#define NN_WAVES (NN_THREADS / GSPN_WAVE)
#define NN_MAX_P 4096
#define NN_MAX_N 32768

namespace {

// ---------------------------------------------------------------------------------------------------- nearest point of each set
// grid (ceil(n / (NN_THREADS * QB)), r, b), NN_THREADS lanes.  Dynamic LDS: the set as three planes of p4 = p rounded up to 4 floats, the
// slots past p NaN (a NaN distance is smaller than nothing).  list: the tile's inside queries, ascending.
template <int QB>
__global__ __launch_bounds__(NN_THREADS) void nearest_in_sets_kernel(int r, int n, int p, int p4, const float* __restrict__ query,
                                                                     const float* __restrict__ sets, const float* __restrict__ boxes,
                                                                     int* __restrict__ idx) {
    extern __shared__ __align__(16) float nn_planes[];               // [3][p4]
    __shared__ int list[NN_THREADS * QB];
    __shared__ int wcnt[QB][NN_WAVES];
    const int ri = blockIdx.y, bi = blockIdx.z, tid = threadIdx.x;
    const int i0 = blockIdx.x * NN_THREADS * QB;
    const float* q = query + (long)bi * n * 3;
    int* o = idx + ((long)bi * r + ri) * n;
    int total = min(NN_THREADS * QB, n - i0);                        // not gated: every query of the tile

    if (boxes != nullptr) {
        const float* bx = boxes + ((long)bi * r + ri) * 6;           // uniform: scalar loads
        float lo[3], hi[3];
        box_bounds(bx, lo, hi);
        bool in[QB];
        total = inbox_compact<NN_THREADS, QB>(q, i0, n, lo, hi, in, list, wcnt);
#pragma unroll
        for (int u = 0; u < QB; ++u) {
            const int i = i0 + u * NN_THREADS + tid;
            if (i < n && !in[u]) o[i] = -1;
        }
        if (total == 0) return;                                      // uniform: nothing of this tile lies in the box
    }
    inbox_stage<NN_THREADS>(sets + ((long)bi * r + ri) * p * 3, p, p4, nn_planes);
    __syncthreads();
    inbox_walk<NN_THREADS, QB>(q, i0, nn_planes, p, p4, list, boxes != nullptr, total, [&](int at, int arg) { o[i0 + at] = arg; });
}

}  // namespace

extern "C" int gspn_nearest_in_sets(int b, int r, int n, int p, const float* query, const float* sets, const float* boxes, int* idx, void* stream) {
    if (b <= 0 || r <= 0 || n <= 0 || p <= 0) return GSPN_ERR_ARG;
    if (p > NN_MAX_P || n > NN_MAX_N || r > 65535 || b > 65535) return GSPN_ERR_UNSUPPORTED;
    const int p4 = (p + 3) / 4 * 4;
    const size_t lds = (size_t)3 * p4 * sizeof(float);               // <= 48 KiB, beside 4 KiB of static LDS
    hipStream_t st = (hipStream_t)stream;
    if (inbox_points_per_lane<NN_THREADS>((long)b * r, n) == 4)
        nearest_in_sets_kernel<4><<<dim3((n + NN_THREADS * 4 - 1) / (NN_THREADS * 4), r, b), NN_THREADS, lds, st>>>(r, n, p, p4, query, sets, boxes, idx);
    else
        nearest_in_sets_kernel<1><<<dim3((n + NN_THREADS - 1) / NN_THREADS, r, b), NN_THREADS, lds, st>>>(r, n, p, p4, query, sets, boxes, idx);
    return gspn_launch_status();
}
