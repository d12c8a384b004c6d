// detect.hip -- the detection output stage of R-PointNet (models/model_rpointnet.py) behind the two heads, ABI 14, without its per-class NMS
// (gspn_class_nms3d of nms3d.hip).
//   gspn_nearest_in_sets   the argmin of unmold_segmentation (:1032-1033) behind the box test of :1042, without the (B, R, N, P) distance
//                          tensor: a workgroup per (scene, ROI, query tile).  The inside test first; the inside queries are compacted into
//                          LDS by wave ballot, and a tile without one leaves before anything is staged.  Then the ROI's points are staged as
//                          three planes and every lane walks them for QB compacted queries held in registers (one broadcast LDS read of
//                          four points serves 4 x QB distances).  A tile with few inside queries -- the usual case, a detection holds about
//                          a hundredth of the cloud -- gives each query to 2..64 lanes that split the points and meet by shuffles.
//
// fp32 throughout, no atomics, no host synchronisation, no allocation.  Compiled with -ffp-contract=off: every bound, volume, IoU and distance
// below is evaluated exactly as the reference writes it.
#include "box_common.h"

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
    const int ri = blockIdx.y, bi = blockIdx.z, tid = threadIdx.x, lane = tid % GSPN_WAVE, wave = tid / GSPN_WAVE;
    const int i0 = blockIdx.x * NN_THREADS * QB;
    const float* q = query + (long)bi * n * 3;
    int* o = idx + ((long)bi * r + ri) * n;
    int total = min(NN_THREADS * QB, n - i0);

    if (boxes != nullptr) {
        const float* bx = boxes + ((long)bi * r + ri) * 6;           // uniform: scalar loads
        float lo[3], hi[3];
        box_bounds(bx, lo, hi);
        bool in[QB];
        int before[QB];
#pragma unroll
        for (int u = 0; u < QB; ++u) {
            const int i = i0 + u * NN_THREADS + tid;
            const float* g = q + 3 * (long)min(i, n - 1);
            const float x = i < n ? g[0] : NAN, y = g[1], z = g[2];  // a slot past n holds NaN, which is inside no box
            in[u] = point_in_box(x, y, z, lo, hi);
            const unsigned long long mask = __ballot(in[u]);
            before[u] = mbcnt64(mask);
            if (lane == 0) wcnt[u][wave] = __popcll(mask);
            if (i < n && !in[u]) o[i] = -1;
        }
        __syncthreads();
        total = 0;                                                   // before[u]: the inside queries ahead of this one, in (u, wave, lane) order
#pragma unroll
        for (int u = 0; u < QB; ++u) {
#pragma unroll
            for (int w = 0; w < NN_WAVES; ++w) {
                if (in[u] && w == wave) before[u] += total;
                total += wcnt[u][w];
            }
        }
        if (total == 0) return;                                      // uniform: nothing of this tile lies in the box
#pragma unroll
        for (int u = 0; u < QB; ++u)
            if (in[u]) list[before[u]] = u * NN_THREADS + tid;       // before[u] < total <= NN_THREADS * QB
    }
    const float* s = sets + ((long)bi * r + ri) * p * 3;
    for (int j = tid; j < p4; j += NN_THREADS) {
        const float* g = s + 3 * (long)min(j, p - 1);
        nn_planes[j] = j < p ? g[0] : NAN;
        nn_planes[p4 + j] = g[1];
        nn_planes[2 * p4 + j] = g[2];
    }
    __syncthreads();

    // Few inside queries (a detection holds about a hundredth of the cloud): s lanes share one query, lane g of them walks the points
    // g, g + s, ... (neighbouring lanes read neighbouring words of a plane), and the s results meet by shuffles.  The smaller distance
    // wins, the smaller position among equal ones: the first minimum, as in the walk of one lane.
    int s_lanes = 1;
    if (boxes != nullptr)
        while (s_lanes < GSPN_WAVE && 2 * s_lanes * total <= NN_THREADS) s_lanes <<= 1;
    if (s_lanes > 1) {                                               // uniform
        if (wave * GSPN_WAVE >= total * s_lanes) return;             // (no barrier below) no query for this wave
        const int e = tid / s_lanes, g = tid % s_lanes;
        const int qi = e < total ? i0 + list[e] : -1;
        const float* c = q + 3 * (long)max(qi, 0);
        const float qx = c[0], qy = c[1], qz = c[2];
        float best = INFINITY;
        int arg = 0;
        for (int j = g; j < p; j += s_lanes) {
            const float dx = qx - nn_planes[j], dy = qy - nn_planes[p4 + j], dz = qz - nn_planes[2 * p4 + j];
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
        if (g == 0 && qi >= 0) o[qi] = arg;
        return;
    }

    const float4* X = (const float4*)nn_planes;
    const float4* Y = (const float4*)(nn_planes + p4);
    const float4* Z = (const float4*)(nn_planes + 2 * p4);
    if (wave * GSPN_WAVE >= total) return;                           // (no barrier below) entry u * NN_THREADS + tid: none for this wave
    int qi[QB];
    float qx[QB], qy[QB], qz[QB], best[QB];
    int arg[QB];
#pragma unroll
    for (int u = 0; u < QB; ++u) {
        const int e = u * NN_THREADS + tid;                          // e < NN_THREADS * QB, the size of list
        qi[u] = -1;
        if (e < total) qi[u] = i0 + (boxes != nullptr ? list[e] : e);
        const float* g = q + 3 * (long)max(qi[u], 0);
        qx[u] = g[0];
        qy[u] = g[1];
        qz[u] = g[2];
        best[u] = INFINITY;
        arg[u] = 0;
    }
    for (int j4 = 0; j4 < p4 / 4; ++j4) {
        const float4 sx = X[j4], sy = Y[j4], sz = Z[j4];
        const float px[4] = {sx.x, sx.y, sx.z, sx.w}, py[4] = {sy.x, sy.y, sy.z, sy.w}, pz[4] = {sz.x, sz.y, sz.z, sz.w};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
#pragma unroll
            for (int u = 0; u < QB; ++u) {
                const float dx = qx[u] - px[v], dy = qy[u] - py[v], dz = qz[u] - pz[v];
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (d < best[u]) {                                   // strict: the smallest position among equal distances (tf.argmin)
                    best[u] = d;
                    arg[u] = 4 * j4 + v;
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < QB; ++u)
        if (qi[u] >= 0) o[qi[u]] = arg[u];
}

}  // namespace

extern "C" int gspn_nearest_in_sets(int b, int r, int n, int p, const float* query, const float* sets, const float* boxes, int* idx, void* stream) {
    if (b <= 0 || r <= 0 || n <= 0 || p <= 0) return GSPN_ERR_ARG;
    if (p > NN_MAX_P || n > NN_MAX_N || r > 65535 || b > 65535) return GSPN_ERR_UNSUPPORTED;
    const int p4 = (p + 3) / 4 * 4;
    const size_t lds = (size_t)3 * p4 * sizeof(float);               // <= 48 KiB, beside 4 KiB of static LDS
    hipStream_t st = (hipStream_t)stream;
    // four queries per lane once that still gives every CU two workgroups; one per lane below (the one-set form, small clouds)
    if ((long)b * r * ((n + NN_THREADS * 4 - 1) / (NN_THREADS * 4)) >= 512)
        nearest_in_sets_kernel<4><<<dim3((n + NN_THREADS * 4 - 1) / (NN_THREADS * 4), r, b), NN_THREADS, lds, st>>>(r, n, p, p4, query, sets, boxes, idx);
    else
        nearest_in_sets_kernel<1><<<dim3((n + NN_THREADS - 1) / NN_THREADS, r, b), NN_THREADS, lds, st>>>(r, n, p, p4, query, sets, boxes, idx);
    return gspn_launch_status();
}
