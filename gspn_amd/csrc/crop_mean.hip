// crop_mean.hip -- the per-ROI mean of a few gathered columns, ABI 16.
//
// R-PointNet's inference path (models/model_rpointnet.py:1144-1150) appends fb_prob (1 column) and sem_prob (NUM_CATEGORY columns) to the
// feature tensor, crops all of it per ROI and then only averages those columns over each ROI's points.  Here the average is taken from the
// narrow table itself:
//     out[s, k, :] = (1 / p) * sum_j table[s, idx[s, k, j], :]
// so the cropped feature tensor stays as wide as the features and the (b, r, p, c) crop of the table is never written.
//
//   gspn_crop_mean   one workgroup per (scene, ROI).  The index row is staged through LDS CM_THREADS values at a time (a coalesced read,
//                    clamped there); LANES = the smallest power of two >= c lanes share a gathered row -- one contiguous read of c floats --
//                    and the CM_THREADS / LANES row groups walk the staged rows with that stride.  Every thread adds its rows in double in
//                    ascending order, the row groups are added through LDS in group order, the sum is divided by p in double and rounded to
//                    float once.  No atomics: the rows a thread takes and both orders depend on the shape alone, so the bits repeat, and a
//                    row that names one point p times returns that point's values exactly (p * x is exact in double).
//
// An index outside [0, n) is clamped, as in gspn_crop_linear_fwd.  No alignment beyond 4 bytes: every access is one float or one int.
#include "common.h"

#define CM_THREADS 256
#define CM_MAX_C 64

namespace {

__global__ __launch_bounds__(CM_THREADS) void crop_mean_kernel(int n, int r, int p, int c, int lanes_log2, const float* __restrict__ table,
                                                               const int* __restrict__ idx, float* __restrict__ out) {
    __shared__ int src[CM_THREADS];
    __shared__ double red[CM_THREADS];                                           // [groups][lanes]
    const int lanes = 1 << lanes_log2, groups = CM_THREADS >> lanes_log2;
    const int lane = threadIdx.x & (lanes - 1), g = threadIdx.x >> lanes_log2;
    const long roi = blockIdx.x;                                                  // scene * r + k
    const float* scene_table = table + (roi / r) * (long)n * c;
    const int* row_idx = idx + roi * p;
    const bool live = lane < c;
    double acc = 0.0;
    for (long j0 = 0; j0 < p; j0 += CM_THREADS) {
        const int staged = p - j0 < CM_THREADS ? (int)(p - j0) : CM_THREADS;
        __syncthreads();                                                          // the previous chunk's indices have been read
        if ((int)threadIdx.x < staged) src[threadIdx.x] = min(max(row_idx[j0 + threadIdx.x], 0), n - 1);
        __syncthreads();
        if (live)
            for (int i = g; i < staged; i += groups) acc += (double)scene_table[(long)src[i] * c + lane];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < c) {                                                   // c <= lanes: thread t is lane t of group 0
        double sum = 0.0;
        for (int u = 0; u < groups; ++u) sum += red[(u << lanes_log2) + threadIdx.x];
        out[roi * c + threadIdx.x] = (float)(sum / (double)p);
    }
}

}  // namespace

extern "C" int gspn_crop_mean(int b, int n, int r, int p, int c, const float* table, const int* idx, float* out, void* stream) {
    if (b <= 0 || n <= 0 || r <= 0 || p <= 0 || c <= 0 || !table || !idx || !out) return GSPN_ERR_ARG;
    if (c > CM_MAX_C || (long)b * r >= (1L << 31)) return GSPN_ERR_UNSUPPORTED;
    int lanes_log2 = 0;
    while ((1 << lanes_log2) < c) ++lanes_log2;
    crop_mean_kernel<<<(unsigned)((long)b * r), CM_THREADS, 0, (hipStream_t)stream>>>(n, r, p, c, lanes_log2, table, idx, out);
    return gspn_launch_status();
}
