// detect.hip -- the detection output stage of R-PointNet (models/model_rpointnet.py) behind the two heads, ABI 14.
//
//   gspn_class_nms3d       the per-class NMS of refine_detections (:855-901): the reference calls nms_3d once per class through a py_func and
//                          intersects index sets on the host.  One workgroup per scene and ONE pass over all candidates in score order: the
//                          sort, the register-resident candidates and the double-buffered live mask of gspn_nms3d (roi.hip); a pick tests only
//                          the live candidates of its own class, and every live candidate counts the picks of its class, so a class leaves
//                          after max_per_class picks -- or at once after a pick that survives its own IoU test, which the reference would pick
//                          again until the class is full and then collapse into one row (:893).  The picks come out in descending score, which
//                          is the order of the reference's final top_k (:900).
//   gspn_nearest_in_sets   the argmin of unmold_segmentation (:1032-1033) behind the box test of :1042, without the (B, R, N, P) distance
//                          tensor: a workgroup per (scene, ROI, query tile).  The inside test first; the inside queries are compacted into
//                          LDS by wave ballot, and a tile without one leaves before anything is staged.  Then the ROI's points are staged as
//                          three planes and every lane walks them for QB compacted queries held in registers (one broadcast LDS read of
//                          four points serves 4 x QB distances).  A tile with few inside queries -- the usual case, a detection holds about
//                          a hundredth of the cloud -- gives each query to 2..64 lanes that split the points and meet by shuffles.
//
// fp32 throughout, no atomics, no host synchronisation, no allocation.  Compiled with -ffp-contract=off: every bound, volume, IoU and distance
// below is evaluated exactly as the reference writes it.
#include <math.h>

#include "common.h"

#define CN_THREADS 1024
#define CN_WAVES (CN_THREADS / GSPN_WAVE)
#define CN_MAX_N 4096
#define CN_SLOTS (CN_MAX_N / CN_THREADS)
#define CN_WORDS (CN_MAX_N / 64)
#define NN_THREADS 256
#define NN_WAVES (NN_THREADS / GSPN_WAVE)
#define NN_MAX_P 4096
#define NN_MAX_N 32768

namespace {

__device__ __forceinline__ int det_mbcnt64(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// ---------------------------------------------------------------------------------------------------- per-class nms_3d
// grid (b), CN_THREADS lanes, p = n rounded up to a power of two (>= 64).  Dynamic LDS: the live mask twice (2 x 64 words), the sorted
// indices and their classes (2 x p ints), then lo[3], hi[3], volume of the sorted candidates (7 x p floats); the sort's 64-bit keys lie
// over the last region.
__global__ __launch_bounds__(CN_THREADS) void class_nms3d_kernel(int n, int p, int per_class, int m, float iou_thr, const float* __restrict__ boxes,
                                                                 const float* __restrict__ scores, const int* __restrict__ class_ids,
                                                                 int* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char cn_smem[];
    unsigned long long* alive = (unsigned long long*)cn_smem;                      // [2][CN_WORDS]
    int* sidx = (int*)(cn_smem + 2 * CN_WORDS * 8);                               // [p]
    int* scls = sidx + p;                                                          // [p]
    float* cb = (float*)(scls + p);                                                // [7][p]
    unsigned long long* key = (unsigned long long*)cb;                             // [p], dead before cb is written
    const int bi = blockIdx.x, tid = threadIdx.x, lane = tid % GSPN_WAVE, wave = tid / GSPN_WAVE;
    const float* bx = boxes + (long)bi * n * 6;
    const float* sc = scores + (long)bi * n;
    const int* ci = class_ids + (long)bi * n;
    int* o = out + (long)bi * m;

    // ascending 64-bit keys = descending score, lower index first among equal scores (-0 counts as +0); a row of class <= 0 is no candidate
    for (int k = tid; k < p; k += CN_THREADS) {
        unsigned long long v = ~0ull;
        if (k < n && ci[k] > 0) {
            unsigned u = __float_as_uint(sc[k] + 0.0f);
            u = (u >> 31) ? ~u : (u | 0x80000000u);
            v = ((unsigned long long)(~u) << 32) | (unsigned)k;
        }
        key[k] = v;
    }
    __syncthreads();
    for (int size = 2; size <= p; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < p / 2; t += CN_THREADS) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;
                const unsigned long long a = key[i], c = key[l];
                if ((a > c) == ((i & size) == 0)) {
                    key[i] = c;
                    key[l] = a;
                }
            }
            __syncthreads();
        }
    }

    // candidate k = u * CN_THREADS + tid lives in this lane's registers; bit (k % 64) of word (k / 64) says whether it is still live
    int si[CN_SLOTS];
#pragma unroll
    for (int u = 0; u < CN_SLOTS; ++u) {
        const int k = u * CN_THREADS + tid;
        si[u] = -1;
        if (k < p) {
            const unsigned long long v = key[k];
            if (v != ~0ull) si[u] = (int)(unsigned)v;
        }
    }
    __syncthreads();                                                 // the keys are dead: cb takes their place
    float lo[CN_SLOTS][3], hi[CN_SLOTS][3], vol[CN_SLOTS];
    int cls[CN_SLOTS], seen[CN_SLOTS];                               // seen: the picks of this candidate's class so far
    bool live[CN_SLOTS];
#pragma unroll
    for (int u = 0; u < CN_SLOTS; ++u) {
        const int k = u * CN_THREADS + tid;
        live[u] = false;
        cls[u] = 0;
        seen[u] = 0;
        if (k < p) {
            float q[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (si[u] >= 0) {
#pragma unroll
                for (int a = 0; a < 6; ++a) q[a] = bx[(long)si[u] * 6 + a];
                cls[u] = ci[si[u]];
                live[u] = true;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[u][a] = q[a] - q[3 + a] / 2.0f;
                hi[u][a] = q[a] + q[3 + a] / 2.0f;
                cb[a * p + k] = lo[u][a];
                cb[(3 + a) * p + k] = hi[u][a];
            }
            vol[u] = q[3] * q[4] * q[5];
            cb[6 * p + k] = vol[u];
            sidx[k] = si[u];
            scls[k] = cls[u];
        }
        const unsigned long long mask = __ballot(live[u]);
        if (lane == 0) alive[u * CN_WAVES + wave] = mask;
    }
    __syncthreads();

    int count = 0;
    for (; count < m; ++count) {
        const unsigned long long* cur = alive + (count & 1) * CN_WORDS;
        unsigned long long* nxt = alive + ((count + 1) & 1) * CN_WORDS;
        const unsigned long long nz = __ballot(cur[lane] != 0ull);   // lane l looks at word l: CN_WORDS == 64
        if (nz == 0ull) break;                                       // every wave reads the same words: uniform
        const int word = __builtin_ctzll(nz);
        const int k0 = word * 64 + __builtin_ctzll(cur[word]);
        float plo[3], phi[3], own[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            plo[a] = cb[a * p + k0];
            phi[a] = cb[(3 + a) * p + k0];
            own[a] = fmaxf(phi[a] - plo[a], 0.0f);                   // min(hi, hi) - max(lo, lo)
        }
        const float pvol = cb[6 * p + k0];
        const int pcls = scls[k0];
        if (tid == 0) o[count] = sidx[k0];
        // the pick's own test, as its lane evaluates it below: a pick that survives it would be picked until its class is full
        const float own_inter = own[0] * own[1] * own[2];
        const bool exhausted = !(own_inter / (((pvol + pvol) - own_inter) + 1e-8f) > iou_thr);
#pragma unroll
        for (int u = 0; u < CN_SLOTS; ++u) {
            if (live[u] && cls[u] == pcls) {
                float cube[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) cube[a] = fmaxf(fminf(phi[a], hi[u][a]) - fmaxf(plo[a], lo[u][a]), 0.0f);
                const float inter = cube[0] * cube[1] * cube[2];
                const float iou = inter / (((vol[u] + pvol) - inter) + 1e-8f);
                ++seen[u];
                if (iou > iou_thr || exhausted || seen[u] >= per_class) live[u] = false;
            }
            const unsigned long long mask = __ballot(live[u]);
            if (lane == 0) nxt[u * CN_WAVES + wave] = mask;
        }
        __syncthreads();
    }
    for (int j = count + tid; j < m; j += CN_THREADS) o[j] = -1;
}

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
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = bx[a] - bx[3 + a] / 2.0f;
            hi[a] = bx[a] + bx[3 + a] / 2.0f;
        }
        bool in[QB];
        int before[QB];
#pragma unroll
        for (int u = 0; u < QB; ++u) {
            const int i = i0 + u * NN_THREADS + tid;
            const float* g = q + 3 * (long)min(i, n - 1);
            const float x = i < n ? g[0] : NAN, y = g[1], z = g[2];  // a slot past n holds NaN, which is inside no box
            in[u] = x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] && z >= lo[2] && z <= hi[2];
            const unsigned long long mask = __ballot(in[u]);
            before[u] = det_mbcnt64(mask);
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

extern "C" int gspn_class_nms3d(int b, int n, int max_per_class, int max_output_size, float iou_threshold, const float* boxes, const float* scores,
                                const int* class_ids, int* selected, void* stream) {
    if (b <= 0 || n <= 0 || max_per_class <= 0 || max_output_size <= 0) return GSPN_ERR_ARG;
    if (n > CN_MAX_N) return GSPN_ERR_UNSUPPORTED;
    int p = 64;
    while (p < n) p <<= 1;
    const size_t lds = 2 * CN_WORDS * 8 + (size_t)p * 8 + (size_t)p * 28;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)class_nms3d_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * CN_WORDS * 8 + CN_MAX_N * 36) != hipSuccess)
        return (int)hipGetLastError();
    class_nms3d_kernel<<<b, CN_THREADS, lds, (hipStream_t)stream>>>(n, p, max_per_class, max_output_size, iou_threshold, boxes, scores, class_ids,
                                                                   selected);
    return gspn_launch_status();
}

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
