// lift.hip -- predictions on a scan's own vertices (additive at ABI 21): test.py:163-189 and :204 with a vertex of the scan in
// the place of a scene point, for one scan of v vertices (50 000 to over 500 000) and its r detections.
//
//   gspn_lift_masks   gspn_nearest_in_sets (detect.hip) and gspn_scene_confidence (predict.hip) in one pass that never writes the (r, v) index
//                     tensor.  A workgroup per (detection, tile of LM_THREADS * QB vertices), with the structure of nearest_in_sets_kernel:
//                     the inside test first; the inside vertices are compacted into LDS by wave ballot, and a tile without one stages
//                     nothing; the detection's crop points sit in LDS as three planes; few inside vertices are split over 2..64 lanes that
//                     meet by shuffles.  The lane that finds a vertex's nearest crop point j leaves masks[k][j] in the vertex's own LDS
//                     slot; behind a barrier every lane is back at its own vertices, in tile order: it reads sem_prob[src[v]][class] and
//                     vert_fb[v] for an inside vertex alone (about one in a hundred), writes every mask byte of the tile -- zeros outside
//                     the box -- and adds its three double terms and its set bytes.  Lanes meet in a __shfl_down tree, waves through LDS in
//                     wave order, and the tile's (S0, S1, S2, count) goes to its own slot of `part`, also when the tile is empty.
//   lift_finish       one wave per detection adds its tiles' slots in ascending order with a lane stride of 64 and a shuffle tree, and
//                     writes sem_conf, fb_conf and mask_points.
//
// Which lane adds which term, and both orders, depend on (r, v) alone: the same bits on every call.  fp32 distances exactly as the reference
// writes them (-ffp-contract=off), double sums of exact terms, no float atomics, no host synchronisation, nothing allocated.  Row offsets
// are 64-bit: r * v exceeds 2^31.
#include "box_common.h"

#define LM_THREADS 256
#define LM_WAVES (LM_THREADS / GSPN_WAVE)
#define LM_MAX_P 4096
#define LM_MAX_V (1 << 24)
#define LM_PART 4                                                    // doubles per slot: S0, S1, S2, the set bytes

namespace {

__device__ __forceinline__ double lm_wave_sum(double v) {
    for (int off = GSPN_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, GSPN_WAVE);
    return v;                                                        // lane 0 holds the wave's sum
}

// grid (tiles, r), LM_THREADS lanes.  Dynamic LDS: the crop points as three planes of p4 = p rounded up to 4 floats, the slots past p NaN
// (a NaN distance is smaller than nothing).  list: the tile's inside vertices, ascending; value[e]: the mask value of tile entry e.
template <int QB>
__global__ __launch_bounds__(LM_THREADS) void lift_masks_kernel(int v, int p, int p4, int n, int c, const float* __restrict__ verts,
                                                                const float* __restrict__ crops, const float* __restrict__ boxes,
                                                                const float* __restrict__ masks, const int* __restrict__ class_ids,
                                                                const int* __restrict__ src, const float* __restrict__ sem_prob,
                                                                const float* __restrict__ vert_fb, double mask_th, double* __restrict__ part,
                                                                unsigned char* __restrict__ mask) {
    extern __shared__ __align__(16) float lm_planes[];               // [3][p4]
    __shared__ int list[LM_THREADS * QB];
    __shared__ float value[LM_THREADS * QB];
    __shared__ int wcnt[QB][LM_WAVES];
    __shared__ double red[LM_PART][LM_WAVES];
    const int ri = blockIdx.y, tid = threadIdx.x, lane = tid % GSPN_WAVE, wave = tid / GSPN_WAVE;
    const int i0 = blockIdx.x * LM_THREADS * QB;                     // < v <= 2^24
    unsigned char* o = mask + (long)ri * v;
    double* slot = part + ((long)ri * gridDim.x + blockIdx.x) * LM_PART;
    const int cls = class_ids[ri];                                   // uniform

    bool in[QB] = {};
    int total = 0;
    if (cls > 0 && cls < c) {                                        // a row test.py:159-161 drops holds no vertex
        const float* bx = boxes + (long)ri * 6;                      // uniform: scalar loads
        float lo[3], hi[3];
        box_bounds(bx, lo, hi);
        int before[QB];
#pragma unroll
        for (int u = 0; u < QB; ++u) {
            const int i = i0 + u * LM_THREADS + tid;
            const float* g = verts + 3 * (long)min(i, v - 1);
            const float x = i < v ? g[0] : NAN, y = g[1], z = g[2];  // a slot past v holds NaN, which is inside no box
            in[u] = point_in_box(x, y, z, lo, hi);
            const unsigned long long ballot = __ballot(in[u]);
            before[u] = mbcnt64(ballot);
            if (lane == 0) wcnt[u][wave] = __popcll(ballot);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < QB; ++u) {                               // before[u]: the inside vertices ahead of this one, in (u, wave, lane) order
#pragma unroll
            for (int w = 0; w < LM_WAVES; ++w) {
                if (in[u] && w == wave) before[u] += total;
                total += wcnt[u][w];
            }
        }
#pragma unroll
        for (int u = 0; u < QB; ++u)
            if (total > 0 && in[u]) list[before[u]] = u * LM_THREADS + tid;      // before[u] < total <= LM_THREADS * QB
    }
    if (total == 0) {                                                // uniform: a dropped row, or nothing of this tile lies in the box
#pragma unroll
        for (int u = 0; u < QB; ++u) {
            const int i = i0 + u * LM_THREADS + tid;
            if (i < v) o[i] = 0;
        }
        if (tid < LM_PART) slot[tid] = 0.0;
        return;
    }

    const float* s = crops + (long)ri * p * 3;
    for (int j = tid; j < p4; j += LM_THREADS) {
        const float* g = s + 3 * (long)min(j, p - 1);
        lm_planes[j] = j < p ? g[0] : NAN;
        lm_planes[p4 + j] = g[1];
        lm_planes[2 * p4 + j] = g[2];
    }
    __syncthreads();
    const float* row_masks = masks + (long)ri * p;

    // Few inside vertices (a detection holds about a hundredth of the scan): s lanes share one vertex, lane g of them walks the points
    // g, g + s, ... (neighbouring lanes read neighbouring words of a plane), and the s results meet by shuffles.  The smaller distance
    // wins, the smaller position among equal ones: the first minimum, as in the walk of one lane.
    int s_lanes = 1;
    while (s_lanes < GSPN_WAVE && 2 * s_lanes * total <= LM_THREADS) s_lanes <<= 1;
    if (s_lanes > 1) {                                               // uniform
        if (wave * GSPN_WAVE < total * s_lanes) {                    // uniform over the wave: it has a vertex
            const int e = tid / s_lanes, g = tid % s_lanes;
            const int at = e < total ? list[e] : -1;
            const float* q = verts + 3 * (long)(i0 + max(at, 0));    // list[e] names a vertex < v
            const float qx = q[0], qy = q[1], qz = q[2];
            float best = INFINITY;
            int arg = 0;
            for (int j = g; j < p; j += s_lanes) {
                const float dx = qx - lm_planes[j], dy = qy - lm_planes[p4 + j], dz = qz - lm_planes[2 * p4 + j];
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
            if (g == 0 && at >= 0) value[at] = row_masks[arg];       // arg < p: a slot past p never wins
        }
    } else if (wave * GSPN_WAVE < total) {                           // entry u * LM_THREADS + tid: none for the waves behind
        const float4* X = (const float4*)lm_planes;
        const float4* Y = (const float4*)(lm_planes + p4);
        const float4* Z = (const float4*)(lm_planes + 2 * p4);
        int at[QB];
        float qx[QB], qy[QB], qz[QB], best[QB];
        int arg[QB];
#pragma unroll
        for (int u = 0; u < QB; ++u) {
            const int e = u * LM_THREADS + tid;                      // e < LM_THREADS * QB, the size of list
            at[u] = e < total ? list[e] : -1;
            const float* q = verts + 3 * (long)(i0 + max(at[u], 0));
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
                    if (d < best[u]) {                               // strict: the smallest position among equal distances
                        best[u] = d;
                        arg[u] = 4 * j4 + t;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < QB; ++u)
            if (at[u] >= 0) value[at[u]] = row_masks[arg[u]];
    }
    __syncthreads();

    // every lane back at its own vertices: the order of the additions no longer depends on where the inside vertices lie
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, points = 0.0;
#pragma unroll
    for (int u = 0; u < QB; ++u) {
        const int i = i0 + u * LM_THREADS + tid;
        float g = 0.0f;
        if (in[u]) {                                                 // i < v; the only reads of the tables
            g = value[u * LM_THREADS + tid];
            const int from = min(max(src[i], 0), n - 1);
            const double gd = (double)g;
            s0 += gd;
            s1 += gd * (double)sem_prob[(long)from * c + cls];
            s2 += gd * (double)vert_fb[i];
        }
        const bool set = (double)g > mask_th;                        // :204: a float64 copy of the float32 value against a double
        if (i < v) o[i] = set ? 1 : 0;
        points += set ? 1.0 : 0.0;
    }
    s0 = lm_wave_sum(s0);
    s1 = lm_wave_sum(s1);
    s2 = lm_wave_sum(s2);
    points = lm_wave_sum(points);
    if (lane == 0) {
        red[0][wave] = s0;
        red[1][wave] = s1;
        red[2][wave] = s2;
        red[3][wave] = points;
    }
    __syncthreads();
    if (tid < LM_PART) {
        double t = 0.0;
        for (int w = 0; w < LM_WAVES; ++w) t += red[tid][w];
        slot[tid] = t;
    }
}

// grid r, one wave.  Lane l adds the slots of tiles l, l + 64, ... in ascending order.
__global__ __launch_bounds__(GSPN_WAVE) void lift_finish_kernel(int tiles, int c, const int* __restrict__ class_ids, const double* __restrict__ part,
                                                               double* __restrict__ sem_conf, double* __restrict__ fb_conf,
                                                               int* __restrict__ mask_points) {
    const int ri = blockIdx.x, cls = class_ids[ri];
    double t[LM_PART] = {0.0, 0.0, 0.0, 0.0};
    if (cls > 0 && cls < c) {                                        // uniform
        const double* row = part + (long)ri * tiles * LM_PART;
        for (int k = threadIdx.x; k < tiles; k += GSPN_WAVE)
#pragma unroll
            for (int a = 0; a < LM_PART; ++a) t[a] += row[(long)k * LM_PART + a];
#pragma unroll
        for (int a = 0; a < LM_PART; ++a) t[a] = lm_wave_sum(t[a]);
    }
    if (threadIdx.x == 0) {
        sem_conf[ri] = t[1] / (1e-8 + t[0]);                         // :179; a dropped row: 0 / 1e-8 = 0
        fb_conf[ri] = t[2] / (1e-8 + t[0]);                          // :189
        mask_points[ri] = (int)t[3];                                 // whole numbers up to 2^24: exact
    }
}

// four vertices per lane once that still gives every CU two workgroups; one per lane below
int lm_queries(int r, int v) { return (long)r * ((v + LM_THREADS * 4 - 1) / (LM_THREADS * 4)) >= 512 ? 4 : 1; }
int lm_tiles(int r, int v) {
    const int per = LM_THREADS * lm_queries(r, v);
    return (v + per - 1) / per;
}

}  // namespace

extern "C" long gspn_lift_part_doubles(int r, int v) {
    if (r <= 0 || v <= 0 || r > 65535 || v > LM_MAX_V) return 0;
    return (long)r * lm_tiles(r, v) * LM_PART;
}

extern "C" int gspn_lift_masks(int r, int v, int p, int n, int c, const float* verts, const float* crops, const float* boxes, const float* masks,
                               const int* class_ids, const int* src, const float* sem_prob, const float* vert_fb, double mask_th, double* part,
                               double* sem_conf, double* fb_conf, unsigned char* mask, int* mask_points, void* stream) {
    if (r <= 0 || v <= 0 || p <= 0 || n <= 0 || c <= 0 || !verts || !crops || !boxes || !masks || !class_ids || !src || !sem_prob || !vert_fb ||
        !part || !sem_conf || !fb_conf || !mask || !mask_points || mask_th != mask_th)
        return GSPN_ERR_ARG;
    if (p > LM_MAX_P || r > 65535 || v > LM_MAX_V) return GSPN_ERR_UNSUPPORTED;
    const int p4 = (p + 3) / 4 * 4;
    const size_t lds = (size_t)3 * p4 * sizeof(float);               // <= 48 KiB, beside 8.2 KiB of static LDS
    const int tiles = lm_tiles(r, v);
    hipStream_t st = (hipStream_t)stream;
    if (lm_queries(r, v) == 4)
        lift_masks_kernel<4><<<dim3(tiles, r), LM_THREADS, lds, st>>>(v, p, p4, n, c, verts, crops, boxes, masks, class_ids, src, sem_prob, vert_fb,
                                                                      mask_th, part, mask);
    else
        lift_masks_kernel<1><<<dim3(tiles, r), LM_THREADS, lds, st>>>(v, p, p4, n, c, verts, crops, boxes, masks, class_ids, src, sem_prob, vert_fb,
                                                                      mask_th, part, mask);
    const int rc = gspn_launch_status();
    if (rc != 0) return rc;
    lift_finish_kernel<<<r, GSPN_WAVE, 0, st>>>(tiles, c, class_ids, part, sem_conf, fb_conf, mask_points);
    return gspn_launch_status();
}
