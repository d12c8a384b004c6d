// lift.hip -- predictions on a scan's own vertices (additive at ABI 21): test.py:163-189 and :204 with a vertex of the scan in
// the place of a scene point, for one scan of v vertices (50 000 to over 500 000) and its r detections.
//
//   gspn_lift_masks   gspn_nearest_in_sets (detect.hip) and gspn_scene_confidence (predict.hip) in one pass that never writes the (r, v) index
//                     tensor.  A workgroup per (detection, tile of LM_THREADS * QB vertices) over the in-box nearest-point tile of
//                     inbox_nearest.h, which detect.hip shares: the inside test, the compacted list, the detection's crop points as three
//                     LDS planes, the two walks.  What the kernel adds: a dropped class counts as an empty tile without a box test, and an
//                     empty tile writes its zeros and stages nothing.  The lane that finds a vertex's nearest crop point j leaves
//                     masks[k][j] in the vertex's own LDS slot; behind a barrier every lane is back at its own vertices, in tile order: it
//                     reads sem_prob[src[v]][class] and vert_fb[v] for an inside vertex alone (about one in a hundred), writes every mask
//                     byte of the tile -- zeros outside the box -- and adds its three double terms and its set bytes.  Lanes meet in a
//                     __shfl_down tree, waves through LDS in wave order, and the tile's (S0, S1, S2, count) goes to its own slot of `part`,
//                     also when the tile is empty.
//   lift_finish       one wave per detection adds its tiles' slots in ascending order with a lane stride of 64 and a shuffle tree, and
//                     writes sem_conf, fb_conf and mask_points.
//
// Which lane adds which term, and both orders, depend on (r, v) alone: the same bits on every call.  fp32 distances exactly as the reference
// writes them (-ffp-contract=off), double sums of exact terms, no float atomics, no host synchronisation, nothing allocated.  Row offsets
// are 64-bit: r * v exceeds 2^31.
#include "inbox_nearest.h"

#define LM_THREADS 256
#define LM_WAVES (LM_THREADS / GSPN_WAVE)
#define LM_MAX_P 4096
#define LM_MAX_V (1 << 24)
#define LM_PART 4                                                    // doubles per slot: S0, S1, S2, the set bytes

namespace {

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
        total = inbox_compact<LM_THREADS, QB>(verts, i0, v, lo, hi, in, list, wcnt);
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

    inbox_stage<LM_THREADS>(crops + (long)ri * p * 3, p, p4, lm_planes);
    __syncthreads();
    const float* row_masks = masks + (long)ri * p;
    inbox_walk<LM_THREADS, QB>(verts, i0, lm_planes, p, p4, list, true, total, [&](int at, int arg) { value[at] = row_masks[arg]; });
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
    s0 = wave_sum_lane0(s0);
    s1 = wave_sum_lane0(s1);
    s2 = wave_sum_lane0(s2);
    points = wave_sum_lane0(points);
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
        for (int a = 0; a < LM_PART; ++a) t[a] = wave_sum_lane0(t[a]);
    }
    if (threadIdx.x == 0) {
        sem_conf[ri] = t[1] / (1e-8 + t[0]);                         // :179; a dropped row: 0 / 1e-8 = 0
        fb_conf[ri] = t[2] / (1e-8 + t[0]);                          // :189
        mask_points[ri] = (int)t[3];                                 // whole numbers up to 2^24: exact
    }
}

int lm_tiles(int r, int v) {
    const int per = LM_THREADS * inbox_points_per_lane<LM_THREADS>(r, v);
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
    if (inbox_points_per_lane<LM_THREADS>(r, v) == 4)
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
