// spn_boxes.hip -- the box arithmetic of GSPN's shape proposal stage (models/model_rpointnet.py), ABI 12.
//
//   gspn_box_shrink      box_shrink (:529-551): every box scans its scene's points and keeps the min / max of the ones inside.  The reference
//                        broadcasts boxes against points into (B, S, N, 3) temporaries; here a workgroup takes one scene and a chunk of
//                        boxes, its lanes stride over the points, each lane keeps running min / max per box in registers, then a wave
//                        shuffle reduction and one LDS step across the waves.  Nothing but the (B, S, 6) output is written.
//   gspn_points_bbox     per-row bounding box of (rows, m, 3) points, optionally shifted by a per-row offset (:358, :406-408): one wave per row.
//   gspn_spn_target_gen  spn_target_gen (:599-644) for the whole batch in one launch, one workgroup per scene; ground-truth rows with
//                        gt_cls <= 0 are skipped in place, so no shape depends on data.  Two passes over the (never stored) IoU matrix:
//                        row maxima, then column arg-maxima.
//
// fp32 throughout, no atomics, no host synchronisation.  The translation unit is compiled with -ffp-contract=off like the distance kernels
// (common.h): every bound, sum and product below is evaluated exactly as written, nothing is fused.
#include "box_common.h"

#define BX_THREADS 256
#define BX_WAVES (BX_THREADS / GSPN_WAVE)
#define TG_THREADS 1024
#define TG_WAVES (TG_THREADS / GSPN_WAVE)

namespace {

// ---------------------------------------------------------------------------------------------------- box_shrink
// grid (ceil(s / NB), b).  Boxes past s in the last chunk are computed on a clamped index and not written.
template <int NB>
__global__ __launch_bounds__(BOX_SCAN_THREADS) void box_shrink_kernel(int s, int n, const float* __restrict__ box, const float* __restrict__ pc,
                                                                      float* __restrict__ out) {
    __shared__ float red[BOX_SCAN_WAVES][NB][6];
    const int bi = blockIdx.y, s0 = blockIdx.x * NB, tid = threadIdx.x;
    const float* bx = box + (long)bi * s * 6;
    const float* p = pc + (long)bi * n * 3;
    float lo[NB][3], hi[NB][3], mn[NB][3], mx[NB][3];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        box_bounds(bx + (long)min(s0 + k, s - 1) * 6, lo[k], hi[k]);  // uniform across the workgroup: scalar loads
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[k][a] = INFINITY;
            mx[k][a] = -INFINITY;
        }
    }
    // BOX_SCAN_UNROLL points per lane and trip, all their loads issued before the first test: the scan is bound by load latency, not by
    // the compares.  A slot past n holds NaN, which is inside no box.
    for (int i0 = tid; i0 < n; i0 += BOX_SCAN_THREADS * BOX_SCAN_UNROLL) {
        float x[BOX_SCAN_UNROLL], y[BOX_SCAN_UNROLL], z[BOX_SCAN_UNROLL];
#pragma unroll
        for (int u = 0; u < BOX_SCAN_UNROLL; ++u) {
            const int i = i0 + u * BOX_SCAN_THREADS;
            const float* q = p + 3 * (long)min(i, n - 1);
            x[u] = i < n ? q[0] : NAN;
            y[u] = q[1];
            z[u] = q[2];
        }
#pragma unroll
        for (int u = 0; u < BOX_SCAN_UNROLL; ++u) {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const bool in = point_in_box(x[u], y[u], z[u], lo[k], hi[k]);
                mx[k][0] = fmaxf(mx[k][0], in ? x[u] : -INFINITY);
                mx[k][1] = fmaxf(mx[k][1], in ? y[u] : -INFINITY);
                mx[k][2] = fmaxf(mx[k][2], in ? z[u] : -INFINITY);
                mn[k][0] = fminf(mn[k][0], in ? x[u] : INFINITY);
                mn[k][1] = fminf(mn[k][1], in ? y[u] : INFINITY);
                mn[k][2] = fminf(mn[k][2], in ? z[u] : INFINITY);
            }
        }
    }
    const int wave = tid / GSPN_WAVE, lane = tid % GSPN_WAVE;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float vmax = wave_max_f32(mx[k][a]), vmin = wave_min_f32(mn[k][a]);
            if (lane == 0) {
                red[wave][k][a] = vmax;
                red[wave][k][3 + a] = vmin;
            }
        }
    }
    __syncthreads();
    if (tid < NB && s0 + tid < s) {
        float bmax[3], bmin[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            bmax[a] = red[0][tid][a];
            bmin[a] = red[0][tid][3 + a];
#pragma unroll
            for (int w = 1; w < BOX_SCAN_WAVES; ++w) {
                bmax[a] = fmaxf(bmax[a], red[w][tid][a]);
                bmin[a] = fminf(bmin[a], red[w][tid][3 + a]);
            }
        }
        // no point inside: max - min = -inf;  flat on an axis: 0.  Either way the reference's `keep` zeroes the row.
        const bool keep = bmax[0] - bmin[0] > 0.0f && bmax[1] - bmin[1] > 0.0f && bmax[2] - bmin[2] > 0.0f;
        float* o = out + ((long)bi * s + s0 + tid) * 6;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            o[a] = keep ? (bmax[a] + bmin[a]) / 2.0f : 0.0f;
            o[3 + a] = keep ? bmax[a] - bmin[a] + 1e-3f : 0.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- points_bbox
// one wave per row, BX_WAVES rows per workgroup
__global__ __launch_bounds__(BX_THREADS) void points_bbox_kernel(long rows, int m, const float* __restrict__ pts, const float* __restrict__ offset,
                                                                 float* __restrict__ out) {
    const int lane = threadIdx.x % GSPN_WAVE;
    const long r = (long)blockIdx.x * BX_WAVES + threadIdx.x / GSPN_WAVE;
    if (r >= rows) return;                                           // whole waves leave; no barrier below
    const float* p = pts + r * m * 3;
    float off[3] = {0.0f, 0.0f, 0.0f};
    if (offset != nullptr) {
        off[0] = offset[r * 3];
        off[1] = offset[r * 3 + 1];
        off[2] = offset[r * 3 + 2];
    }
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = lane; i < m; i += GSPN_WAVE) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = offset != nullptr ? p[3 * (long)i + a] + off[a] : p[3 * (long)i + a];
            mx[a] = fmaxf(mx[a], v);
            mn[a] = fminf(mn[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mx[a] = wave_max_f32(mx[a]);
        mn[a] = wave_min_f32(mn[a]);
    }
    if (lane == 0) {
        float* o = out + r * 6;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            o[a] = (mx[a] + mn[a]) / 2.0f;
            o[3 + a] = mx[a] - mn[a];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- spn_target_gen
// grid (b), one workgroup per scene
__global__ __launch_bounds__(TG_THREADS) void spn_target_gen_kernel(int s, int g, const float* __restrict__ proposals,
                                                                    const float* __restrict__ seed_cls, const float* __restrict__ gt_cls,
                                                                    const float* __restrict__ gt_boxes, int* __restrict__ spn_match) {
    const int bi = blockIdx.x, tid = threadIdx.x;
    const float* pr = proposals + (long)bi * s * 6;
    const float* sc = seed_cls + (long)bi * s;
    const float* gc = gt_cls + (long)bi * g;
    const float* gb = gt_boxes + (long)bi * g * 6;
    int* match = spn_match + (long)bi * s;
    // pass 1, rows: the largest IoU of each proposal over the valid ground-truth boxes (-inf when there is none: the reference's
    // reduce_max over an empty axis), :626-629 and :640
    for (int i = tid; i < s; i += TG_THREADS) {
        float p[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) p[a] = pr[(long)i * 6 + a];
        float best = -INFINITY;
        for (int j = 0; j < g; ++j) {
            if (!(gc[j] > 0.0f)) continue;
            best = fmaxf(best, box_iou(p, gb + (long)j * 6));
        }
        match[i] = best >= 0.5f ? (sc[i] == 1.0f ? 1 : 0) : -1;
    }
    __syncthreads();          // pass 2 overwrites entries other threads wrote in pass 1
    // pass 2, columns: for each valid ground-truth box the foreground-seed proposal of largest IoU, lowest index on ties (tf.argmax),
    // is positive when that IoU is > 0, :630-638.  One wave per column; several waves may store the same 1 to one entry.
    const int wave = tid / GSPN_WAVE, lane = tid % GSPN_WAVE;
    for (int j = wave; j < g; j += TG_WAVES) {
        if (!(gc[j] > 0.0f)) continue;                               // uniform across the wave
        float q[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) q[a] = gb[(long)j * 6 + a];
        float best = 0.0f;
        int arg = s;                                                 // s: nothing with IoU > 0 yet
        for (int i = lane; i < s; i += GSPN_WAVE) {
            if (sc[i] != 1.0f) continue;
            const float v = box_iou(pr + (long)i * 6, q);
            if (v > best) { best = v; arg = i; }                     // strict: the lowest index of this lane's ties stays
        }
#pragma unroll
        for (int o = GSPN_WAVE / 2; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, GSPN_WAVE);
            const int oa = __shfl_xor(arg, o, GSPN_WAVE);
            if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
        }
        if (lane == 0 && arg < s) match[arg] = 1;
    }
}

}  // namespace

extern "C" int gspn_box_shrink(int b, int s, int n, const float* box, const float* pc, float* out, void* stream) {
    if (b <= 0 || s <= 0 || n <= 0) return GSPN_ERR_ARG;
    if (b > 65535) return GSPN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    // 8 boxes per workgroup once that fills the chip, 4 below (the training shape, 2 x 256 boxes: 128 workgroups instead of 64)
    if ((long)b * ((s + 7) / 8) >= 256)
        box_shrink_kernel<8><<<dim3((s + 7) / 8, b), BOX_SCAN_THREADS, 0, st>>>(s, n, box, pc, out);
    else
        box_shrink_kernel<4><<<dim3((s + 3) / 4, b), BOX_SCAN_THREADS, 0, st>>>(s, n, box, pc, out);
    return gspn_launch_status();
}

extern "C" int gspn_points_bbox(int rows, int m, const float* pts, const float* offset, float* out, void* stream) {
    if (rows <= 0 || m <= 0) return GSPN_ERR_ARG;
    points_bbox_kernel<<<(rows + BX_WAVES - 1) / BX_WAVES, BX_THREADS, 0, (hipStream_t)stream>>>((long)rows, m, pts, offset, out);
    return gspn_launch_status();
}

extern "C" int gspn_spn_target_gen(int b, int s, int g, const float* proposals, const float* seed_cls, const float* gt_cls,
                                   const float* gt_boxes, int* spn_match, void* stream) {
    if (b <= 0 || s <= 0 || g <= 0) return GSPN_ERR_ARG;
    spn_target_gen_kernel<<<b, TG_THREADS, 0, (hipStream_t)stream>>>(s, g, proposals, seed_cls, gt_cls, gt_boxes, spn_match);
    return gspn_launch_status();
}
