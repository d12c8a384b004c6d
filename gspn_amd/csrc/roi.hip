// roi.hip -- the ROI stage of R-PointNet (models/model_rpointnet.py) between the shape proposals and the two heads, ABI 13, behind its first
// step, nms_3d (gspn_nms3d of nms3d.hip).
//   gspn_box_point_count          number of points inside each box (the "remove empty proposals" test of :671-678 and :762-770): the scan of
//                                 gspn_box_shrink (spn_boxes.hip), same shape (BOX_SCAN_* of box_common.h), with a count for accumulator.
//   gspn_sample_points_in_boxes   sample_points_within_box (:584-597) without its (boxes, points) mask matrix: a workgroup per box, every wave
//                                 compacts the inside indices of a contiguous quarter of the points, ascending, into its own LDS region
//                                 (ballot + mbcnt), then draw j looks up rank (rand32 * count) >> 32 across the four regions.
//   gspn_sample_points_in_boxes_seeds  the same kernel with a seed per scene (b of them on the device) in place of one seed and the scene's slot.
//   gspn_detection_target_select  the decisions of detection_target_gen (:662-720) for the whole batch, one workgroup per scene, one lane per
//                                 proposal: IoU against the ground-truth boxes, positive / negative, a random subsample of each by ranking
//                                 32-bit keys.  Integer outputs only; padding rows are skipped in place, so no shape depends on data.
//   gspn_crop_gather_grad         the gradient of points_cropping's gathers (:801-803) through the inverse lists of the sample indices.  The rows
//                                 of negative and padding ROIs are zeros, so point 0 alone is drawn ~11000 times at the training shape: a walk
//                                 of one list by one wave (gspn_sa_group_concat_grad_csr) is bound by that list.  Here the sorted positions are
//                                 cut into chunks of 64, a wave per chunk and 64 channels sums every run inside it, and a second pass adds the
//                                 partial sums of the runs that cross chunks, in chunk order: a fixed order, no atomics.
//
// fp32 throughout, no atomics, no host synchronisation, no allocation.  Compiled with -ffp-contract=off: every bound, volume and IoU below
// is evaluated exactly as the reference writes it.  The random numbers are gspn_roi_rand32 of include/gspn_hip.h.
#include "box_common.h"
#include "rand32.h"          // roi_rand_scene / roi_rand32

#define SM_THREADS 256
#define SM_WAVES (SM_THREADS / GSPN_WAVE)
#define SM_UNROLL 4
#define SM_MAX_N 32768
#define DT_THREADS 1024
#define CG_CHUNK 64

namespace {

// ---------------------------------------------------------------------------------------------------- points inside boxes
// a point is inside when  pc >= (c - s/2) - margin  &&  pc <= (c + s/2) + margin  on all axes (:673-674 with margin 0, :764-765 with 1e-3).
// The two kernels below spell the six compares out where they use them: there the compiler keeps the early exits of the && chain, which
// point_in_box (flattened before it is inlined) does not.
// grid (ceil(s / NB), b).  Boxes past s in the last chunk are counted on a clamped index and not written.
template <int NB>
__global__ __launch_bounds__(BOX_SCAN_THREADS) void box_point_count_kernel(int s, int n, float margin, const float* __restrict__ box,
                                                                           const float* __restrict__ pc, int* __restrict__ count) {
    __shared__ int red[BOX_SCAN_WAVES][NB];
    const int bi = blockIdx.y, s0 = blockIdx.x * NB, tid = threadIdx.x;
    const float* bx = box + (long)bi * s * 6;
    const float* p = pc + (long)bi * n * 3;
    float lo[NB][3], hi[NB][3];
    int cnt[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        box_bounds(bx + (long)min(s0 + k, s - 1) * 6, margin, lo[k], hi[k]);        // uniform across the workgroup: scalar loads
        cnt[k] = 0;
    }
    // a slot past n holds NaN, which is inside no box
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
            for (int k = 0; k < NB; ++k)
                cnt[k] += (x[u] >= lo[k][0] && x[u] <= hi[k][0] && y[u] >= lo[k][1] && y[u] <= hi[k][1] && z[u] >= lo[k][2] && z[u] <= hi[k][2]) ? 1 : 0;
        }
    }
    const int wave = tid / GSPN_WAVE, lane = tid % GSPN_WAVE;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        int v = cnt[k];
#pragma unroll
        for (int o = GSPN_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, GSPN_WAVE);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid < NB && s0 + tid < s) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < BOX_SCAN_WAVES; ++w) v += red[w][tid];
        count[(long)bi * s + s0 + tid] = v;
    }
}

// grid (r, b), SM_THREADS lanes.  Dynamic LDS: SM_WAVES regions of q = ceil(n / SM_WAVES) ints.
// seed_stride 0: one seed for the batch, scene bi draws from the stream (seed_dev[0], bi).  1: a seed per scene, scene bi draws from
// (seed_dev[bi], 0) -- what the scene draws when it is run alone with that seed, whichever slot of the batch it sits in.
__global__ __launch_bounds__(SM_THREADS) void sample_points_kernel(int r, int n, int nsmp, int q, float margin, int seed_stride,
                                                                   const long long* __restrict__ seed_dev, const float* __restrict__ boxes,
                                                                   const float* __restrict__ pc, int* __restrict__ idx_out) {
    extern __shared__ __align__(16) int sm_list[];                   // [SM_WAVES][q]
    __shared__ int wcnt[SM_WAVES];
    const int ri = blockIdx.x, bi = blockIdx.y, tid = threadIdx.x, lane = tid % GSPN_WAVE, wave = tid / GSPN_WAVE;
    const float* bx = boxes + ((long)bi * r + ri) * 6;
    const float* p = pc + (long)bi * n * 3;
    int* o = idx_out + ((long)bi * r + ri) * nsmp;
    const bool zero_row = zero_row6(bx);
    float lo[3], hi[3];
    box_bounds(bx, margin, lo, hi);
    int cnt = 0;                                                     // uniform across the wave
    if (!zero_row) {
        int* list = sm_list + wave * q;
        const int beg = wave * q, end = min(n, beg + q);
        for (int i0 = beg; i0 < end; i0 += GSPN_WAVE * SM_UNROLL) {
            float x[SM_UNROLL], y[SM_UNROLL], z[SM_UNROLL];
#pragma unroll
            for (int u = 0; u < SM_UNROLL; ++u) {
                const int i = i0 + u * GSPN_WAVE + lane;
                const float* g = p + 3 * (long)min(i, n - 1);
                x[u] = i < end ? g[0] : NAN;
                y[u] = g[1];
                z[u] = g[2];
            }
#pragma unroll
            for (int u = 0; u < SM_UNROLL; ++u) {
                const bool in = x[u] >= lo[0] && x[u] <= hi[0] && y[u] >= lo[1] && y[u] <= hi[1] && z[u] >= lo[2] && z[u] <= hi[2];
                const unsigned long long mask = __ballot(in);
                if (in) list[cnt + mbcnt64(mask)] = i0 + u * GSPN_WAVE + lane;       // cnt + hits so far <= points of this quarter <= q
                cnt += __popcll(mask);
            }
        }
    }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    int c[SM_WAVES], total = 0;
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w) {
        c[w] = wcnt[w];
        total += c[w];
    }
    const unsigned long long st = roi_rand_scene(seed_dev[(long)bi * seed_stride], seed_stride ? 0 : bi);
    for (int j = tid; j < nsmp; j += SM_THREADS) {
        int v = 0;                                                   // no inside point, or an all-zero box: a row of zeros (:595)
        if (total > 0) {
            int rank = (int)(((unsigned long long)roi_rand32(st, (unsigned)ri, (unsigned)j) * (unsigned long long)total) >> 32);
            int w = 0;
#pragma unroll
            for (int k = 0; k < SM_WAVES - 1; ++k) {
                if (w == k && rank >= c[k]) {
                    rank -= c[k];
                    w = k + 1;
                }
            }
            v = sm_list[w * q + rank];
        }
        o[j] = v;
    }
}

// ---------------------------------------------------------------------------------------------------- detection targets
// grid (b), one lane per proposal (s <= DT_THREADS)
__global__ __launch_bounds__(DT_THREADS) void detection_target_select_kernel(int s, int g, int rois, int max_positive, float inv_ratio,
                                                                             const long long* __restrict__ seed_dev,
                                                                             const float* __restrict__ proposals, const int* __restrict__ count,
                                                                             const float* __restrict__ gt_boxes, int* __restrict__ roi_src,
                                                                             int* __restrict__ roi_gt) {
    __shared__ unsigned key[DT_THREADS];
    __shared__ int cls[DT_THREADS];                                  // 1 positive, 2 negative, 0 takes no part
    const int bi = blockIdx.x, i = threadIdx.x;
    const float* gb = gt_boxes + (long)bi * g * 6;
    int* src = roi_src + (long)bi * rois;
    int* rgt = roi_gt + (long)bi * rois;
    int mycls = 0, arg = -1;
    unsigned mykey = 0u;
    if (i < s) {
        float p[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) p[a] = proposals[((long)bi * s + i) * 6 + a];
        if (!zero_row6(p) && count[(long)bi * s + i] > 0) {
            float best = -INFINITY;                                  // no ground-truth box: reduce_max over an empty axis, negative
            for (int j = 0; j < g; ++j) {
                const float* q = gb + (long)j * 6;                   // uniform: scalar loads
                if (zero_row6(q)) continue;
                const float v = box_iou(p, q);
                if (v > best) { best = v; arg = j; }                 // strict: the lowest index among equal IoUs (tf.argmax)
            }
            mycls = best >= 0.5f ? 1 : (best < 0.5f ? 2 : 0);
        }
        mykey = roi_rand32(roi_rand_scene(seed_dev[0], bi), (unsigned)i, 0xFFFFFFFFu);
    }
    key[i] = mykey;
    cls[i] = mycls;
    for (int j = i; j < rois; j += DT_THREADS) {
        src[j] = -1;
        rgt[j] = -1;
    }
    __syncthreads();
    // rank among the candidates of the same class by (key, index); every lane also counts both classes
    int rank = 0, npos = 0, nneg = 0;
    for (int j = 0; j < s; ++j) {
        const unsigned kj = key[j];
        const int cj = cls[j];
        npos += cj == 1 ? 1 : 0;
        nneg += cj == 2 ? 1 : 0;
        rank += (cj == mycls && (kj < mykey || (kj == mykey && j < i))) ? 1 : 0;
    }
    npos = min(npos, max_positive);
    nneg = min(nneg, max((int)(inv_ratio * (float)npos) - npos, 0)); // :705-707, the product in fp32, truncated
    if (mycls == 1 && rank < npos && rank < rois) {
        src[rank] = i;
        rgt[rank] = arg;
    } else if (mycls == 2 && rank < nneg && npos + rank < rois) {
        src[npos + rank] = i;
    }
}

// ---------------------------------------------------------------------------------------------------- gradient of the cropping gathers
// order / offsets: the inverse lists of idx (gspn_inverse_lists).  Sorted position e belongs to point idx[order[e]], whose run is
// [offsets[p], offsets[p + 1]).  Chunk t holds the sorted positions [t * CG_CHUNK, (t + 1) * CG_CHUNK).  part (b, chunks, 2, c): slot 0 the
// sum of a run that began before the chunk, slot 1 of a run that goes on after it.
__device__ __forceinline__ float run_sum(const float* __restrict__ gs, const int* __restrict__ ord, int c, int lc, int e0, int e1) {
    float acc = 0.0f;
    int e = e0;
    for (; e + 3 < e1; e += 4) {
        const float v0 = gs[(size_t)ord[e] * c + lc], v1 = gs[(size_t)ord[e + 1] * c + lc];
        const float v2 = gs[(size_t)ord[e + 2] * c + lc], v3 = gs[(size_t)ord[e + 3] * c + lc];
        acc += v0; acc += v1; acc += v2; acc += v3;
    }
    for (; e < e1; ++e) acc += gs[(size_t)ord[e] * c + lc];
    return acc;
}

// grid (chunks, ceil(c / 64), b), one wave each
__global__ __launch_bounds__(GSPN_WAVE) void crop_grad_chunk_kernel(int n, int c, int len, int chunks, const int* __restrict__ idx,
                                                                    const int* __restrict__ order, const int* __restrict__ offsets,
                                                                    const float* __restrict__ grad_out, float* __restrict__ part,
                                                                    float* __restrict__ grad_points) {
    const int t = blockIdx.x, bi = blockIdx.z, l = blockIdx.y * GSPN_WAVE + threadIdx.x, lc = min(l, c - 1);
    const int* off = offsets + (size_t)bi * (n + 1);
    const int* ord = order + (size_t)bi * len;
    const int* ix = idx + (size_t)bi * len;
    const float* gs = grad_out + (size_t)bi * len * c;
    const int e_beg = t * CG_CHUNK, e_end = min(off[n], e_beg + CG_CHUNK);
    int e = e_beg;
    while (e < e_end) {
        const int p = ix[ord[e]];                                    // uniform across the wave
        const int r0 = off[p], r1 = off[p + 1];
        const int run_end = max(min(r1, e_end), e + 1);
        const float acc = run_sum(gs, ord, c, lc, e, run_end);
        if (l < c) {
            if (r0 >= e_beg && r1 <= e_end)
                grad_points[((size_t)bi * n + p) * c + l] = acc;     // the whole run lies in this chunk
            else
                part[(((size_t)bi * chunks + t) * 2 + (r0 >= e_beg ? 1 : 0)) * c + l] = acc;
        }
        e = run_end;
    }
}

// the wave of the chunk in which a crossing run begins adds that run's partial sums in chunk order
__global__ __launch_bounds__(GSPN_WAVE) void crop_grad_join_kernel(int n, int c, int len, int chunks, const int* __restrict__ idx,
                                                                   const int* __restrict__ order, const int* __restrict__ offsets,
                                                                   const float* __restrict__ part, float* __restrict__ grad_points) {
    const int t = blockIdx.x, bi = blockIdx.z, l = blockIdx.y * GSPN_WAVE + threadIdx.x;
    const int* off = offsets + (size_t)bi * (n + 1);
    const int e_beg = t * CG_CHUNK, e_end = min(off[n], e_beg + CG_CHUNK);
    if (e_beg >= e_end || l >= c) return;
    const int p = idx[(size_t)bi * len + order[(size_t)bi * len + e_end - 1]];
    const int r0 = off[p], r1 = off[p + 1];
    if (r1 <= e_end || r0 < e_beg) return;                           // the last run ends here, or began in an earlier chunk
    const float* ps = part + (size_t)bi * chunks * 2 * c + l;
    float acc = ps[((size_t)t * 2 + 1) * c];
    const int t_last = min((r1 - 1) / CG_CHUNK, chunks - 1);
    for (int u = t + 1; u <= t_last; ++u) acc += ps[(size_t)u * 2 * c];
    grad_points[((size_t)bi * n + p) * c + l] = acc;
}

}  // namespace

extern "C" int gspn_box_point_count(int b, int s, int n, float margin, const float* boxes, const float* pc, int* count, void* stream) {
    if (b <= 0 || s <= 0 || n <= 0) return GSPN_ERR_ARG;
    if (b > 65535) return GSPN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    // as gspn_box_shrink: 8 boxes per workgroup once that fills the chip, 4 below
    if ((long)b * ((s + 7) / 8) >= 256)
        box_point_count_kernel<8><<<dim3((s + 7) / 8, b), BOX_SCAN_THREADS, 0, st>>>(s, n, margin, boxes, pc, count);
    else
        box_point_count_kernel<4><<<dim3((s + 3) / 4, b), BOX_SCAN_THREADS, 0, st>>>(s, n, margin, boxes, pc, count);
    return gspn_launch_status();
}

static int sample_points_launch(int b, int r, int n, int nsmp, float margin, int seed_stride, const long long* seed_dev, const float* boxes,
                                const float* pc, int* idx_out, void* stream) {
    if (b <= 0 || r <= 0 || n <= 0 || nsmp <= 0) return GSPN_ERR_ARG;
    if (n > SM_MAX_N || b > 65535) return GSPN_ERR_UNSUPPORTED;
    const int q = (n + SM_WAVES - 1) / SM_WAVES;
    const size_t lds = (size_t)SM_WAVES * q * sizeof(int);
    const hipError_t e = lds > 64 * 1024 ? gspn_dyn_lds_optin<&sample_points_kernel>(SM_MAX_N * (int)sizeof(int)) : hipSuccess;
    if (e != hipSuccess) return (int)e;
    sample_points_kernel<<<dim3(r, b), SM_THREADS, lds, (hipStream_t)stream>>>(r, n, nsmp, q, margin, seed_stride, seed_dev, boxes, pc,
                                                                               idx_out);
    return gspn_launch_status();
}

extern "C" int gspn_sample_points_in_boxes(int b, int r, int n, int nsmp, float margin, const long long* seed_dev, const float* boxes,
                                           const float* pc, int* idx_out, void* stream) {
    return sample_points_launch(b, r, n, nsmp, margin, 0, seed_dev, boxes, pc, idx_out, stream);
}

extern "C" int gspn_sample_points_in_boxes_seeds(int b, int r, int n, int nsmp, float margin, const long long* seeds, const float* boxes,
                                                 const float* pc, int* idx_out, void* stream) {
    return sample_points_launch(b, r, n, nsmp, margin, 1, seeds, boxes, pc, idx_out, stream);
}

extern "C" int gspn_detection_target_select(int b, int s, int g, int rois_per_image, int max_positive, float inv_ratio, const long long* seed_dev,
                                            const float* proposals, const int* count, const float* gt_cls, const float* gt_boxes, int* roi_src,
                                            int* roi_gt, void* stream) {
    (void)gt_cls;                                                    // the reference trims its ground truth by all-zero boxes alone (:664)
    if (b <= 0 || s <= 0 || g <= 0 || rois_per_image <= 0 || max_positive < 0) return GSPN_ERR_ARG;
    if (s > DT_THREADS) return GSPN_ERR_UNSUPPORTED;
    detection_target_select_kernel<<<b, DT_THREADS, 0, (hipStream_t)stream>>>(s, g, rois_per_image, max_positive, inv_ratio, seed_dev, proposals,
                                                                              count, gt_boxes, roi_src, roi_gt);
    return gspn_launch_status();
}

extern "C" long gspn_crop_gather_grad_part_floats(int b, int len, int c) {
    if (b <= 0 || len <= 0 || c <= 0) return 0;
    return (long)b * ((len + CG_CHUNK - 1) / CG_CHUNK) * 2 * c;
}

extern "C" int gspn_crop_gather_grad(int b, int n, int c, int len, const int* idx, const int* order, const int* offsets, const float* grad_out,
                                     float* part, float* grad_points, void* stream) {
    if (b <= 0 || n <= 0 || c <= 0 || len <= 0) return GSPN_ERR_ARG;
    const int chunks = (len + CG_CHUNK - 1) / CG_CHUNK, tiles = (c + GSPN_WAVE - 1) / GSPN_WAVE;
    if (b > 65535 || tiles > 65535) return GSPN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(grad_points, 0, sizeof(float) * (size_t)b * n * c, st);         // the points nothing was gathered from
    if (e != hipSuccess) return (int)e;
    crop_grad_chunk_kernel<<<dim3(chunks, tiles, b), GSPN_WAVE, 0, st>>>(n, c, len, chunks, idx, order, offsets, grad_out, part, grad_points);
    crop_grad_join_kernel<<<dim3(chunks, tiles, b), GSPN_WAVE, 0, st>>>(n, c, len, chunks, idx, order, offsets, part, grad_points);
    return gspn_launch_status();
}
