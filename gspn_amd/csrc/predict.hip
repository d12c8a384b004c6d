// predict.hip -- the arithmetic of the prediction export stage, ABI 19.  Reference: test.py:155-205 (per-scene instance masks with a label id
// and a confidence each) and train.py:365-368, 385-386 (the semantic IoU counts of an evaluation pass).
//
// The reference works on the host, one detection at a time: a ball tree per detection (:165), a (ND, N) float64 matrix of mask values
// (:163), its product with the (N, NC) softmax table (:178) and two argsorts (:194-197).  gspn_nearest_in_sets (detect.hip) already
// replaces the ball trees by one launch that writes (B, R, N) indices; what follows reads those indices and never writes the float matrix.
//
//   gspn_scene_confidence   one workgroup per (scene, detection).  Thread t walks the points t, t + SC_THREADS, ... in ascending order and
//                           adds g, g * sem_prob[class] and g * point_fb in double (each float product is widened first, so every term
//                           is exact); the lanes of a wave are added by a shuffle tree, the waves through LDS in wave order.  Which terms a
//                           thread takes and both orders depend on the shape alone, so the bits repeat from call to call.  The same walk
//                           writes the thresholded mask, one byte per point, and counts its set bytes.
//   gspn_scene_rank         one workgroup per scene.  The keys (group, score) of the R rows sit in LDS; every row counts the rows that go
//                           before it, which is its output position.  R <= 1024: R * R / 256 LDS reads per thread, all of them broadcasts.
//   gspn_sem_iou_counts     one thread per row takes the first maximal column, the workgroup counts per class in LDS and adds its non-zero
//                           counts to the caller's int64 accumulators, one integer atomic per class.  Integers: exact in any order.
//
// No float atomics, no host synchronisation, nothing allocated.  No alignment beyond the element's own.
#include "common.h"

#define SC_THREADS 256
#define SR_THREADS 256
#define SI_THREADS 256

namespace {

__global__ __launch_bounds__(SC_THREADS) void scene_confidence_kernel(int r, int n, int p, int c, const int* __restrict__ idx,
                                                                      const float* __restrict__ masks, const int* __restrict__ class_ids,
                                                                      const float* __restrict__ sem_prob, const float* __restrict__ point_fb,
                                                                      double mask_th, double* __restrict__ sem_conf,
                                                                      double* __restrict__ fb_conf, unsigned char* __restrict__ mask,
                                                                      int* __restrict__ mask_points) {
    constexpr int WAVES = SC_THREADS / GSPN_WAVE;
    __shared__ double red[3][WAVES];
    __shared__ int red_points[WAVES];
    const long row = blockIdx.x;                                                  // scene * r + k
    const long scene = row / r;
    const int cls = class_ids[row];
    unsigned char* out_mask = mask + row * n;
    if (cls <= 0 || cls >= c) {                                                   // a row test.py:159-161 drops (uniform over the workgroup)
        for (int j = threadIdx.x; j < n; j += SC_THREADS) out_mask[j] = 0;
        if (threadIdx.x == 0) {
            sem_conf[row] = 0.0;
            fb_conf[row] = 0.0;
            mask_points[row] = 0;
        }
        return;
    }
    const int* row_idx = idx + row * n;
    const float* row_masks = masks + row * p;
    const float* sem_col = sem_prob + scene * (long)n * c + cls;
    const float* fb = point_fb + scene * (long)n;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int points = 0;
    for (int j = threadIdx.x; j < n; j += SC_THREADS) {
        const int at = row_idx[j];
        float g = 0.0f;
        if (at >= 0) {                                                            // about one point in a hundred: the only reads of the tables
            g = row_masks[min(at, p - 1)];
            const double gd = (double)g;
            s0 += gd;
            s1 += gd * (double)sem_col[(long)j * c];
            s2 += gd * (double)fb[j];
        }
        const bool set = (double)g > mask_th;                                     // :204: a float64 copy of the float32 value against a double
        out_mask[j] = set ? 1 : 0;
        points += set ? 1 : 0;
    }
    s0 = wave_sum_lane0(s0);
    s1 = wave_sum_lane0(s1);
    s2 = wave_sum_lane0(s2);
    points = wave_sum_lane0(points);
    const int wave = threadIdx.x / GSPN_WAVE;
    if ((threadIdx.x & (GSPN_WAVE - 1)) == 0) {
        red[0][wave] = s0;
        red[1][wave] = s1;
        red[2][wave] = s2;
        red_points[wave] = points;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        int total = 0;
        for (int w = 0; w < WAVES; ++w) {
            t0 += red[0][w];
            t1 += red[1][w];
            t2 += red[2][w];
            total += red_points[w];
        }
        sem_conf[row] = t1 / (1e-8 + t0);                                         // :179
        fb_conf[row] = t2 / (1e-8 + t0);                                          // :189
        mask_points[row] = total;
    }
}

// row a goes before row b: (group ascending, score descending, row ascending); the keys hold no NaN
__device__ __forceinline__ bool goes_before(int ga, double sa, int a, int gb, double sb, int b) {
    if (ga != gb) return ga < gb;
    if (sa != sb) return sa > sb;
    return a < b;
}

__global__ __launch_bounds__(SR_THREADS) void scene_rank_kernel(int r, int c, const float* __restrict__ det_score,
                                                                const int* __restrict__ class_ids, const double* __restrict__ sem_conf,
                                                                const double* __restrict__ fb_conf, double sem_th, double fb_th,
                                                                const int* __restrict__ label_map, int* __restrict__ order,
                                                                int* __restrict__ count, int* __restrict__ label_ids,
                                                                float* __restrict__ confidence, double* __restrict__ score) {
    __shared__ double key[GSPN_SCENE_RANK_MAX_R];
    __shared__ double value[GSPN_SCENE_RANK_MAX_R];
    __shared__ int group[GSPN_SCENE_RANK_MAX_R];
    __shared__ int live;
    const long base = (long)blockIdx.x * r;
    if (threadIdx.x == 0) live = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < r; k += SR_THREADS) {
        const int cls = class_ids[base + k];
        int g = 2;
        double s = 0.0;
        if (cls > 0 && cls < c) {
            const double sc = sem_conf[base + k], fc = fb_conf[base + k];
            s = ((double)det_score[base + k] * sc) * fc;                          // :194
            g = (sc > sem_th && fc > fb_th) ? 0 : 1;                              // :192-193
            atomicAdd(&live, 1);                                                  // an integer in LDS
        }
        group[k] = g;
        value[k] = s;
        key[k] = s != s ? -__builtin_huge_val() : s;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < r; k += SR_THREADS) {
        const int g = group[k];
        const double s = key[k];
        int at = 0;
        for (int j = 0; j < r; ++j) at += goes_before(group[j], key[j], j, g, s, k) ? 1 : 0;
        const int cls = class_ids[base + k];
        order[base + at] = k;
        label_ids[base + at] = g == 2 ? 0 : label_map[cls];                       // :205
        confidence[base + at] = g == 0 ? 1.0f : (g == 1 ? 0.97f : 0.0f);          // :202
        score[base + at] = value[k];
    }
    if (threadIdx.x == 0) count[blockIdx.x] = live;
}

__global__ __launch_bounds__(SI_THREADS) void sem_iou_counts_kernel(long rows, int c, const float* __restrict__ logits,
                                                                    const int* __restrict__ labels, unsigned long long* __restrict__ inter,
                                                                    unsigned long long* __restrict__ uni) {
    __shared__ int hit[GSPN_SEM_IOU_MAX_C];                                       // [s]: pred == s and label == s
    __shared__ int any[GSPN_SEM_IOU_MAX_C];                                       // [s]: pred == s or label == s
    for (int s = threadIdx.x; s < c; s += SI_THREADS) {
        hit[s] = 0;
        any[s] = 0;
    }
    __syncthreads();
    for (long row = (long)blockIdx.x * SI_THREADS + threadIdx.x; row < rows; row += (long)gridDim.x * SI_THREADS) {
        const float* x = logits + row * c;
        float best = x[0];
        int pred = 0;
        for (int s = 1; s < c; ++s) {
            const float v = x[s];
            if (v > best) {                                                       // strictly: the first maximum stays (np.argmax)
                best = v;
                pred = s;
            }
        }
        const int label = labels[row];
        if (pred > 0) {
            atomicAdd(&any[pred], 1);
            if (label == pred) atomicAdd(&hit[pred], 1);
        }
        if (label > 0 && label < c && label != pred) atomicAdd(&any[label], 1);
    }
    __syncthreads();
    for (int s = 1 + threadIdx.x; s < c; s += SI_THREADS) {
        if (hit[s]) atomicAdd(&inter[s - 1], (unsigned long long)hit[s]);
        if (any[s]) atomicAdd(&uni[s - 1], (unsigned long long)any[s]);
    }
}

}  // namespace

extern "C" int gspn_scene_confidence(int b, int r, int n, int p, int c, const int* idx, const float* masks, const int* class_ids,
                                     const float* sem_prob, const float* point_fb, double mask_th, double* sem_conf, double* fb_conf,
                                     unsigned char* mask, int* mask_points, void* stream) {
    if (b <= 0 || r <= 0 || n <= 0 || p <= 0 || c <= 0 || !idx || !masks || !class_ids || !sem_prob || !point_fb || !sem_conf || !fb_conf ||
        !mask || !mask_points || mask_th != mask_th)
        return GSPN_ERR_ARG;
    if ((long)b * r >= (1L << 31)) return GSPN_ERR_UNSUPPORTED;
    scene_confidence_kernel<<<(unsigned)((long)b * r), SC_THREADS, 0, (hipStream_t)stream>>>(r, n, p, c, idx, masks, class_ids, sem_prob, point_fb,
                                                                                            mask_th, sem_conf, fb_conf, mask, mask_points);
    return gspn_launch_status();
}

extern "C" int gspn_scene_rank(int b, int r, int c, const float* det_score, const int* class_ids, const double* sem_conf, const double* fb_conf,
                               double sem_th, double fb_th, const int* label_map, int* order, int* count, int* label_ids, float* confidence,
                               double* score, void* stream) {
    if (b <= 0 || r <= 0 || c <= 0 || !det_score || !class_ids || !sem_conf || !fb_conf || !label_map || !order || !count || !label_ids ||
        !confidence || !score || sem_th != sem_th || fb_th != fb_th)
        return GSPN_ERR_ARG;
    if (r > GSPN_SCENE_RANK_MAX_R) return GSPN_ERR_UNSUPPORTED;
    scene_rank_kernel<<<(unsigned)b, SR_THREADS, 0, (hipStream_t)stream>>>(r, c, det_score, class_ids, sem_conf, fb_conf, sem_th, fb_th, label_map,
                                                                          order, count, label_ids, confidence, score);
    return gspn_launch_status();
}

extern "C" int gspn_sem_iou_counts(long rows, int c, const float* logits, const int* labels, long long* inter, long long* uni, void* stream) {
    if (rows <= 0 || c < 2 || !logits || !labels || !inter || !uni) return GSPN_ERR_ARG;
    if (c > GSPN_SEM_IOU_MAX_C) return GSPN_ERR_UNSUPPORTED;
    sem_iou_counts_kernel<<<grid_for(rows, SI_THREADS), SI_THREADS, 0, (hipStream_t)stream>>>(
        rows, c, logits, labels, reinterpret_cast<unsigned long long*>(inter), reinterpret_cast<unsigned long long*>(uni));
    return gspn_launch_status();
}
