// nms3d.hip -- the greedy 3-D non-maximum suppression of R-PointNet (models/model_rpointnet.py): one kernel body, two entry points.
//
//   gspn_nms3d         nms_3d (:436-466), a numpy loop per scene on the host in the reference (ABI 13).  One workgroup per scene, the scene
//                      resident on chip: a bitonic sort of (score, index) in LDS, then the greedy loop -- the first live candidate in score
//                      order is written out, every lane tests its own candidates (bounds and volumes in registers) against it and clears
//                      those with iou > threshold.  The live set is 64 words of bits kept twice in LDS, one read, one written: a barrier per pick.
//   gspn_class_nms3d   the per-class NMS of refine_detections (:855-901, ABI 14), in the reference one nms_3d per class through a py_func.
//                      The same body (PER_CLASS), ONE pass over all candidates in score order: a pick tests only the live candidates of its
//                      class, each of which counts the picks of its class, so a class leaves after max_per_class picks -- or at once after
//                      a pick that survives its own IoU test, which the reference would pick again until the class is full and then collapse
//                      into one row (:893).  The picks come out in descending score, the order of :900.
//
// fp32, no atomics, no host synchronisation, no allocation.  Compiled with -ffp-contract=off: every bound, volume and IoU below is evaluated
// exactly as the reference writes it.
#include "box_common.h"

#define NMS_THREADS 1024
#define NMS_WAVES (NMS_THREADS / GSPN_WAVE)
#define NMS_MAX_N 4096
#define NMS_SLOTS (NMS_MAX_N / NMS_THREADS)
#define NMS_WORDS (NMS_MAX_N / 64)

namespace {

// grid (b), NMS_THREADS lanes, p = n rounded up to a power of two (>= 64).  Dynamic LDS: the live mask twice (2 x 64 words), the sorted
// indices (p ints), PER_CLASS their classes (p ints), then lo[3], hi[3], volume of the sorted candidates (7 x p floats); the sort's 64-bit
// keys lie over the last region.  limit and score_thr are read by the plain instance only, per_class and class_ids by the other.
template <bool PER_CLASS>
__global__ __launch_bounds__(NMS_THREADS) void greedy_nms3d_kernel(int n, int p, int limit, int per_class, int m, float iou_thr, float score_thr,
                                                                   const float* __restrict__ boxes, const float* __restrict__ scores,
                                                                   const int* __restrict__ class_ids, int* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char nms_smem[];
    unsigned long long* alive = (unsigned long long*)nms_smem;                      // [2][NMS_WORDS]
    int* sidx = (int*)(nms_smem + 2 * NMS_WORDS * 8);                              // [p]
    int* scls = sidx + p;                                                          // [p], PER_CLASS only
    float* cb = (float*)(sidx + (PER_CLASS ? 2 : 1) * (size_t)p);                  // [7][p]
    unsigned long long* key = (unsigned long long*)cb;                              // [p], dead before cb is written
    const int bi = blockIdx.x, tid = threadIdx.x, lane = tid % GSPN_WAVE, wave = tid / GSPN_WAVE;
    const float* bx = boxes + (long)bi * n * 6;
    const float* sc = scores + (long)bi * n;
    const int* ci = PER_CLASS ? class_ids + (long)bi * n : nullptr;
    int* o = out + (long)bi * m;

    // ascending 64-bit keys = descending score, lower index first among equal scores (-0 counts as +0, as numpy's argsort of -scores has
    // it); PER_CLASS a row of class <= 0 is no candidate
    for (int k = tid; k < p; k += NMS_THREADS) {
        unsigned long long v = ~0ull;
        if (k < n && (!PER_CLASS || ci[k] > 0)) {
            unsigned u = __float_as_uint(sc[k] + 0.0f);
            u = (u >> 31) ? ~u : (u | 0x80000000u);
            v = ((unsigned long long)(~u) << 32) | (unsigned)k;
        }
        key[k] = v;
    }
    __syncthreads();
    for (int size = 2; size <= p; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < p / 2; t += NMS_THREADS) {
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

    // candidate k = u * NMS_THREADS + tid lives in this lane's registers; bit (k % 64) of word (k / 64) says whether it is still live
    int si[NMS_SLOTS];                                               // its row, -1 (the low half of ~0ull) where there is none
#pragma unroll
    for (int u = 0; u < NMS_SLOTS; ++u) {
        const int k = u * NMS_THREADS + tid;
        si[u] = k < p ? (int)(unsigned)key[k] : -1;
    }
    __syncthreads();                                                 // the keys are dead: cb takes their place
    float lo[NMS_SLOTS][3], hi[NMS_SLOTS][3], vol[NMS_SLOTS];
    int cls[NMS_SLOTS], seen[NMS_SLOTS];                             // PER_CLASS only; seen: the picks of this candidate's class so far
    bool live[NMS_SLOTS];
#pragma unroll
    for (int u = 0; u < NMS_SLOTS; ++u) {
        const int k = u * NMS_THREADS + tid;
        live[u] = false;
        cls[u] = 0;
        seen[u] = 0;
        if (k < p) {
            float q[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (si[u] >= 0) {
#pragma unroll
                for (int a = 0; a < 6; ++a) q[a] = bx[(long)si[u] * 6 + a];
                if (PER_CLASS) cls[u] = ci[si[u]];
                live[u] = PER_CLASS || (k < limit && sc[si[u]] > score_thr);
            }
            box_bounds(q, lo[u], hi[u]);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                cb[a * p + k] = lo[u][a];
                cb[(3 + a) * p + k] = hi[u][a];
            }
            vol[u] = q[3] * q[4] * q[5];
            cb[6 * p + k] = vol[u];
            sidx[k] = si[u];
            if (PER_CLASS) scls[k] = cls[u];
        }
        const unsigned long long mask = __ballot(live[u]);
        if (lane == 0) alive[u * NMS_WAVES + wave] = mask;
    }
    __syncthreads();

    int count = 0;
    for (; count < m; ++count) {
        const unsigned long long* cur = alive + (count & 1) * NMS_WORDS;
        unsigned long long* nxt = alive + ((count + 1) & 1) * NMS_WORDS;
        const unsigned long long nz = __ballot(cur[lane] != 0ull);   // lane l looks at word l: NMS_WORDS == 64
        if (nz == 0ull) break;                                       // every wave reads the same words: uniform
        const int word = __builtin_ctzll(nz);
        const int k0 = word * 64 + __builtin_ctzll(cur[word]);
        float plo[3], phi[3], own[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            plo[a] = cb[a * p + k0];
            phi[a] = cb[(3 + a) * p + k0];
            own[a] = fmaxf(phi[a] - plo[a], 0.0f);                   // PER_CLASS only: min(hi, hi) - max(lo, lo)
        }
        const float pvol = cb[6 * p + k0];
        const int pcls = PER_CLASS ? scls[k0] : 0;
        if (tid == 0) o[count] = sidx[k0];
        // the pick's own test, as its lane evaluates it below: a pick that survives it would be picked until its class is full
        const float own_inter = own[0] * own[1] * own[2];
        const bool exhausted = PER_CLASS && !(own_inter / (((pvol + pvol) - own_inter) + 1e-8f) > iou_thr);
#pragma unroll
        for (int u = 0; u < NMS_SLOTS; ++u) {
            if (live[u] && cls[u] == pcls) {                         // plain: both are 0
                float cube[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) cube[a] = fmaxf(fminf(phi[a], hi[u][a]) - fmaxf(plo[a], lo[u][a]), 0.0f);
                const float inter = cube[0] * cube[1] * cube[2];
                const float iou = inter / (((vol[u] + pvol) - inter) + 1e-8f);
                if (PER_CLASS) ++seen[u];                            // plain: the pick itself leaves only by the IoU test (:464-465)
                if (iou > iou_thr || (PER_CLASS && (exhausted || seen[u] >= per_class))) live[u] = false;
            }
            const unsigned long long mask = __ballot(live[u]);
            if (lane == 0) nxt[u * NMS_WAVES + wave] = mask;
        }
        __syncthreads();
    }
    for (int j = count + tid; j < m; j += NMS_THREADS) o[j] = -1;
}

template <bool PER_CLASS>
int launch_nms3d(int b, int n, int limit, int per_class, int m, float iou_thr, float score_thr, const float* boxes, const float* scores,
                 const int* class_ids, int* selected, void* stream) {
    if (b <= 0 || n <= 0 || m <= 0 || (PER_CLASS && per_class <= 0)) return GSPN_ERR_ARG;
    if (n > NMS_MAX_N) return GSPN_ERR_UNSUPPORTED;
    int p = 64;
    while (p < n) p <<= 1;
    const int row = PER_CLASS ? 36 : 32;                             // bytes of dynamic LDS per sorted candidate
    const size_t lds = 2 * NMS_WORDS * 8 + (size_t)p * row;
    const hipError_t e = lds > 64 * 1024 ? gspn_dyn_lds_optin<&greedy_nms3d_kernel<PER_CLASS>>(2 * NMS_WORDS * 8 + NMS_MAX_N * row) : hipSuccess;
    if (e != hipSuccess) return (int)e;
    greedy_nms3d_kernel<PER_CLASS><<<b, NMS_THREADS, lds, (hipStream_t)stream>>>(n, p, limit, per_class, m, iou_thr, score_thr, boxes, scores,
                                                                                class_ids, selected);
    return gspn_launch_status();
}

}  // namespace

extern "C" int gspn_nms3d(int b, int n, int pre_nms_limit, int max_output_size, float iou_threshold, float score_threshold, const float* boxes,
                          const float* scores, int* selected, void* stream) {
    const int limit = pre_nms_limit > 0 ? min(pre_nms_limit, n) : n;
    return launch_nms3d<false>(b, n, limit, 0, max_output_size, iou_threshold, score_threshold, boxes, scores, nullptr, selected, stream);
}

extern "C" int gspn_class_nms3d(int b, int n, int max_per_class, int max_output_size, float iou_threshold, const float* boxes, const float* scores,
                                const int* class_ids, int* selected, void* stream) {
    return launch_nms3d<true>(b, n, 0, max_per_class, max_output_size, iou_threshold, 0.0f, boxes, scores, class_ids, selected, stream);
}
