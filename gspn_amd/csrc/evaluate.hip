// evaluate.hip -- the counting and the matching of the instance AP evaluation (the ScanNet benchmark's evaluate_semantic_instance step, which
// the reference runs after test.py:221-222), additive at ABI 20.  The definition is DESIGN.md 4.18.
//
//   gspn_instance_overlaps  instance_overlaps_kernel: one workgroup per (scene, prediction row).  It walks the row's mask bytes, 16 per lane where
//                           the row's address allows and byte-wise in front of and behind that span, and reads the two label arrays only at set
//                           bytes (masks are about 1 % dense).  A set point whose seg label is the row's class counts into one of g LDS bins by
//                           its group; one whose seg or group label is outside its range counts as void; every set point counts for the row's
//                           size.  gt_count_kernel: one workgroup per scene counts the points of every (class, group) pair in c * g LDS bins.
//   gspn_instance_match     one wave per (scene, threshold, class).  The class's gts are taken one after the other; inside a gt the rows are taken
//                           64 at a time, and the events of the gt are the ballot of the wave: the first set lane of the first non-empty ballot
//                           is the row that becomes visited.  iou and the ignore proportion are double divisions of exact integers, so a
//                           comparison at the boundary agrees with numpy bit for bit.
//
// Integer counts only: exact in any order.  No float atomics, no host synchronisation, nothing allocated, no alignment beyond the element's own.
#include "common.h"

#define IO_THREADS 256
#define GC_THREADS 1024

namespace {

// one set point j of a row of class cls
__device__ __forceinline__ void count_point(int j, int cls, int c, int g, const int* __restrict__ seg, const int* __restrict__ group, int* bins,
                                            int& size, int& void_points) {
    const int s = seg[j], gr = group[j];
    ++size;
    if (s <= 0 || s >= c || gr < 0 || gr >= g)
        ++void_points;
    else if (s == cls)
        atomicAdd(&bins[gr], 1);                                                  // an integer in LDS
}

__global__ __launch_bounds__(IO_THREADS) void instance_overlaps_kernel(int r, int n, int c, int g, const unsigned char* __restrict__ masks,
                                                                       const int* __restrict__ pred_class, const int* __restrict__ seg_label,
                                                                       const int* __restrict__ group_label, int* __restrict__ inter,
                                                                       int* __restrict__ void_count, int* __restrict__ pred_count) {
    extern __shared__ int bins[];                                                 // g bins, then the void counter and the size
    const long row = blockIdx.x;                                                  // scene * r + k
    const long scene = row / r;
    const int cls = pred_class[row];
    int* out = inter + row * g;
    if (cls <= 0 || cls >= c) {                                                   // uniform over the workgroup
        for (int i = threadIdx.x; i < g; i += IO_THREADS) out[i] = 0;
        if (threadIdx.x == 0) {
            void_count[row] = 0;
            pred_count[row] = 0;
        }
        return;
    }
    for (int i = threadIdx.x; i < g + 2; i += IO_THREADS) bins[i] = 0;
    __syncthreads();
    const unsigned char* m = masks + row * n;
    const int* seg = seg_label + scene * (long)n;
    const int* group = group_label + scene * (long)n;
    int size = 0, void_points = 0;
    // [0, head): the bytes in front of the first 16-byte boundary; [head, head + 16 * vecs): whole 16-byte words; the rest byte-wise again
    const int head = min(n, (int)((16 - ((uintptr_t)m & 15)) & 15));
    const int vecs = (n - head) / 16;
    const int tail = head + 16 * vecs;
    for (int j = threadIdx.x; j < head; j += IO_THREADS)
        if (m[j]) count_point(j, cls, c, g, seg, group, bins, size, void_points);
    const uint4* mv = reinterpret_cast<const uint4*>(m + head);
    for (int v = threadIdx.x; v < vecs; v += IO_THREADS) {
        const uint4 q = mv[v];
        if ((q.x | q.y | q.z | q.w) == 0) continue;
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        const int j0 = head + 16 * v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (w[i] == 0) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((w[i] >> (8 * k)) & 0xFFu) count_point(j0 + 4 * i + k, cls, c, g, seg, group, bins, size, void_points);
        }
    }
    for (int j = tail + threadIdx.x; j < n; j += IO_THREADS)
        if (m[j]) count_point(j, cls, c, g, seg, group, bins, size, void_points);
    size = wave_sum_lane0(size);
    void_points = wave_sum_lane0(void_points);
    if ((threadIdx.x & (GSPN_WAVE - 1)) == 0) {
        if (void_points) atomicAdd(&bins[g], void_points);
        if (size) atomicAdd(&bins[g + 1], size);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < g; i += IO_THREADS) out[i] = bins[i];
    if (threadIdx.x == 0) {
        void_count[row] = bins[g];
        pred_count[row] = bins[g + 1];
    }
}

__global__ __launch_bounds__(GC_THREADS) void gt_count_kernel(int n, int c, int g, const int* __restrict__ seg_label,
                                                              const int* __restrict__ group_label, int* __restrict__ gt_count) {
    extern __shared__ int bins[];                                                 // c * g
    const int total = c * g;
    for (int i = threadIdx.x; i < total; i += GC_THREADS) bins[i] = 0;
    __syncthreads();
    const int* seg = seg_label + (long)blockIdx.x * n;
    const int* group = group_label + (long)blockIdx.x * n;
    for (int j = threadIdx.x; j < n; j += GC_THREADS) {
        const int s = seg[j], gr = group[j];
        if (s > 0 && s < c && gr >= 0 && gr < g) atomicAdd(&bins[s * g + gr], 1);
    }
    __syncthreads();
    int* out = gt_count + (long)blockIdx.x * total;
    for (int i = threadIdx.x; i < total; i += GC_THREADS) out[i] = bins[i];
}

#define IM_CHUNKS (GSPN_INSTANCE_MATCH_MAX_R / GSPN_WAVE)

// One wave.  Lane l owns the rows l, l + 64, ...: every per-row array below is read and written by the row's own lane only.
__global__ __launch_bounds__(GSPN_WAVE) void instance_match_kernel(int r, int c, int g, int t, int min_region, const int* __restrict__ inter,
                                                                   const int* __restrict__ void_count, const int* __restrict__ pred_count,
                                                                   const int* __restrict__ pred_class, const float* __restrict__ confidence,
                                                                   const int* __restrict__ count, const int* __restrict__ gt_count,
                                                                   const double* __restrict__ thresholds, int* __restrict__ n_true,
                                                                   int* __restrict__ n_false, int* __restrict__ hard_fn, int* __restrict__ n_gt,
                                                                   int* __restrict__ n_pred) {
    __shared__ int size_of[GSPN_INSTANCE_MATCH_MAX_R];                            // pred_count of a valid row of this class, 0 for every other row
    __shared__ int ignore_of[GSPN_INSTANCE_MATCH_MAX_R];
    __shared__ int trues[GSPN_INSTANCE_MATCH_MAX_R];
    __shared__ int falses[GSPN_INSTANCE_MATCH_MAX_R];
    __shared__ unsigned char visited[GSPN_INSTANCE_MATCH_MAX_R];
    __shared__ unsigned char matched[GSPN_INSTANCE_MATCH_MAX_R];                  // some gt of the class, of any size, overlaps the row above th
    const int s = blockIdx.x % c;
    const int ti = (blockIdx.x / c) % t;
    const int scene = blockIdx.x / c / t;
    const int lane = threadIdx.x;
    const long rows = (long)scene * r;
    int* out_true = n_true + ((long)scene * t + ti) * r;
    int* out_false = n_false + ((long)scene * t + ti) * r;
    if (s == 0) {                                                                 // the rows of no class belong to this wave: they record nothing
        for (int k = lane; k < r; k += GSPN_WAVE) {
            const int cls = pred_class[rows + k];
            if (cls <= 0 || cls >= c) {
                out_true[k] = 0;
                out_false[k] = 0;
            }
        }
        if (lane == 0) {
            hard_fn[((long)scene * t + ti) * c] = 0;
            if (ti == 0) {
                n_gt[(long)scene * c] = 0;
                n_pred[(long)scene * c] = 0;
            }
        }
        return;
    }
    const double th = thresholds[ti];
    const int live = count[scene];
    const int chunks = (r + GSPN_WAVE - 1) / GSPN_WAVE;
    unsigned has_valid = 0;                                                       // bit ch: chunk ch holds a valid row of this class (uniform)
    int valid_rows = 0;
    for (int ch = 0; ch < chunks; ++ch) {
        const int k = ch * GSPN_WAVE + lane;
        int size = 0;
        if (k < r) {
            const int pc = pred_count[rows + k];
            if (k < live && pred_class[rows + k] == s && pc >= min_region) size = pc;
            size_of[k] = size;
            ignore_of[k] = size ? void_count[rows + k] : 0;
            trues[k] = 0;
            falses[k] = 0;
            visited[k] = 0;
            matched[k] = 0;
        }
        const unsigned long long any = __ballot(size > 0);
        if (any) has_valid |= 1u << ch;
        valid_rows += __popcll(any);
    }
    int hard = 0, eligible = 0;
    const int* gts = gt_count + ((long)scene * c + s) * g;
    for (int gi = 0; gi < g; ++gi) {
        const int gc = gts[gi];                                                   // uniform
        if (gc == 0) continue;
        const bool small = gc < min_region;
        if (!small) ++eligible;
        unsigned mine = 0;                                                        // bit ch: this lane's row of chunk ch is an event of the gt
        int first = -1;                                                           // the lowest event row (uniform)
        float best_conf = 0.0f;
        int best_row = -1;                                                        // this lane's event of the largest confidence, the lowest row on a tie
        for (int ch = 0; ch < chunks; ++ch) {
            if (!(has_valid >> ch & 1u)) continue;
            const int k = ch * GSPN_WAVE + lane;
            bool event = false;
            if (k < r && size_of[k] > 0) {
                const int in = inter[(rows + k) * g + gi];
                if (in > 0) {
                    const double iou = (double)in / (double)((long)gc + size_of[k] - in);
                    const bool over = iou > th;
                    if (over) matched[k] = 1;
                    if (small) ignore_of[k] += in;
                    event = over && !small && !visited[k];
                }
            }
            const unsigned long long events = __ballot(event);
            if (events && first < 0) first = ch * GSPN_WAVE + __builtin_ctzll(events);
            if (event) {
                mine |= 1u << ch;
                const float conf = confidence[rows + k];
                if (best_row < 0 || conf > best_conf) {
                    best_conf = conf;
                    best_row = k;
                }
            }
        }
        if (small) continue;
        if (first < 0) {
            ++hard;
            continue;
        }
        if (lane == (first & (GSPN_WAVE - 1))) visited[first] = 1;
        for (int off = GSPN_WAVE / 2; off > 0; off >>= 1) {                       // the holder over the wave: afterwards in lane 0
            const float oc = __shfl_down(best_conf, off, GSPN_WAVE);
            const int orow = __shfl_down(best_row, off, GSPN_WAVE);
            if (orow >= 0 && (best_row < 0 || oc > best_conf || (oc == best_conf && orow < best_row))) {
                best_conf = oc;
                best_row = orow;
            }
        }
        const int holder = __shfl(best_row, 0, GSPN_WAVE);
        while (mine) {
            const int ch = __builtin_ctz(mine);
            mine &= mine - 1;
            const int k = ch * GSPN_WAVE + lane;
            if (k == holder)
                ++trues[k];
            else
                ++falses[k];
        }
    }
    for (int k = lane; k < r; k += GSPN_WAVE) {
        const int size = size_of[k];
        if (size > 0 && !matched[k] && (double)ignore_of[k] / (double)size <= th) ++falses[k];
        if (pred_class[rows + k] == s) {
            out_true[k] = trues[k];
            out_false[k] = falses[k];
        }
    }
    if (lane == 0) {
        hard_fn[((long)scene * t + ti) * c + s] = hard;
        if (ti == 0) {
            n_gt[(long)scene * c + s] = eligible;
            n_pred[(long)scene * c + s] = valid_rows;
        }
    }
}

}  // namespace

extern "C" int gspn_instance_overlaps(int b, int r, int n, int c, int g, const unsigned char* masks, const int* pred_class, const int* seg_label,
                                      const int* group_label, int* inter, int* void_count, int* pred_count, int* gt_count, void* stream) {
    if (b <= 0 || r <= 0 || n <= 0 || c <= 0 || g <= 0 || !masks || !pred_class || !seg_label || !group_label || !inter || !void_count ||
        !pred_count || !gt_count)
        return GSPN_ERR_ARG;
    if (g > GSPN_INSTANCE_MAX_G || (long)c * g > GSPN_INSTANCE_MAX_CG || (long)b * r >= (1L << 31)) return GSPN_ERR_UNSUPPORTED;
    instance_overlaps_kernel<<<(unsigned)((long)b * r), IO_THREADS, (size_t)(g + 2) * sizeof(int), (hipStream_t)stream>>>(
        r, n, c, g, masks, pred_class, seg_label, group_label, inter, void_count, pred_count);
    gt_count_kernel<<<(unsigned)b, GC_THREADS, (size_t)c * g * sizeof(int), (hipStream_t)stream>>>(n, c, g, seg_label, group_label, gt_count);
    return gspn_launch_status();
}

extern "C" int gspn_instance_match(int b, int r, int c, int g, int t, int min_region, const int* inter, const int* void_count,
                                   const int* pred_count, const int* pred_class, const float* confidence, const int* count, const int* gt_count,
                                   const double* thresholds, int* n_true, int* n_false, int* hard_fn, int* n_gt, int* n_pred, void* stream) {
    if (b <= 0 || r <= 0 || c <= 0 || g <= 0 || t <= 0 || !inter || !void_count || !pred_count || !pred_class || !confidence || !count ||
        !gt_count || !thresholds || !n_true || !n_false || !hard_fn || !n_gt || !n_pred)
        return GSPN_ERR_ARG;
    if (r > GSPN_INSTANCE_MATCH_MAX_R || min_region < 1 || (long)b * t * c >= (1L << 31)) return GSPN_ERR_UNSUPPORTED;
    instance_match_kernel<<<(unsigned)((long)b * t * c), GSPN_WAVE, 0, (hipStream_t)stream>>>(
        r, c, g, t, min_region, inter, void_count, pred_count, pred_class, confidence, count, gt_count, thresholds, n_true, n_false, hard_fn, n_gt,
        n_pred);
    return gspn_launch_status();
}
