// data_prep.hip -- the segment-to-instance labels of the reference's collect_label (data_prep.py:25-40), additive at ABI 21.  DESIGN.md 4.19.
//
// The reference starts every vertex at -1, walks the (segment, objectId) pairs of segGroups in file order and writes the pair's objectId onto
// every vertex of that segment, printing Error! when one of them already had a label: the last pair of a segment wins.  Here that is a table
// of s segments and a gather:
//   segment_table_init_kernel   winner = -1, named = 0, seen = 0 for every segment; the conflict counter to 0
//   segment_pairs_kernel        one thread per pair: atomicMax of the pair's index into winner[segment], atomicAdd into named[segment]
//   segment_gather_kernel       seg_indices in 16-byte vectors between the first and the last 16-byte boundary, element-wise outside:
//                               label = pair_object[winner[segment]] or -1, and seen[segment] = 1 where the segment has a pair
//   segment_conflicts_kernel    the sum over seen segments of named - 1, reduced per wave, one integer atomicAdd per wave that has any
//
// Integer max and integer sums only: the result is the same in any thread order.  No host synchronisation, nothing allocated, no alignment
// beyond the element's own.
#include "common.h"

#define SL_THREADS 256

namespace {

__global__ __launch_bounds__(SL_THREADS) void segment_table_init_kernel(int s, int* __restrict__ winner, int* __restrict__ named,
                                                                        int* __restrict__ seen, int* __restrict__ conflicts) {
    const int stride = gridDim.x * SL_THREADS;
    for (int i = blockIdx.x * SL_THREADS + threadIdx.x; i < s; i += stride) {
        winner[i] = -1;
        named[i] = 0;
        seen[i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *conflicts = 0;
}

__global__ __launch_bounds__(SL_THREADS) void segment_pairs_kernel(int p, int s, const int* __restrict__ pair_segment, int* __restrict__ winner,
                                                                   int* __restrict__ named) {
    const int stride = gridDim.x * SL_THREADS;
    for (int i = blockIdx.x * SL_THREADS + threadIdx.x; i < p; i += stride) {
        const int seg = pair_segment[i];
        if (seg < 0 || seg >= s) continue;                                        // a segment no vertex can have
        atomicMax(&winner[seg], i);
        atomicAdd(&named[seg], 1);
    }
}

// the label of one vertex; marks its segment as one that has a vertex
__device__ __forceinline__ int label_of(int seg, int s, const int* __restrict__ winner, const int* __restrict__ pair_object, int* __restrict__ seen) {
    if (seg < 0 || seg >= s) return -1;
    const int w = winner[seg];
    if (w < 0) return -1;
    seen[seg] = 1;                                                                // every writer writes the same word
    return pair_object[w];
}

__global__ __launch_bounds__(SL_THREADS) void segment_gather_kernel(int n, int s, const int* __restrict__ seg_indices, const int* __restrict__ winner,
                                                                    const int* __restrict__ pair_object, int* __restrict__ seen,
                                                                    int* __restrict__ out_label) {
    // [0, head): the entries in front of the first 16-byte boundary of seg_indices; [head, head + 4 * vecs): whole vectors; then the tail
    const int head = min(n, (int)(((16 - ((uintptr_t)seg_indices & 15)) & 15) / 4));
    const int vecs = (n - head) / 4;
    const int tail = head + 4 * vecs;
    const bool out_vec = ((uintptr_t)(out_label + head) & 15) == 0;               // uniform
    const int gid = blockIdx.x * SL_THREADS + threadIdx.x;
    const int stride = gridDim.x * SL_THREADS;
    const int4* sv = reinterpret_cast<const int4*>(seg_indices + head);
    for (int v = gid; v < vecs; v += stride) {
        const int4 q = sv[v];
        int4 r;
        r.x = label_of(q.x, s, winner, pair_object, seen);
        r.y = label_of(q.y, s, winner, pair_object, seen);
        r.z = label_of(q.z, s, winner, pair_object, seen);
        r.w = label_of(q.w, s, winner, pair_object, seen);
        int* o = out_label + head + 4 * (long)v;
        if (out_vec) {
            *reinterpret_cast<int4*>(o) = r;
        } else {
            o[0] = r.x;
            o[1] = r.y;
            o[2] = r.z;
            o[3] = r.w;
        }
    }
    if (blockIdx.x == 0) {                                                        // at most 3 + 3 entries
        for (int j = threadIdx.x; j < head; j += SL_THREADS) out_label[j] = label_of(seg_indices[j], s, winner, pair_object, seen);
        for (int j = tail + threadIdx.x; j < n; j += SL_THREADS) out_label[j] = label_of(seg_indices[j], s, winner, pair_object, seen);
    }
}

__global__ __launch_bounds__(SL_THREADS) void segment_conflicts_kernel(int s, const int* __restrict__ named, const int* __restrict__ seen,
                                                                       int* __restrict__ conflicts) {
    const int stride = gridDim.x * SL_THREADS;
    int sum = 0;
    for (int i = blockIdx.x * SL_THREADS + threadIdx.x; i < s; i += stride)
        if (seen[i]) sum += named[i] - 1;                                         // seen implies named >= 1
    sum = wave_sum_lane0(sum);
    if ((threadIdx.x & (GSPN_WAVE - 1)) == 0 && sum) atomicAdd(conflicts, sum);
}

}  // namespace

extern "C" long gspn_segment_labels_ws_bytes(int s) {
    if (s < 1) return GSPN_ERR_ARG;
    if (s > GSPN_SEGMENT_LABELS_MAX_S) return GSPN_ERR_UNSUPPORTED;
    return 3L * s * (long)sizeof(int);
}

extern "C" int gspn_segment_labels(int n, int p, int s, const int* seg_indices, const int* pair_segment, const int* pair_object, void* ws,
                                   int* out_label, int* out_conflicts, void* stream) {
    if (n < 1 || p < 0 || s < 1 || !seg_indices || !pair_segment || !pair_object || !ws || !out_label || !out_conflicts) return GSPN_ERR_ARG;
    if (n > GSPN_SEGMENT_LABELS_MAX_N || s > GSPN_SEGMENT_LABELS_MAX_S) return GSPN_ERR_UNSUPPORTED;
    int* winner = static_cast<int*>(ws);
    int* named = winner + s;
    int* seen = named + s;
    hipStream_t st = (hipStream_t)stream;
    segment_table_init_kernel<<<grid_for(s, SL_THREADS), SL_THREADS, 0, st>>>(s, winner, named, seen, out_conflicts);
    if (p > 0) segment_pairs_kernel<<<grid_for(p, SL_THREADS), SL_THREADS, 0, st>>>(p, s, pair_segment, winner, named);
    segment_gather_kernel<<<grid_for((n + 3) / 4, SL_THREADS), SL_THREADS, 0, st>>>(n, s, seg_indices, winner, pair_object, seen, out_label);
    if (p > 0) segment_conflicts_kernel<<<grid_for(s, SL_THREADS), SL_THREADS, 0, st>>>(s, named, seen, out_conflicts);
    return gspn_launch_status();
}
