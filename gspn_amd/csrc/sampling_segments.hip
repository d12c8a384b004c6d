// sampling_segments.hip -- segmented (ragged) farthest point sampling: every instance of every scene resampled to m points in one fixed
// set of launches (ABI 18).  Reference: dataset.py:107-118, which runs farthestpointsamplingKernel (tf_sampling_g.cu:105-170) once per
// instance at b = 1 on the host-compacted cloud curpc[curgroup == j].
//
// The instances of a scene are the groups of gspn_inverse_lists over its labels: group j holds the points order[offsets[j] .. offsets[j+1])
// in ascending point index, which IS the reference's boolean compaction.  A workgroup per (scene, group) samples the compacted cloud
// L[k] = order[offsets[j] + k], k = 0..c-1: the position k plays the part of the reference's point index (first pick k = 0, ties by
// (k mod 512, k)), and only the results are translated back to scene indices.
//
// The size c of an instance is known on the device alone and nothing is read back, so every launch covers all b*g instances and a
// workgroup with nothing to do in it returns at once (before any barrier).  The size classes are the instantiations of the two on-chip
// round loops of fps_rounds.h, the very code fps_small_kernel and fps_resident_kernel (sampling.hip) run on a dense scene; here they read
// their points through the point source Segment, whose index(k) is the clamped order[k], and that is the only difference:
//   fps_small_rounds<C>           256 threads, c <= 512 C,  C = 1..4
//   fps_resident_rounds<P, ZLDS>  1024 threads, c <= 1024 P, P = 4, 8, 16, 32  (z plane in LDS at P = 32)
// Launches on one stream run one after the other, each for as long as its largest instance, so a launch per class costs the SUM of the
// classes' m - 1 rounds: measured 2.40 ms at 2 x 18000, m = 512.  There is instead one launch per workgroup shape -- 256 threads;
// 1024 threads; 1024 threads with the 129 KiB z plane -- and inside it the workgroup's own c selects the instantiation by a scalar branch
// (registers and LDS are those of the largest class of the launch; none spills): 1.26 ms, profiles/instance_sets.txt.  The launcher skips
// a launch no instance can be in (c > m and c <= n), and fps_seg_fill_kernel writes the rows that need no sampling: the background
// (j = 0), empty groups, and c <= m (all members, then draws with replacement from gspn_roi_rand32).
//
// Inside the round loop a pick is stored as its position k, for a segment as for a dense scene; the look-up order[k] would put a global load on the
// serial path of every round.  After the last round the whole workgroup translates the m picks in place and gathers their coordinates.
// Every squared distance goes through dist2_cuda / dist2_cuda_v2 (GSPN_DIST_POLICY).
#include <limits.h>

#include "fps_rounds.h"
#include "rand32.h"

namespace {

// the instance of workgroup blockIdx.x = scene * g + group; a point source of the round loops (fps_rounds.h)
struct Segment {
    const float* xyz;     // the scene's points
    const int* ord;       // L: c scene indices, ascending
    int c;
    int n;                // points in the scene
    int* idx;             // m picks of this instance
    float* pts;           // m x 3
    __device__ __forceinline__ int index(int k) const;      // seg_point
};

// c = 0 for a run that does not lie inside the scene's n positions (lists not built by gspn_inverse_lists): such a row is written as empty
__device__ __forceinline__ Segment seg_open(int n, int g, int m, const float* pc, const int* order, const int* offsets, int* idx_out, float* pts_out) {
    const int s = blockIdx.x / g, j = blockIdx.x % g;
    const int* off = offsets + (size_t)s * (g + 1);
    const int base = off[j];
    int c = off[j + 1] - base;
    if (base < 0 || c < 0 || base > n - c) c = 0;
    Segment sg;
    sg.xyz = pc + (size_t)s * n * 3;
    sg.ord = order + (size_t)s * n + (c > 0 ? base : 0);
    sg.n = n;
    sg.c = __builtin_amdgcn_readfirstlane(c);          // the same for the whole workgroup: branches on it are scalar
    sg.idx = idx_out + (size_t)blockIdx.x * m;
    sg.pts = pts_out + (size_t)blockIdx.x * m * 3;
    return sg;
}
// the workgroups that sample: not the background, more members than picks, size inside the class (lo, hi]
__device__ __forceinline__ bool seg_samples(const Segment& sg, int g, int m, int lo, int hi) {
    return blockIdx.x % g != 0 && sg.c > m && sg.c > lo && sg.c <= hi;
}
// scene index of compacted position k (clamped: a bad list reads a wrong point, never out of bounds)
__device__ __forceinline__ int seg_point(const Segment& sg, int n, int k) {
    const int a = sg.ord[k];
    return a < 0 ? 0 : (a < n ? a : n - 1);
}
__device__ __forceinline__ int Segment::index(int k) const { return seg_point(*this, n, k); }
// positions -> scene indices and coordinates, by the whole workgroup, after the last round
__device__ __forceinline__ void seg_finish(const Segment& sg, int n, int m) {
    __syncthreads();                                        // thread 0's picks are visible to the workgroup
    for (int j = threadIdx.x; j < m; j += blockDim.x) {
        int k = sg.idx[j];
        k = k < 0 ? 0 : (k < sg.c ? k : sg.c - 1);
        const int a = seg_point(sg, n, k);
        sg.idx[j] = a;
        sg.pts[j * 3 + 0] = sg.xyz[a * 3 + 0];
        sg.pts[j * 3 + 1] = sg.xyz[a * 3 + 1];
        sg.pts[j * 3 + 2] = sg.xyz[a * 3 + 2];
    }
}

// one launch for the four classes: the workgroup's own c picks the instantiation (a wave-uniform branch on a scalar)
__global__ __launch_bounds__(256) void fps_seg_small_kernel(int n, int g, int m, const float* __restrict__ pc, const int* __restrict__ order,
                                                            const int* __restrict__ offsets, int* idx_out, float* __restrict__ pts_out) {
    __shared__ int4 s_cand[2][4];            // {max bits, x, y, z} per wave, double buffered
    __shared__ int s_k[2][4];
    const Segment sg = seg_open(n, g, m, pc, order, offsets, idx_out, pts_out);
    if (!seg_samples(sg, g, m, 0, 2048)) return;
    if (sg.c <= 512) fps_small_rounds<1>(sg, sg.idx, m, s_cand, s_k);
    else if (sg.c <= 1024) fps_small_rounds<2>(sg, sg.idx, m, s_cand, s_k);
    else if (sg.c <= 1536) fps_small_rounds<3>(sg, sg.idx, m, s_cand, s_k);
    else fps_small_rounds<4>(sg, sg.idx, m, s_cand, s_k);
    seg_finish(sg, n, m);
}

// ZLDS = false: one launch for the classes c <= 4096 / 8192 / 16384, picked by the workgroup's own c; ZLDS = true: 16384 < c <= 32768 alone,
// because its 129 KiB of LDS would otherwise be every workgroup's
template <bool ZLDS>
__global__ __launch_bounds__(FPS_T) void fps_seg_resident_kernel(int n, int g, int m, const float* __restrict__ pc, const int* __restrict__ order,
                                                                 const int* __restrict__ offsets, int* idx_out, float* __restrict__ pts_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Segment sg = seg_open(n, g, m, pc, order, offsets, idx_out, pts_out);
    if (!seg_samples(sg, g, m, ZLDS ? 16384 : 2048, ZLDS ? 32768 : 16384)) return;
    if constexpr (ZLDS) {
        fps_resident_rounds<32, true>(sg, sg.idx, m, smem);
    } else {
        if (sg.c <= 4096) fps_resident_rounds<4, false>(sg, sg.idx, m, smem);
        else if (sg.c <= 8192) fps_resident_rounds<8, false>(sg, sg.idx, m, smem);
        else fps_resident_rounds<16, false>(sg, sg.idx, m, smem);
    }
    seg_finish(sg, n, m);
}

// ---- the rows that need no sampling, and count_out of every row.  dataset.py:108-109 (background: zeros), :114-118 (c <= m: the members
//      in order, then m - c draws with replacement -- np.random.choice there, gspn_roi_rand32(seed, scene, group, draw) here).
__global__ __launch_bounds__(256) void fps_seg_fill_kernel(int n, int g, int m, const long long* __restrict__ seed_dev, const float* __restrict__ pc,
                                                           const int* __restrict__ order, const int* __restrict__ offsets, int* __restrict__ idx_out,
                                                           float* __restrict__ pts_out, int* __restrict__ count_out) {
    const Segment sg = seg_open(n, g, m, pc, order, offsets, idx_out, pts_out);
    const int s = blockIdx.x / g, j = blockIdx.x % g, c = sg.c;
    if (threadIdx.x == 0) count_out[blockIdx.x] = c;
    if (j != 0 && c > m) return;                           // a sampling kernel writes this row
    const bool empty = j == 0 || c == 0;
    const unsigned long long st = roi_rand_scene(seed_dev[0], s);
    for (int i = threadIdx.x; i < m; i += blockDim.x) {
        int a = -1;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (!empty) {
            const int k = i < c ? i : (int)(((unsigned long long)roi_rand32(st, (unsigned)j, (unsigned)(i - c)) * (unsigned long long)c) >> 32);
            a = seg_point(sg, n, k);
            px = sg.xyz[a * 3 + 0]; py = sg.xyz[a * 3 + 1]; pz = sg.xyz[a * 3 + 2];
        }
        sg.idx[i] = a;
        sg.pts[i * 3 + 0] = px; sg.pts[i * 3 + 1] = py; sg.pts[i * 3 + 2] = pz;
    }
}

struct SegArgs {
    int blocks, n, g, m;
    const float* pc;
    const int *order, *offsets;
    int* idx_out;
    float* pts_out;
    hipStream_t st;
    // can an instance with more members than picks (c > m) of a scene of n points be in the class (lo, hi]?
    bool reachable(int lo, int hi) const { return lo < n && hi > m; }
};

int launch_seg_small(const SegArgs& a) {
    if (!a.reachable(0, 2048)) return 0;
    hipLaunchKernelGGL(fps_seg_small_kernel, dim3(a.blocks), dim3(256), 0, a.st, a.n, a.g, a.m, a.pc, a.order, a.offsets, a.idx_out, a.pts_out);
    return gspn_launch_status();
}
template <bool ZLDS>
int launch_seg_resident(const SegArgs& a) {
    if (!a.reachable(ZLDS ? 16384 : 2048, ZLDS ? 32768 : 16384)) return 0;
    const size_t lds = 1024 + (ZLDS ? (size_t)32 * FPS_T * sizeof(float) : 0);
    if (ZLDS) {
        const hipError_t e = gspn_dyn_lds_optin<&fps_seg_resident_kernel<ZLDS>>((int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((fps_seg_resident_kernel<ZLDS>), dim3(a.blocks), dim3(FPS_T), lds, a.st, a.n, a.g, a.m, a.pc, a.order, a.offsets, a.idx_out,
                       a.pts_out);
    return gspn_launch_status();
}

int seg_sizes_status(int b, int n, int g, int m) {
    if (b < 0 || n <= 0 || g <= 0 || m <= 0) return GSPN_ERR_ARG;
    if (n > GSPN_FPS_RESIDENT_MAX || (long long)b * g > INT_MAX) return GSPN_ERR_UNSUPPORTED;
    return 0;
}

}  // namespace

// no workspace in this build: the instances are read through `order` in the kernels' load phase
extern "C" long gspn_fps_segments_ws_bytes(int b, int n, int g) { return seg_sizes_status(b, n, g, 1); }

extern "C" int gspn_fps_segments(int b, int n, int g, int m, const long long* seed_dev, const float* pc, const int* order, const int* offsets, void* ws,
                                 int* idx_out, float* pts_out, int* count_out, void* stream) {
    (void)ws;
    const int bad = seg_sizes_status(b, n, g, m);
    if (bad) return bad;
    if (b == 0) return 0;
    if (!seed_dev || !pc || !order || !offsets || !idx_out || !pts_out || !count_out) return GSPN_ERR_ARG;
    const SegArgs a = {b * g, n, g, m, pc, order, offsets, idx_out, pts_out, (hipStream_t)stream};
    hipLaunchKernelGGL(fps_seg_fill_kernel, dim3(a.blocks), dim3(256), 0, a.st, n, g, m, seed_dev, pc, order, offsets, idx_out, pts_out, count_out);
    int rc = gspn_launch_status();
    if (!rc) rc = launch_seg_small(a);
    if (!rc) rc = launch_seg_resident<false>(a);
    if (!rc) rc = launch_seg_resident<true>(a);
    return rc;
}
