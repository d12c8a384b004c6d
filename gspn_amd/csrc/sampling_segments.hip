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
// schemes of sampling.hip, restated here with the (order, c) indirection in their load phase -- sampling.hip is not touched, so the
// kernels of gspn_farthestpointsampling compile to the code they had:
//   fps_seg_small_rounds<C>           256 threads, c <= 512 C,  C = 1..4           (fps_small_kernel)
//   fps_seg_resident_rounds<P, ZLDS>  1024 threads, c <= 1024 P, P = 4, 8, 16, 32  (fps_resident_kernel; z plane in LDS at P = 32)
// Launches on one stream run one after the other, each for as long as its largest instance, so a launch per class costs the SUM of the
// classes' m - 1 rounds: measured 2.40 ms at 2 x 18000, m = 512.  There is instead one launch per workgroup shape -- 256 threads;
// 1024 threads; 1024 threads with the 129 KiB z plane -- and inside it the workgroup's own c selects the instantiation by a scalar branch
// (registers and LDS are those of the largest class of the launch; none spills): 1.26 ms, profiles/instance_sets.txt.  The launcher skips
// a launch no instance can be in (c > m and c <= n), and fps_seg_fill_kernel writes the rows that need no sampling: the background
// (j = 0), empty groups, and c <= m (all members, then draws with replacement from gspn_roi_rand32).
//
// Inside the round loop a pick is stored as its position k, exactly as in sampling.hip; the look-up order[k] would put a global load on the
// serial path of every round.  After the last round the whole workgroup translates the m picks in place and gathers their coordinates.
// Every squared distance goes through dist2_cuda / dist2_cuda_v2 (GSPN_DIST_POLICY).
#include <limits.h>

#include "fps_common.h"
#include "rand32.h"

namespace {

// the instance of workgroup blockIdx.x = scene * g + group
struct Segment {
    const float* xyz;     // the scene's points
    const int* ord;       // L: c scene indices, ascending
    int c;
    int* idx;             // m picks of this instance
    float* pts;           // m x 3
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

// ---- c <= 2048: fps_small_kernel<C> of sampling.hip on a segment.  Thread t, slot p hold the position of tie rank q = t*2C + p, i.e.
//      k = (q % C)*512 + q / C, so "lowest (wave, lane, slot)" is (k mod 512 asc, k asc).
template <int C>
__device__ __forceinline__ void fps_seg_small_rounds(const Segment& sg, int n, int m, int4 (*s_cand)[4], int (*s_k)[4]) {
    constexpr int P = 2 * C;
    const int c = sg.c;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float* xyz = sg.xyz;
    int* o = sg.idx;
    float x[P], y[P], z[P], td[P];
    int kk[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int q = t * P + p;
        const int k = (q % C) * 512 + q / C;
        const int a = seg_point(sg, n, k < c ? k : c - 1);
        kk[p] = k;
        x[p] = xyz[a * 3 + 0]; y[p] = xyz[a * 3 + 1]; z[p] = xyz[a * 3 + 2];
        td[p] = k < c ? 1e38f : -1.0f;        // tf_sampling_g.cu:117-119; padding never wins (real candidates are >= 0)
    }
    if (t == 0) o[0] = 0;                      // :114-116
    const int a0 = seg_point(sg, n, 0);
    float cx = xyz[a0 * 3 + 0], cy = xyz[a0 * 3 + 1], cz = xyz[a0 * 3 + 2];
    for (int j = 1; j < m; ++j) {
        int best = NEG_ONE_BITS, bk = 0;
        float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const float d = dist2_cuda(x[p] - cx, y[p] - cy, z[p] - cz);          // :139-142
            td[p] = vmin_f32(d, td[p]);                                          // :143
            const int v = __float_as_int(td[p]);
            const bool up = v > best;                                             // strict: the lowest slot keeps a tie (:146-149)
            best = up ? v : best;
            bx = up ? x[p] : bx; by = up ? y[p] : by; bz = up ? z[p] : bz;
            bk = up ? kk[p] : bk;
        }
        const int wmax = wave_max_i32(best);
        const int lw = __builtin_ctzll(__ballot(best == wmax));                  // lowest lane on ties
        const int buf = j & 1;
        if (lane == lw) {
            s_cand[buf][wave] = make_int4(wmax, __float_as_int(bx), __float_as_int(by), __float_as_int(bz));
            s_k[buf][wave] = bk;
        }
        __syncthreads();
        const int4 c0 = s_cand[buf][0], c1 = s_cand[buf][1], c2 = s_cand[buf][2], c3 = s_cand[buf][3];
        int w = 0, mv = c0.x;
        if (c1.x > mv) { mv = c1.x; w = 1; }                                      // lowest wave on ties
        if (c2.x > mv) { mv = c2.x; w = 2; }
        if (c3.x > mv) { mv = c3.x; w = 3; }
        const int4 cw = w == 0 ? c0 : (w == 1 ? c1 : (w == 2 ? c2 : c3));
        cx = __int_as_float(cw.y); cy = __int_as_float(cw.z); cz = __int_as_float(cw.w);
        if (t == 0) o[j] = s_k[buf][w];                                          // :166-168
    }
}
// one launch for the four classes: the workgroup's own c picks the instantiation (a wave-uniform branch on a scalar)
__global__ __launch_bounds__(256) void fps_seg_small_kernel(int n, int g, int m, const float* __restrict__ pc, const int* __restrict__ order,
                                                            const int* __restrict__ offsets, int* idx_out, float* __restrict__ pts_out) {
    __shared__ int4 s_cand[2][4];            // {max bits, x, y, z} per wave, double buffered
    __shared__ int s_k[2][4];
    const Segment sg = seg_open(n, g, m, pc, order, offsets, idx_out, pts_out);
    if (!seg_samples(sg, g, m, 0, 2048)) return;
    if (sg.c <= 512) fps_seg_small_rounds<1>(sg, n, m, s_cand, s_k);
    else if (sg.c <= 1024) fps_seg_small_rounds<2>(sg, n, m, s_cand, s_k);
    else if (sg.c <= 1536) fps_seg_small_rounds<3>(sg, n, m, s_cand, s_k);
    else fps_seg_small_rounds<4>(sg, n, m, s_cand, s_k);
    seg_finish(sg, n, m);
}

// ---- c <= 32768: fps_resident_kernel<P, ZLDS> of sampling.hip on a segment (its header explains the scheme).  Thread t = 2*rho + half
//      owns the positions k = (half*P + p)*512 + rho, so the reference tie order (d desc, k mod 512 asc, k asc) is (d desc, t asc, p asc).
template <int P, bool ZLDS>
__device__ __forceinline__ void fps_seg_resident_rounds(const Segment& sg, int n, int m, char* smem) {
    // [0,512)    : candidates, 2 buffers x 16 waves x int4 {max bits, x, y, z}
    // [512,640)  : candidate positions, 2 buffers x 16 waves x int
    // [1024,..)  : z plane, float4 [P/4][1024]   (ZLDS only)
    int4* s_cand = reinterpret_cast<int4*>(smem);
    int* s_k = reinterpret_cast<int*>(smem + 512);
    v4f* s_z = reinterpret_cast<v4f*>(smem + 1024);

    constexpr int G = FpsGroup<P>::G;
    constexpr int NG = FpsGroup<P>::NG;
    static_assert(P % 2 == 0 && (!ZLDS || P % 4 == 0), "P must be even (multiple of 4 with ZLDS)");

    const int c = sg.c;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // provably wave-uniform (keeps loop state in SGPRs)
    const int rho = t >> 1;                       // residue class k mod 512 of this thread
    const int kbase = (t & 1) * P * 512 + rho;    // slot p holds position kbase + p*512
    const float* xyz = sg.xyz;
    int* o = sg.idx;

    v2f x[P / 2], y[P / 2], z[ZLDS ? 1 : P / 2], td[P / 2];
    // clamped, unconditional loads first (all in flight together), masking afterwards
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int k = kbase + p * 512;
        const int a = seg_point(sg, n, k < c ? k : c - 1);
        float px = xyz[a * 3 + 0], py = xyz[a * 3 + 1], pz = xyz[a * 3 + 2];
        const float d0 = k < c ? 1e38f : -1.0f;   // :117-119; padding never wins (real candidates are >= 0)
        px = k < c ? px : 0.f; py = k < c ? py : 0.f; pz = k < c ? pz : 0.f;
        // detach x/y/z from the dwordx3 load tuple so the allocator may place them independently
        asm("" : "+v"(px), "+v"(py), "+v"(pz));
        x[p >> 1][p & 1] = px;
        y[p >> 1][p & 1] = py;
        td[p >> 1][p & 1] = d0;
        if (ZLDS) reinterpret_cast<float*>(s_z)[((p >> 2) * FPS_T + t) * 4 + (p & 3)] = pz;
        else z[p >> 1][p & 1] = pz;
    }
    if (t == 0) o[0] = 0;                          // :114-116
    const int a0 = seg_point(sg, n, 0);
    float cx = xyz[a0 * 3 + 0], cy = xyz[a0 * 3 + 1], cz = xyz[a0 * 3 + 2];   // centre of round 1 = position 0
    __syncthreads();

    for (int j = 1; j < m; ++j) {
        // ---- update min-dist + per-group maxima (value only) ----
        int gmax[NG];
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            int gm = NEG_ONE_BITS;
            v2f zhold = {0.f, 0.f};
#pragma unroll
            for (int h = 0; h < G / 2; ++h) {
                const int pp = (q * G) / 2 + h;            // pair index
                v2f zz;
                if constexpr (ZLDS) {
                    // one ds_read_b128 serves 4 consecutive slots; the empty asm keeps the compiler from narrowing it back into scalar LDS reads
                    if ((h & 1) == 0) {
                        v4f z4 = s_z[(pp >> 1) * FPS_T + t];
                        asm("" : "+v"(z4));
                        zz = z4.xy;
                        zhold = z4.zw;
                    } else {
                        zz = zhold;
                    }
                } else {
                    zz = z[pp];
                }
                const v2f dx = x[pp] - cx, dy = y[pp] - cy, dz = zz - cz;
                const v2f d = dist2_cuda_v2(dx, dy, dz);                                   // contraction policy: fps_common.h, :142
                td[pp][0] = vmin_f32(d[0], td[pp][0]);             // :143
                td[pp][1] = vmin_f32(d[1], td[pp][1]);
                gm = vmax3_i32(gm, __float_as_int(td[pp][0]), __float_as_int(td[pp][1]));
            }
            gmax[q] = gm;
            __builtin_amdgcn_sched_barrier(0);   // keep the scheduler from interleaving groups (VGPR pressure)
        }
        int best = gmax[0];
#pragma unroll
        for (int q = 1; q < NG; ++q) best = max(best, gmax[q]);

        // ---- wave arg-max: value -> lowest lane holding it -> lowest slot inside that lane ----
        int qsel = NG - 1;                         // per lane: first group that holds the lane's best
#pragma unroll
        for (int q = NG - 2; q >= 0; --q) qsel = (gmax[q] == best) ? q : qsel;
        const int wmax = wave_max_i32(best);
        const int lw = __builtin_ctzll(__ballot(best == wmax));
        const int qw = __builtin_amdgcn_readlane(qsel, lw);
        int isel = G - 1;                          // per lane: first slot of group qw equal to the lane's best
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            if (qw == q) {                         // wave-uniform: static register indices inside
#pragma unroll
                for (int i = G - 2; i >= 0; --i) {
                    const int p = q * G + i;
                    isel = (__float_as_int(td[p >> 1][p & 1]) == best) ? i : isel;
                }
            }
        }
        const int iw = __builtin_amdgcn_readlane(isel, lw);
        float fx = 0.f, fy = 0.f, fz = 0.f;
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            if (qw == q) {
#pragma unroll
                for (int i = 0; i < G; ++i) {
                    if (iw == i) {
                        const int p = q * G + i;
                        fx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[p >> 1][p & 1]), lw));
                        fy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y[p >> 1][p & 1]), lw));
                        if (!ZLDS) fz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z[ZLDS ? 0 : (p >> 1)][p & 1]), lw));
                    }
                }
            }
        }
        const int fp = qw * G + iw;
        const int tw = wave * 64 + lw;
        if (ZLDS) fz = reinterpret_cast<const float*>(s_z)[((fp >> 2) * FPS_T + tw) * 4 + (fp & 3)];
        const int buf = (j & 1) * FPS_W;
        if (lane == 0) {
            s_cand[buf + wave] = make_int4(wmax, __float_as_int(fx), __float_as_int(fy), __float_as_int(fz));
            s_k[buf + wave] = ((tw & 1) * P + fp) * 512 + (tw >> 1);
        }
        __syncthreads();

        // ---- workgroup arg-max: every wave reduces the 16 candidates redundantly (lowest wave wins ties)
        const int4 cand = s_cand[buf + (lane & (FPS_W - 1))];
        const int ck = s_k[buf + (lane & (FPS_W - 1))];
        const int M = __builtin_amdgcn_readfirstlane(row_max_i32(cand.x));
        const int wbest = __builtin_ctz((unsigned)(__ballot(cand.x == M) & 0xFFFFull));
        cx = __int_as_float(__builtin_amdgcn_readlane(cand.y, wbest));
        cy = __int_as_float(__builtin_amdgcn_readlane(cand.z, wbest));
        cz = __int_as_float(__builtin_amdgcn_readlane(cand.w, wbest));
        // cross-lane reads stay OUTSIDE the divergent store (a readlane sunk under `if (t == 0)` would let the compiler load s_k for lane 0 only)
        const int kbest = __builtin_amdgcn_readlane(ck, wbest);
        if (t == 0) o[j] = kbest;                                  // :166-168
    }
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
        fps_seg_resident_rounds<32, true>(sg, n, m, smem);
    } else {
        if (sg.c <= 4096) fps_seg_resident_rounds<4, false>(sg, n, m, smem);
        else if (sg.c <= 8192) fps_seg_resident_rounds<8, false>(sg, n, m, smem);
        else fps_seg_resident_rounds<16, false>(sg, n, m, smem);
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
