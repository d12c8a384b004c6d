// fps_rounds.h -- the two on-chip round loops of farthest point sampling, once each, for every kernel that runs a whole cloud in one
// workgroup: fps_small_kernel / fps_resident_kernel (sampling.hip) on a dense scene, fps_seg_small_kernel / fps_seg_resident_kernel
// (sampling_segments.hip) on an instance read through its index list.  Generated code and timing of the four against their former
// private copies: profiles/fps_rounds_shared.txt.
//
// A loop is a template over a point source Src, which is all that differs between the callers:
//   const float* xyz   base of the coordinates, 3 floats per row
//   int c              number of points in the cloud
//   int index(int k)   row of xyz that holds position k, 0 <= k < c
// Position k plays the part of the reference's point index: the first pick is position 0, ties go by (k mod 512 asc, k asc), and a pick
// is stored as its position.
#pragma once
#include "fps_common.h"

// a scene as it lies in memory: position k is row k
struct FpsDense {
    const float* xyz;
    int c;
    __device__ __forceinline__ int index(int k) const { return k; }
};

// ============================================================================================
// Farthest point sampling (reference: tf_sampling_g.cu:105-170)
//
// The reference is m-1 strictly serial rounds of {update the min-dist of all n points, arg-max}.
// It re-reads xyz + the min-dist scratch from L2/global every round (20 B/point/round) and
// spends 10 block barriers per round.  On MI355X a whole 32768-point scene fits ON CHIP in one
// CU, so the resident loop keeps it there for all rounds (zero HBM/L2 traffic in the loop):
//
//   * one 1024-thread workgroup (16 waves, 4 per SIMD) per scene.  Measured on gfx950
//     (tools/valu_probe.hip): one wave issues at most one VALU op per ~5 cycles, a SIMD reaches
//     ~1.27 cycles/op only with 4 waves, and v_pk_*_f32 costs the same issue slot as a scalar
//     op -- hence 16 waves and packed-fp32 math (two points per instruction);
//   * thread t = 2*rho + half owns the points k = (half*P + p)*512 + rho, p = 0..P-1: all of
//     one residue class k mod 512 sits in two adjacent lanes in ascending k, so the reference
//     tie order (d desc, k mod 512 asc, k asc) is simply (d desc, t asc, p asc);
//   * x, y and the running min-dist live in VGPRs (3*P registers); z lives in VGPRs too for
//     P <= 16 and in LDS (128 KiB, read-only, ds_read_b128) for P = 32, which is what lets
//     32768 points fit: 384 KiB of registers + 128 KiB of LDS;
//   * arg-max = integer max on the float bit patterns (all candidates are >= +0, padding is
//     -1.0f, so signed-int order == float order): DPP row reductions inside a wave, one LDS hop
//     across the 16 waves, ONE workgroup barrier per round (double-buffered candidates);
//   * the slot of the maximum is NOT tracked in the hot loop (2 more VALU per point); each wave
//     resolves it afterwards for its best lane only, through per-8-point group maxima that the
//     max3 tree yields for free, wave-uniform switches and v_readlane.
// ============================================================================================

// P = points per thread (even), ZLDS = z plane in LDS instead of VGPRs.  FPS_T threads; o = the m picks; smem = 1024 bytes, plus
// P * FPS_T floats with ZLDS, 16-byte aligned.
template <int P, bool ZLDS, class Src>
__device__ __forceinline__ void fps_resident_rounds(const Src& src, int* o, int m, char* smem) {
    // [0,512)    : candidates, 2 buffers x 16 waves x int4 {max bits, x, y, z}
    // [512,640)  : candidate positions, 2 buffers x 16 waves x int
    // [1024,..)  : z plane, float4 [P/4][1024]   (ZLDS only)
    int4* s_cand = reinterpret_cast<int4*>(smem);
    int* s_k = reinterpret_cast<int*>(smem + 512);
    v4f* s_z = reinterpret_cast<v4f*>(smem + 1024);

    constexpr int G = FpsGroup<P>::G;
    constexpr int NG = FpsGroup<P>::NG;
    static_assert(P % 2 == 0 && (!ZLDS || P % 4 == 0), "P must be even (multiple of 4 with ZLDS)");

    const int c = src.c;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // provably wave-uniform (keeps loop state in SGPRs)
    const int rho = t >> 1;                       // residue class k mod 512 of this thread
    const int kbase = (t & 1) * P * 512 + rho;    // slot p holds position kbase + p*512
    const float* xyz = src.xyz;

    v2f x[P / 2], y[P / 2], z[ZLDS ? 1 : P / 2], td[P / 2];
    // clamped, unconditional loads first (all in flight together), masking afterwards
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int k = kbase + p * 512;
        const int a = src.index(k < c ? k : c - 1);
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
    const int a0 = src.index(0);
    float cx = xyz[a0 * 3 + 0], cy = xyz[a0 * 3 + 1], cz = xyz[a0 * 3 + 2];   // centre of round 1 = position 0
    __syncthreads();

    for (int j = 1; j < m; ++j) {
        // ---- update min-dist + per-group maxima (value only) ----
        int g[NG];
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            int gm = NEG_ONE_BITS;
            v2f zhold = {0.f, 0.f};
#pragma unroll
            for (int h = 0; h < G / 2; ++h) {
                const int pp = (q * G) / 2 + h;            // pair index
                v2f zz;
                if constexpr (ZLDS) {
                    // one ds_read_b128 serves 4 consecutive slots; the empty asm keeps the compiler
                    // from narrowing it back into scalar LDS reads
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
            g[q] = gm;
            __builtin_amdgcn_sched_barrier(0);   // keep the scheduler from interleaving groups (VGPR pressure)
        }
        int best = g[0];
#pragma unroll
        for (int q = 1; q < NG; ++q) best = max(best, g[q]);

        // ---- wave arg-max: value -> lowest lane holding it -> lowest slot inside that lane ----
        int qsel = NG - 1;                         // per lane: first group that holds the lane's best
#pragma unroll
        for (int q = NG - 2; q >= 0; --q) qsel = (g[q] == best) ? q : qsel;
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
        // cross-lane reads stay OUTSIDE the divergent store (a readlane sunk under `if (t == 0)` would
        // let the compiler load s_k for lane 0 only)
        const int kbest = __builtin_amdgcn_readlane(ck, wbest);
        if (t == 0) o[j] = kbest;                                  // :166-168
    }
}

// ============================================================================================
// Small clouds (c <= 2048: the second and third SA level): the same on-chip scheme with FOUR waves instead of sixteen.  A round of
// the resident loop at these sizes is all synchronisation (8 VALU instructions of distance update per wave against a 16-wave
// barrier and a 16-candidate exchange); 256 threads with 2C points each (C = ceil(c/512) <= 4) halve the round time and leave the rest
// of the CU to other workgroups.  Thread t, slot p hold the point of reference tie rank q = t*2C + p, i.e. k = (q % C)*512 + q / C, so
// "lowest (wave, lane, slot)" is again (k mod 512 asc, k asc).  Each lane carries its best slot's coordinates and position along with
// the maximum, so the winner needs no second look-up.
// ============================================================================================
// 256 threads; s_cand = {max bits, x, y, z} per wave, double buffered; s_k = the candidates' positions
template <int C, class Src>
__device__ __forceinline__ void fps_small_rounds(const Src& src, int* o, int m, int4 (*s_cand)[4], int (*s_k)[4]) {
    constexpr int P = 2 * C;
    const int c = src.c;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float* xyz = src.xyz;
    float x[P], y[P], z[P], td[P];
    int kk[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int q = t * P + p;
        const int k = (q % C) * 512 + q / C;
        const int a = src.index(k < c ? k : c - 1);
        kk[p] = k;
        x[p] = xyz[a * 3 + 0]; y[p] = xyz[a * 3 + 1]; z[p] = xyz[a * 3 + 2];
        td[p] = k < c ? 1e38f : -1.0f;        // tf_sampling_g.cu:117-119; padding never wins (real candidates are >= 0)
    }
    if (t == 0) o[0] = 0;                      // :114-116
    const int a0 = src.index(0);
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
