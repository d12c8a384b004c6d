// tile_linear.hip -- the broadcast add and the per-group sum behind a linear layer over concat(tile(global), local), ABI 17.
//
// segmentation_head (models/model_rpointnet.py:966-970) tiles each ROI's global feature over its p points, appends the per-point features
// and runs a linear layer over the concatenation.  The layer is linear, so it splits:
//     y[g * p + j, :] = local[g * p + j, :] . W[cg:]  +  (global[g, :] . W[:cg] + bias)
// two GEMMs (gspn_mlp_fwd), one over the groups * p rows and one over the groups, and what is left is
//
//   gspn_tile_add   Y[g * p + j, :] = A[g * p + j, :] + G[g, :].  A workgroup takes one group and a run of its rows.  LANES = the smallest
//                   power of two >= c / 4 lanes share a row, one float4 each, and keep their float4 of G[g] in registers for the whole run: a
//                   wave reads its G row once.  The TL_THREADS / LANES row groups walk the run with that stride.  One add per element: the bits
//                   of the fp32 broadcast add.  Y may be A (every element is read and written by the same thread).
//   gspn_tile_sum   dG[g, :] = sum_j dY[g * p + j, :], the transpose.  Same lanes; every thread adds its rows in double in ascending order, the
//                   row groups are added through LDS in group order and the sum is rounded to float once (crop_mean's scheme).  With few
//                   groups, a group's rows are cut into `parts` runs, one workgroup each, so that the chip is filled; every workgroup then
//                   writes its sum as doubles into the workspace and a second kernel adds the parts in part order in double
//                   (gspn_crop_linear_bwd_side's join).  No atomics; the rows a thread takes, `parts` and both orders depend on the shape
//                   alone, so the bits repeat, and p equal rows give p * row exactly when p is a power of two.
//
// c a multiple of 4 and <= 1024, groups * p < 2^31, every pointer 16-byte aligned: GSPN_ERR_UNSUPPORTED otherwise, before any launch.
#include "common.h"

#define TL_THREADS 256
#define TL_MAX_C 1024                   // GSPN_MLP_MAX_CHANNELS: at most one float4 per thread of a workgroup
#define TL_ADD_STEPS 8                  // rows a row group adds per workgroup of gspn_tile_add
#define TL_SUM_MIN_ROWS 64              // gspn_tile_sum: a part is at least this many rows ...
#define TL_SUM_BLOCKS 512               // ... and a group is cut only while that leaves at most this many workgroups

namespace {

__device__ __forceinline__ float4 tl_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void tl_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// blockIdx.x = g * runs + run; A and Y may alias
__global__ __launch_bounds__(TL_THREADS) void tile_add_kernel(int p, int c, int lanes_log2, int runs, int run_rows, const float* A,
                                                              const float* __restrict__ G, float* Y) {
    const int lanes = 1 << lanes_log2, groups = TL_THREADS >> lanes_log2;
    const int col = (threadIdx.x & (lanes - 1)) * 4, rg = threadIdx.x >> lanes_log2;
    if (col >= c) return;
    const long g = blockIdx.x / runs;
    const long j0 = (long)(blockIdx.x % runs) * run_rows;
    const long j1 = min(j0 + run_rows, (long)p);
    const float4 gv = tl_ld4(G + (size_t)g * c + col);
    for (long j = j0 + rg; j < j1; j += groups) {
        const size_t at = ((size_t)g * p + j) * c + col;
        const float4 a = tl_ld4(A + at);
        tl_st4(Y + at, make_float4(a.x + gv.x, a.y + gv.y, a.z + gv.z, a.w + gv.w));
    }
}

// blockIdx.x = g * parts + part.  parts == 1: dG (groups, c) is written; otherwise part_out (groups, parts, c) doubles.
__global__ __launch_bounds__(TL_THREADS) void tile_sum_kernel(int p, int c, int lanes_log2, int parts, int part_rows,
                                                              const float* __restrict__ dY, float* __restrict__ dG,
                                                              double* __restrict__ part_out) {
    __shared__ double red[TL_THREADS * 4];                                        // [row group][lane][4]
    const int lanes = 1 << lanes_log2, groups = TL_THREADS >> lanes_log2;
    const int lane = threadIdx.x & (lanes - 1), rg = threadIdx.x >> lanes_log2;
    const int col = lane * 4;
    const bool live = col < c;
    const long g = blockIdx.x / parts;
    const int part = (int)(blockIdx.x % parts);
    const long j0 = min((long)part * part_rows, (long)p);
    const long j1 = min(j0 + part_rows, (long)p);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (live) {
        const float* src = dY + (size_t)g * p * c + col;
#pragma unroll 4
        for (long j = j0 + rg; j < j1; j += groups) {
            const float4 d = tl_ld4(src + (size_t)j * c);
            s0 += (double)d.x, s1 += (double)d.y, s2 += (double)d.z, s3 += (double)d.w;
        }
    }
    double* mine = red + (size_t)threadIdx.x * 4;
    mine[0] = s0, mine[1] = s1, mine[2] = s2, mine[3] = s3;
    __syncthreads();
    if (rg == 0 && live) {                                                        // over the row groups, in group order
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int u = 0; u < groups; ++u) {
            const double* r = red + ((size_t)(u << lanes_log2) + lane) * 4;
            t[0] += r[0], t[1] += r[1], t[2] += r[2], t[3] += r[3];
        }
        if (parts == 1) {
            tl_st4(dG + (size_t)g * c + col, make_float4((float)t[0], (float)t[1], (float)t[2], (float)t[3]));
        } else {
            double* o = part_out + ((size_t)g * parts + part) * c + col;
            o[0] = t[0], o[1] = t[1], o[2] = t[2], o[3] = t[3];
        }
    }
}

// part (groups, parts, c) doubles -> dG (groups, c): the parts of a group added in part order, in double, rounded once
__global__ __launch_bounds__(TL_THREADS) void tile_sum_join_kernel(long total, int c, int parts, const double* __restrict__ part,
                                                                   float* __restrict__ dG) {
    const long e = (long)blockIdx.x * TL_THREADS + threadIdx.x;                   // g * c + column
    if (e >= total) return;
    const long g = e / c;
    const int col = (int)(e % c);
    const double* src = part + (size_t)g * parts * c + col;
    double sum = 0.0;
    for (int u = 0; u < parts; ++u) sum += src[(size_t)u * c];
    dG[e] = (float)sum;
}

inline int tl_lanes_log2(int c) {
    int l = 0;
    while ((4 << l) < c) ++l;
    return l;
}

// sizes every entry point checks the same way: 0 when they are fine
inline int tl_check_sizes(long groups, int p, int c) {
    if (groups <= 0 || p <= 0 || c <= 0) return GSPN_ERR_ARG;
    if (c % 4 || c > TL_MAX_C || groups >= (1L << 31) || groups * p >= (1L << 31)) return GSPN_ERR_UNSUPPORTED;
    return 0;
}

inline bool tl_aligned16(const void* a, const void* b, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16) == 0;
}

// the runs a group's p rows are cut into by gspn_tile_sum: a function of the shape alone
inline int tl_sum_parts(long groups, int p) {
    long parts = TL_SUM_BLOCKS / groups;
    const long most = ((long)p + TL_SUM_MIN_ROWS - 1) / TL_SUM_MIN_ROWS;
    if (parts > most) parts = most;
    return parts < 1 ? 1 : (int)parts;
}

}  // namespace

extern "C" int gspn_tile_add(long groups, int p, int c, const float* A, const float* G, float* Y, void* stream) {
    const int bad = tl_check_sizes(groups, p, c);
    if (bad) return bad;
    if (!A || !G || !Y) return GSPN_ERR_ARG;
    if (!tl_aligned16(A, G, Y)) return GSPN_ERR_UNSUPPORTED;
    const int lanes_log2 = tl_lanes_log2(c);
    const int run_rows = (TL_THREADS >> lanes_log2) * TL_ADD_STEPS;
    const int runs = (p + run_rows - 1) / run_rows;                               // groups * runs <= groups * p < 2^31
    tile_add_kernel<<<(unsigned)(groups * runs), TL_THREADS, 0, (hipStream_t)stream>>>(p, c, lanes_log2, runs, run_rows, A, G, Y);
    return gspn_launch_status();
}

extern "C" long gspn_tile_sum_part_floats(long groups, int p, int c) {
    if (tl_check_sizes(groups, p, c)) return 0;
    const int parts = tl_sum_parts(groups, p);
    return parts == 1 ? 0 : 2 * groups * parts * c;                               // doubles, counted in floats
}

extern "C" int gspn_tile_sum(long groups, int p, int c, const float* dY, float* part, float* dG, void* stream) {
    const int bad = tl_check_sizes(groups, p, c);
    if (bad) return bad;
    const int parts = tl_sum_parts(groups, p);
    if (!dY || !dG || (parts > 1 && !part)) return GSPN_ERR_ARG;
    if (!tl_aligned16(dY, dG, part)) return GSPN_ERR_UNSUPPORTED;
    const int lanes_log2 = tl_lanes_log2(c);
    const int part_rows = (p + parts - 1) / parts;
    hipStream_t st = (hipStream_t)stream;
    tile_sum_kernel<<<(unsigned)(groups * parts), TL_THREADS, 0, st>>>(p, c, lanes_log2, parts, part_rows, dY, dG, (double*)part);
    if (parts > 1) {
        const long total = groups * c;
        tile_sum_join_kernel<<<(unsigned)((total + TL_THREADS - 1) / TL_THREADS), TL_THREADS, 0, st>>>(total, c, parts, (const double*)part, dG);
    }
    return gspn_launch_status();
}
