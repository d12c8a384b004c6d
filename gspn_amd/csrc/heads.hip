// heads.hip -- the first layer of R-PointNet's two heads (models/model_rpointnet.py:915, :946) over the crop that points_cropping (:785-816)
// would have written, ABI 15.
//
// The heads' input row is concat(pc_fea[idx] (C), (pc_center[idx] - roi centre) / roi size (3), (pc[idx] - roi centre) / roi size (3)), and
// their first layer is linear and per point, so it commutes with the gather:
//     y[row, :] = T[scene, idx[row], :] + side[row, 0:6] . Wside (6, cout) + bias,      T = pc_fea . W[:C]   (one gspn_mlp_fwd launch)
// The (rows, C + 6) crop never exists; a gathered row is cout floats wide instead of C + 6.
//
//   gspn_crop_linear_fwd       a workgroup takes a tile of CL_TILE rows.  One thread per row first computes the six side values (the index row
//                              is read coalesced) into LDS; then CL lanes share a row, one float4 of the T row each, with their seven
//                              float4 of Wside / bias in registers: at cout 64 a wave covers 4 rows per step.
//   gspn_crop_linear_bwd_side  dWside = side^T . dY, dbias = colsum(dY) and the per-row gradient of the centre coordinates,
//                              (dY[row] . Wside[0:3]^T) / size.  Same tiles and lanes; every thread keeps seven float4 sums over its rows, the
//                              workgroup adds them over its row groups through LDS in a fixed order and writes ONE partial (7, cout); a
//                              second kernel adds the partials in workgroup order in double.  No atomics: the bits repeat.
//
// The gradients of the two gathers (dT from dY, dcenter from the per-row gradient) are sums over the rows that name a point:
// gspn_crop_gather_grad of roi.hip, through the inverse lists of idx.  No batch-norm statistics here: the layer's batch norm is the
// stand-alone one (batchnorm.hip), which sums about a pivot.
//
// fp32, -ffp-contract=off: the side values are the subtraction and the division points_cropping does.  An index outside [0, n) is clamped.
#include "common.h"

#define CL_THREADS 256
#define CL_TILE 128
#define CL_MAX_COUT 256                 // one float4 per lane, at most a wave per row
#define CL_MAX_PARTS 512
#define CL_SIDE_LD 12                   // per row in LDS: 6 side values, the 3 sizes, the source row of T (as int bits), 2 unused

namespace {

// 1 / 2 / ... / 64 lanes per row: the smallest power of two that covers cout / 4 float4 columns
inline int cl_lanes(int cout) {
    int l = 1;
    while (l * 4 < cout) l <<= 1;
    return l;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 fma4(float s, float4 w, float4 a) {           // a + s * w, a multiply and an add per element
    return make_float4(a.x + s * w.x, a.y + s * w.y, a.z + s * w.z, a.w + s * w.w);
}
__device__ __forceinline__ float dot4(float4 a, float4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }

// the side values of the tile's rows, one thread per row: side[i] = {center_n xyz, coord_n xyz, size xyz, source row of T}
__device__ __forceinline__ void cl_stage_side(float (*side)[CL_SIDE_LD], long row0, int tile_rows, int n, int p, long rows_per_scene,
                                              const int* __restrict__ idx, const float* __restrict__ pc, const float* __restrict__ center,
                                              const float* __restrict__ rois, int normalize) {
    const int i = threadIdx.x;
    if (i < tile_rows) {
        const long row = row0 + i;
        const long scene = row / rows_per_scene;
        const float* roi = rois + (row / p) * 6;
        const int src = min(max(idx[row], 0), n - 1);
        const long point = scene * n + src;
        const float cx = roi[0], cy = roi[1], cz = roi[2];
        float sx = 1.f, sy = 1.f, sz = 1.f;
        if (normalize) {
            const float pad = (((((cx + cy) + cz) + roi[3]) + roi[4]) + roi[5]) == 0.f ? 1.f : 0.f;       // :812
            sx = roi[3] + pad, sy = roi[4] + pad, sz = roi[5] + pad;
        }
        float* s = side[i];
        const float* c = center + point * 3;
        const float* q = pc + point * 3;
        s[0] = c[0] - cx, s[1] = c[1] - cy, s[2] = c[2] - cz;
        s[3] = q[0] - cx, s[4] = q[1] - cy, s[5] = q[2] - cz;
        if (normalize) {
            s[0] /= sx, s[1] /= sy, s[2] /= sz;
            s[3] /= sx, s[4] /= sy, s[5] /= sz;
        }
        s[6] = sx, s[7] = sy, s[8] = sz;
        s[9] = __int_as_float(src);
    }
}

template <int LANES>
__global__ __launch_bounds__(CL_THREADS) void crop_linear_fwd_kernel(long rows, int n, int p, long rows_per_scene, int cout,
                                                                     const float* __restrict__ T, int ldt, const int* __restrict__ idx,
                                                                     const float* __restrict__ pc, const float* __restrict__ center,
                                                                     const float* __restrict__ rois, int normalize,
                                                                     const float* __restrict__ Wside, const float* __restrict__ bias,
                                                                     float* __restrict__ Y) {
    constexpr int GROUPS = CL_THREADS / LANES;                                    // rows in flight per step
    __shared__ float side[CL_TILE][CL_SIDE_LD];
    const long row0 = (long)blockIdx.x * CL_TILE;
    const int tile_rows = rows - row0 < CL_TILE ? (int)(rows - row0) : CL_TILE;
    cl_stage_side(side, row0, tile_rows, n, p, rows_per_scene, idx, pc, center, rois, normalize);
    const int col = (threadIdx.x % LANES) * 4, g = threadIdx.x / LANES;
    const bool live = col < cout;
    float4 w[6], bv = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = live ? ld4(Wside + (size_t)k * cout + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) bv = ld4(bias + col);
    __syncthreads();
    if (!live) return;
    for (int i = g; i < tile_rows; i += GROUPS) {
        const float* s = side[i];
        const long row = row0 + i;
        const long trow = (row / rows_per_scene) * n + __float_as_int(s[9]);
        float4 y = ld4(T + trow * ldt + col);
#pragma unroll
        for (int k = 0; k < 6; ++k) y = fma4(s[k], w[k], y);
        y = make_float4(y.x + bv.x, y.y + bv.y, y.z + bv.z, y.w + bv.w);
        st4(Y + row * cout + col, y);
    }
}

template <int LANES>
__global__ __launch_bounds__(CL_THREADS) void crop_linear_bwd_side_kernel(long rows, int n, int p, long rows_per_scene, int cout,
                                                                          const float* __restrict__ dY, const int* __restrict__ idx,
                                                                          const float* __restrict__ pc, const float* __restrict__ center,
                                                                          const float* __restrict__ rois, int normalize,
                                                                          const float* __restrict__ Wside, float* __restrict__ part,
                                                                          float* __restrict__ dcenter_rows) {
    constexpr int GROUPS = CL_THREADS / LANES;
    constexpr int STEPS = (CL_TILE + GROUPS - 1) / GROUPS;                        // the same trip count for every lane: the shuffles below need it
    __shared__ float side[CL_TILE][CL_SIDE_LD];
    __shared__ float red[7 * CL_THREADS * 4];                                     // [7][GROUPS][LANES * 4]
    const int col = (threadIdx.x % LANES) * 4, g = threadIdx.x / LANES;
    const bool live = col < cout;
    float4 w[3], acc[7];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = live ? ld4(Wside + (size_t)k * cout + col) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    const long tiles = (rows + CL_TILE - 1) / CL_TILE;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {                        // a fixed set of tiles per workgroup, in ascending order
        const long row0 = t * CL_TILE;
        const int tile_rows = rows - row0 < CL_TILE ? (int)(rows - row0) : CL_TILE;
        __syncthreads();                                                          // the previous tile's side values have been read
        cl_stage_side(side, row0, tile_rows, n, p, rows_per_scene, idx, pc, center, rois, normalize);
        __syncthreads();
        for (int j = 0; j < STEPS; ++j) {
            const int i = g + j * GROUPS;
            const bool valid = i < tile_rows;
            const int ii = valid ? i : 0;
            const float* s = side[ii];
            const long row = row0 + ii;
            const float4 d = (valid && live) ? ld4(dY + row * cout + col) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[k] = fma4(s[k], d, acc[k]);
            acc[6] = make_float4(acc[6].x + d.x, acc[6].y + d.y, acc[6].z + d.z, acc[6].w + d.w);
            float gx = dot4(d, w[0]), gy = dot4(d, w[1]), gz = dot4(d, w[2]);
#pragma unroll
            for (int m = 1; m < LANES; m <<= 1) {                                 // over the lanes of the row, the same tree on every call
                gx += __shfl_xor(gx, m);
                gy += __shfl_xor(gy, m);
                gz += __shfl_xor(gz, m);
            }
            if (valid && col == 0) st4(dcenter_rows + row * 4, make_float4(gx / s[6], gy / s[7], gz / s[8], 0.f));
        }
    }
    // over the row groups of the workgroup, in group order
#pragma unroll
    for (int k = 0; k < 7; ++k) st4(red + ((size_t)k * GROUPS + g) * (LANES * 4) + col, acc[k]);
    __syncthreads();
    for (int e = threadIdx.x; e < 7 * cout; e += CL_THREADS) {
        const int k = e / cout, c = e % cout;
        float sum = 0.f;
        for (int u = 0; u < GROUPS; ++u) sum += red[((size_t)k * GROUPS + u) * (LANES * 4) + c];
        part[(size_t)blockIdx.x * 7 * cout + e] = sum;
    }
}

// part (nparts, 7, cout) -> dWside (6, cout), dbias (cout): the partials of the workgroups added in workgroup order, in double
__global__ __launch_bounds__(CL_THREADS) void crop_linear_bwd_join_kernel(int nparts, int cout, const float* __restrict__ part,
                                                                          float* __restrict__ dWside, float* __restrict__ dbias) {
    const int e = blockIdx.x * CL_THREADS + threadIdx.x;
    if (e >= 7 * cout) return;
    double sum = 0.0;
    for (int u = 0; u < nparts; ++u) sum += (double)part[(size_t)u * 7 * cout + e];
    if (e < 6 * cout) dWside[e] = (float)sum;
    else dbias[e - 6 * cout] = (float)sum;
}

inline bool cl_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) % 16) == 0;
}

// sizes every entry point checks the same way: 0 when they are fine
inline int cl_check_sizes(int b, int n, int r, int p, int cout) {
    if (b <= 0 || n <= 0 || r <= 0 || p <= 0 || cout <= 0) return GSPN_ERR_ARG;
    if (cout % 4 || cout > CL_MAX_COUT || (long)b * r * p >= (1L << 31) || (long)b * n >= (1L << 31)) return GSPN_ERR_UNSUPPORTED;
    return 0;
}

inline int cl_parts(long rows) {
    const long tiles = (rows + CL_TILE - 1) / CL_TILE;
    return tiles < CL_MAX_PARTS ? (int)tiles : CL_MAX_PARTS;
}

}  // namespace

#define CL_DISPATCH(lanes, CALL)                 \
    switch (lanes) {                             \
        case 1: CALL(1); break;                  \
        case 2: CALL(2); break;                  \
        case 4: CALL(4); break;                  \
        case 8: CALL(8); break;                  \
        case 16: CALL(16); break;                \
        case 32: CALL(32); break;                \
        default: CALL(64); break;                \
    }

extern "C" int gspn_crop_linear_fwd(int b, int n, int r, int p, int cout, const float* T, int ldt, const int* idx, const float* pc,
                                    const float* center, const float* rois, int normalize, const float* Wside, const float* bias, float* Y,
                                    void* stream) {
    const int bad = cl_check_sizes(b, n, r, p, cout);
    if (bad) return bad;
    if (ldt < cout || !T || !idx || !pc || !center || !rois || !Wside || !bias || !Y) return GSPN_ERR_ARG;
    if (ldt % 4 || !cl_aligned16(T, Wside, bias, Y)) return GSPN_ERR_UNSUPPORTED;
    const long rows = (long)b * r * p;
    const unsigned grid = (unsigned)((rows + CL_TILE - 1) / CL_TILE);
    hipStream_t st = (hipStream_t)stream;
#define CL_FWD(L_) \
    crop_linear_fwd_kernel<L_><<<grid, CL_THREADS, 0, st>>>(rows, n, p, (long)r * p, cout, T, ldt, idx, pc, center, rois, normalize, Wside, bias, Y)
    CL_DISPATCH(cl_lanes(cout), CL_FWD)
#undef CL_FWD
    return gspn_launch_status();
}

extern "C" long gspn_crop_linear_part_floats(int b, int r, int p, int cout) {
    if (cl_check_sizes(b, 1, r, p, cout)) return 0;
    return (long)cl_parts((long)b * r * p) * 7 * cout;
}

extern "C" int gspn_crop_linear_bwd_side(int b, int n, int r, int p, int cout, const float* dY, const int* idx, const float* pc,
                                         const float* center, const float* rois, int normalize, const float* Wside, float* part, float* dWside,
                                         float* dbias, float* dcenter_rows, void* stream) {
    const int bad = cl_check_sizes(b, n, r, p, cout);
    if (bad) return bad;
    if (!dY || !idx || !pc || !center || !rois || !Wside || !part || !dWside || !dbias || !dcenter_rows) return GSPN_ERR_ARG;
    if (!cl_aligned16(dY, Wside, dcenter_rows)) return GSPN_ERR_UNSUPPORTED;
    const long rows = (long)b * r * p;
    const int nparts = cl_parts(rows);
    hipStream_t st = (hipStream_t)stream;
#define CL_BWD(L_)                                                                                                                          \
    crop_linear_bwd_side_kernel<L_><<<nparts, CL_THREADS, 0, st>>>(rows, n, p, (long)r * p, cout, dY, idx, pc, center, rois, normalize, Wside, \
                                                                   part, dcenter_rows)
    CL_DISPATCH(cl_lanes(cout), CL_BWD)
#undef CL_BWD
    crop_linear_bwd_join_kernel<<<(7 * cout + CL_THREADS - 1) / CL_THREADS, CL_THREADS, 0, st>>>(nparts, cout, part, dWside, dbias);
    return gspn_launch_status();
}
