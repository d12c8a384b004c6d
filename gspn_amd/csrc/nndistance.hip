// nndistance.hip -- tf_ops/nn_distance on gfx950: bidirectional nearest neighbour (Chamfer)
// distance and its gradient.  Reference: tf_ops/nn_distance/tf_nndistance_g.cu:5-157.
#include <stdlib.h>
#include "common.h"

// ============================================================================================
// NmDistance (tf_nndistance_g.cu:5-127): for each point of set A the squared distance to, and
// index of, its nearest point of set B; lowest index wins ties (strict '<' inside a 512-tile in
// ascending k, strict '>' across tiles :119).  Arithmetic: (p2-p1) per axis, FMA-contracted sum.
// The reference fixes the grid at 32x16 blocks and loops over the batch; in GSPN the batch is
// b = B*256 small clouds (512 x 512), so here the grid is one block per (cloud, 256-point slab)
// and the other cloud is staged through LDS as float4 (one broadcast ds_read_b128 per candidate).
// ============================================================================================
#define NM_TILE 1024
#define NM_BLOCK 256

// NM_Q queries per lane (r04): one broadcast LDS read feeds NM_Q independent distance chains -- half the LDS instructions per pair at NM_Q = 2
// and twice the independent work between dependent compare / select pairs (round 3's SQ counters: 0.36 of the vector issue rate, half the
// wave cycles stalled on issue).  Queries j, j + NM_BLOCK of a slab of NM_Q * NM_BLOCK points.
// Only when the grid still fills the chip at NM_Q = 2 (the model's 2048 clouds: 267 -> 212 us); a launch with few workgroups keeps one
// query per lane (the harness shape's 1024-query direction: 64 workgroups at NM_Q = 2 ran twice as long).
template <int NM_Q>
__global__ __launch_bounds__(NM_BLOCK) void nm_distance_kernel(int b, int n, const float* __restrict__ xyz, int m, const float* __restrict__ xyz2,
                                                               float* __restrict__ result, int* __restrict__ result_i) {
    __shared__ float4 tile[NM_TILE];
    const int cloud = blockIdx.x % b;
    const int j0 = (blockIdx.x / b) * (NM_BLOCK * NM_Q) + threadIdx.x;
    float x1[NM_Q], y1[NM_Q], z1[NM_Q], best[NM_Q];
    int best_i[NM_Q];
#pragma unroll
    for (int u = 0; u < NM_Q; ++u) {
        const int j = j0 + u * NM_BLOCK;
        x1[u] = y1[u] = z1[u] = 0.f;
        if (j < n) {
            const float* q = xyz + ((size_t)cloud * n + j) * 3;
            x1[u] = q[0]; y1[u] = q[1]; z1[u] = q[2];
        }
        best[u] = 0.f;
        best_i[u] = 0;
    }
    const float* sp = xyz2 + (size_t)cloud * m * 3;
    for (int k0 = 0; k0 < m; k0 += NM_TILE) {
        const int cnt = min(NM_TILE, m - k0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += NM_BLOCK)
            tile[t] = make_float4(sp[(size_t)(k0 + t) * 3 + 0], sp[(size_t)(k0 + t) * 3 + 1], sp[(size_t)(k0 + t) * 3 + 2], 0.f);
        __syncthreads();
        int k = 0;
        if (k0 == 0) {                                            // candidate 0 initialises (:29): peeled, the loop body is then branch-free
            const float4 p = tile[0];
#pragma unroll
            for (int u = 0; u < NM_Q; ++u) { best[u] = dist2_cuda(p.x - x1[u], p.y - y1[u], p.z - z1[u]); best_i[u] = 0; }
            k = 1;
        }
#pragma unroll 8
        for (; k < cnt; ++k) {
            const float4 p = tile[k];
#pragma unroll
            for (int u = 0; u < NM_Q; ++u) {
                const float d = dist2_cuda(p.x - x1[u], p.y - y1[u], p.z - z1[u]);       // :25-28
                if (d < best[u]) { best[u] = d; best_i[u] = k0 + k; }                      // :29, :119: strict '<', the lowest index wins ties
            }
        }
    }
#pragma unroll
    for (int u = 0; u < NM_Q; ++u) {
        const int j = j0 + u * NM_BLOCK;
        if (j < n) {
            result[(size_t)cloud * n + j] = best[u];
            result_i[(size_t)cloud * n + j] = best_i[u];
        }
    }
}
extern "C" int gspn_nmdistance(int b, int n, const float* xyz, int m, const float* xyz2, float* result, int* result_i,
                               float* result2, int* result2_i, void* stream) {
    if (b < 0 || n < 0 || m < 0) return GSPN_ERR_ARG;
    if (b == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    auto go = [&](int nq, const float* q, int nc, const float* c, float* r, int* ri) -> int {
        if (nq <= 0) return 0;
        const long long g2 = (long long)b * ((nq + 2 * NM_BLOCK - 1) / (2 * NM_BLOCK)), g1 = (long long)b * ((nq + NM_BLOCK - 1) / NM_BLOCK);
        if (g1 > 0x7FFFFFFFll) return GSPN_ERR_UNSUPPORTED;
        if (g2 >= 1024) hipLaunchKernelGGL(nm_distance_kernel<2>, dim3((unsigned)g2), dim3(NM_BLOCK), 0, st, b, nq, q, nc, c, r, ri);
        else hipLaunchKernelGGL(nm_distance_kernel<1>, dim3((unsigned)g1), dim3(NM_BLOCK), 0, st, b, nq, q, nc, c, r, ri);
        return 0;
    };
    if (go(n, xyz, m, xyz2, result, result_i) || go(m, xyz2, n, xyz, result2, result2_i)) return GSPN_ERR_UNSUPPORTED;
    return gspn_launch_status();
}

// ============================================================================================
// NmDistanceGrad (tf_nndistance_g.cu:132-157): g = 2*grad_dist[j];  grad1[j] += g*(p1-p2),
// grad2[idx[j]] -= g*(p1-p2), then the symmetric pass.  The reference launches 16 blocks and
// loops the batch serially; here one thread per point over the whole batch.  The write to the
// point's own gradient row races with scatter contributions of the other pass, so both are
// atomics (as in the reference).
// ============================================================================================
__global__ void nm_distance_grad_kernel(long total, int n, const float* __restrict__ xyz1, int m, const float* __restrict__ xyz2,
                                        const float* __restrict__ grad_dist1, const int* __restrict__ idx1,
                                        float* __restrict__ grad_xyz1, float* __restrict__ grad_xyz2) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long cloud = i / n;
        const float* p1 = xyz1 + i * 3;
        const int j2 = idx1[i];
        const float* p2 = xyz2 + ((size_t)cloud * m + j2) * 3;
        const float g = grad_dist1[i] * 2;
        float* g1 = grad_xyz1 + i * 3;
        float* g2 = grad_xyz2 + ((size_t)cloud * m + j2) * 3;
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const float v = g * (p1[l] - p2[l]);
            atomicAdd(g1 + l, v);
            atomicAdd(g2 + l, -v);
        }
    }
}
// Small clouds (the model's use: b = B * NUM_SAMPLE clouds of 512 x 512 points, model_rpointnet.py:1346-1355): one workgroup per cloud, both
// gradient tensors of the cloud in LDS.  A point's own term is a plain store, the scatter terms are LDS atomics (the reference's global
// atomicAdd, tf_nndistance_g.cu:145-150, is order-free as well); the two outputs leave in one coalesced sweep.  No memset, no global
// atomics: 2048 x (512, 512) in 26 us against 310 us for the two atomic launches.
#define NMG_MAX_PTS 4096            // (n + m) * 12 bytes of LDS
__global__ __launch_bounds__(256) void nm_distance_grad_lds_kernel(int n, const float* __restrict__ xyz1, int m, const float* __restrict__ xyz2,
                                                                   const float* __restrict__ grad_dist1, const int* __restrict__ idx1,
                                                                   const float* __restrict__ grad_dist2, const int* __restrict__ idx2,
                                                                   float* __restrict__ grad_xyz1, float* __restrict__ grad_xyz2) {
    extern __shared__ float sg[];                    // [n*3] gradient of cloud 1, [m*3] of cloud 2
    float* g1 = sg;
    float* g2 = sg + (size_t)n * 3;
    const size_t c = blockIdx.x;
    const float* a = xyz1 + c * n * 3;
    const float* bq = xyz2 + c * m * 3;
    // own terms: grad1[i] = g (p1 - p2[idx1[i]]) (:143-147), grad2[j] = g' (p2 - p1[idx2[j]]) (the symmetric launch :156)
    for (int i = threadIdx.x; i < n; i += 256) {
        const int j = idx1[c * n + i];
        const float g = grad_dist1[c * n + i] * 2;
#pragma unroll
        for (int l = 0; l < 3; ++l) g1[i * 3 + l] = g * (a[i * 3 + l] - bq[j * 3 + l]);
    }
    for (int j = threadIdx.x; j < m; j += 256) {
        const int i = idx2[c * m + j];
        const float g = grad_dist2[c * m + j] * 2;
#pragma unroll
        for (int l = 0; l < 3; ++l) g2[j * 3 + l] = g * (bq[j * 3 + l] - a[i * 3 + l]);
    }
    __syncthreads();
    // scatter terms: grad2[idx1[i]] -= g (p1 - p2[idx1[i]]), grad1[idx2[j]] -= g' (p2 - p1[idx2[j]])
    for (int i = threadIdx.x; i < n; i += 256) {
        const int j = idx1[c * n + i];
        const float g = grad_dist1[c * n + i] * 2;
#pragma unroll
        for (int l = 0; l < 3; ++l) atomicAdd(g2 + j * 3 + l, -(g * (a[i * 3 + l] - bq[j * 3 + l])));
    }
    for (int j = threadIdx.x; j < m; j += 256) {
        const int i = idx2[c * m + j];
        const float g = grad_dist2[c * m + j] * 2;
#pragma unroll
        for (int l = 0; l < 3; ++l) atomicAdd(g1 + i * 3 + l, -(g * (bq[j * 3 + l] - a[i * 3 + l])));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n * 3; i += 256) grad_xyz1[c * n * 3 + i] = g1[i];
    for (int i = threadIdx.x; i < m * 3; i += 256) grad_xyz2[c * m * 3 + i] = g2[i];
}
extern "C" int gspn_nmdistance_grad(int b, int n, const float* xyz1, int m, const float* xyz2, const float* grad_dist1, const int* idx1,
                                    const float* grad_dist2, const int* idx2, float* grad_xyz1, float* grad_xyz2, void* stream) {
    if (b < 0 || n < 0 || m < 0) return GSPN_ERR_ARG;
    if (b == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (n > 0 && m > 0 && n + m <= NMG_MAX_PTS) {
        hipLaunchKernelGGL(nm_distance_grad_lds_kernel, dim3((unsigned)b), dim3(256), sizeof(float) * 3 * (size_t)(n + m), st, n, xyz1, m, xyz2, grad_dist1, idx1,
                           grad_dist2, idx2, grad_xyz1, grad_xyz2);
        return gspn_launch_status();
    }
    if (n > 0 && (e = hipMemsetAsync(grad_xyz1, 0, sizeof(float) * (size_t)b * n * 3, st)) != hipSuccess) return (int)e;   // :153
    if (m > 0 && (e = hipMemsetAsync(grad_xyz2, 0, sizeof(float) * (size_t)b * m * 3, st)) != hipSuccess) return (int)e;   // :154
    if (n == 0 || m == 0) return 0;
    const long t1 = (long)b * n, t2 = (long)b * m;
    hipLaunchKernelGGL(nm_distance_grad_kernel, dim3(grid_for(t1, 256)), dim3(256), 0, st, t1, n, xyz1, m, xyz2, grad_dist1, idx1, grad_xyz1, grad_xyz2);
    hipLaunchKernelGGL(nm_distance_grad_kernel, dim3(grid_for(t2, 256)), dim3(256), 0, st, t2, m, xyz2, n, xyz1, grad_dist2, idx2, grad_xyz2, grad_xyz1);
    return gspn_launch_status();
}

// The same gradient as a GATHER, for clouds beyond the LDS kernel: the caller supplies the inverse lists of idx1 over cloud 2's points
// (order1 (b, n): positions of idx1 sorted by value, ties ascending; offsets1 (b, m + 1)) and of idx2 over cloud 1's points (order2 (b, m),
// offsets2 (b, n + 1)) -- gspn_inverse_lists.  One thread per point adds its terms in exactly the order of the reference's SEQUENTIAL CPU
// twin (tf_nndistance.cpp:126-163: first the loop over cloud 1 -- own term of grad1, scatter into grad2 --, then the loop over cloud 2):
//   grad1[i] = own1(i), then  -= t2(j) for the j with idx2[j] == i, ascending j;     grad2[j] = -t1(i) for the i with idx1[i] == j, ascending i, then += own2(j)
// Bit-identical to the oracle's restatement of that loop; no memset, no atomics (the CUDA kernel's atomicAdd, tf_nndistance_g.cu:145-150, has no order).
__global__ void nm_distance_grad_csr_kernel(long total1, long total, int n, const float* __restrict__ xyz1, int m, const float* __restrict__ xyz2,
                                            const float* __restrict__ gd1, const int* __restrict__ idx1, const float* __restrict__ gd2,
                                            const int* __restrict__ idx2, const int* __restrict__ order1, const int* __restrict__ offsets1,
                                            const int* __restrict__ order2, const int* __restrict__ offsets2, float* __restrict__ grad1,
                                            float* __restrict__ grad2) {
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        if (t < total1) {                            // a point of cloud 1
            const long c = t / n;
            const int i = (int)(t - c * n);
            const float* p1 = xyz1 + t * 3;
            const float* q = xyz2 + ((size_t)c * m + idx1[t]) * 3;
            const float g = gd1[t] * 2;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            a0 += g * (p1[0] - q[0]); a1 += g * (p1[1] - q[1]); a2 += g * (p1[2] - q[2]);
            const int* off = offsets2 + c * (n + 1);
            for (int e = off[i]; e < off[i + 1]; ++e) {
                const int j = order2[c * m + e];
                const float* p2 = xyz2 + ((size_t)c * m + j) * 3;
                const float h = gd2[c * m + j] * 2;
                a0 -= h * (p2[0] - p1[0]); a1 -= h * (p2[1] - p1[1]); a2 -= h * (p2[2] - p1[2]);
            }
            grad1[t * 3 + 0] = a0; grad1[t * 3 + 1] = a1; grad1[t * 3 + 2] = a2;
        } else {                                     // a point of cloud 2
            const long u = t - total1;
            const long c = u / m;
            const int j = (int)(u - c * m);
            const float* p2 = xyz2 + u * 3;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            const int* off = offsets1 + c * (m + 1);
            for (int e = off[j]; e < off[j + 1]; ++e) {
                const int i = order1[c * n + e];
                const float* p1 = xyz1 + ((size_t)c * n + i) * 3;
                const float g = gd1[c * n + i] * 2;
                a0 -= g * (p1[0] - p2[0]); a1 -= g * (p1[1] - p2[1]); a2 -= g * (p1[2] - p2[2]);
            }
            const float* q = xyz1 + ((size_t)c * n + idx2[u]) * 3;
            const float h = gd2[u] * 2;
            a0 += h * (p2[0] - q[0]); a1 += h * (p2[1] - q[1]); a2 += h * (p2[2] - q[2]);
            grad2[u * 3 + 0] = a0; grad2[u * 3 + 1] = a1; grad2[u * 3 + 2] = a2;
        }
    }
}
extern "C" int gspn_nmdistance_grad_csr(int b, int n, const float* xyz1, int m, const float* xyz2, const float* grad_dist1, const int* idx1,
                                        const float* grad_dist2, const int* idx2, const int* order1, const int* offsets1, const int* order2,
                                        const int* offsets2, float* grad_xyz1, float* grad_xyz2, void* stream) {
    if (b < 0 || n <= 0 || m <= 0) return GSPN_ERR_ARG;
    if (b == 0) return 0;
    if (!xyz1 || !xyz2 || !grad_dist1 || !idx1 || !grad_dist2 || !idx2 || !order1 || !offsets1 || !order2 || !offsets2 || !grad_xyz1 || !grad_xyz2) return GSPN_ERR_ARG;
    const long t1 = (long)b * n, tot = t1 + (long)b * m;
    hipLaunchKernelGGL(nm_distance_grad_csr_kernel, dim3(grid_for(tot, 256)), dim3(256), 0, (hipStream_t)stream, t1, tot, n, xyz1, m, xyz2, grad_dist1, idx1,
                       grad_dist2, idx2, order1, offsets1, order2, offsets2, grad_xyz1, grad_xyz2);
    return gspn_launch_status();
}

