// threenn_nested.hip -- three_nn of one dense query set against SEVERAL known sets that are subsets of one cloud (ABI 10).
//
// In the full-feature mode of shape_proposal_net (model_rpointnet.py:184-188) every point of the dense cloud needs its three nearest
// neighbours in l4, l3, l2 and l1 of the SA stack.  Those sets are nested subsets of l1 (l2 = l1[fps2], l3 = l2[fps3], l4 = l3[fps4]), so
// one scan of l1 answers every level: the caller passes l1 once plus `local` (L, b, m) -- the index of l1 point k inside level l, or -1 --
// and every lane keeps one top-3 list per level in registers.
//
// Contract: for each level l the output equals gspn_threenn(xyz1, l1[level l]) bit for bit -- the squared distance by the reference's own
// expression (tf_interpolate.cpp:71-74, dist2_host) and the three smallest (distance, level-local index) pairs in that order, which is what
// the reference's strict-'<' cascade over ascending k leaves (ties to the lower index; fewer than three points leave (inf, 0)).  The scan
// visits l1 in its own order, which is NOT ascending in a level's local index, so the lists compare (d, index) pairs (top3_insert, as nn_insert of interpolate.hip) instead of
// relying on the visiting order.
//
// Thread per query, l1 staged through LDS in tiles of float4 {x, y, z, |p|^2} with a per-point level mask and the level-local indices.
// Cheap rejection as in three_nn_kernel (interpolate.hip): |p|^2 - 2 p.q <= b3 - |q|^2 + margin never rejects a candidate that could
// enter (margin covers the rounding of both evaluations; '<=' because a tie with a lower local index may still enter).  The threshold of a
// batch of NN_B candidates is the largest of the levels any of them belongs to; the union mask of the batch is uniform over the workgroup.
#include <math.h>
#include <stdint.h>

#include "common.h"

#define NNN_T 256                 // threads (= queries) per workgroup
#define NNN_TILE 512              // l1 points per LDS tile
#define NNN_B 8                   // candidates per rejection test
#define NNN_MAX_L 8

namespace {
struct Top3 { float b1, b2, b3; int i1, i2, i3; };
__device__ __forceinline__ void top3_insert(Top3& s, float d, int k) {
    if (d < s.b3 || (d == s.b3 && k < s.i3)) {
        if (d < s.b1 || (d == s.b1 && k < s.i1)) { s.b3 = s.b2; s.i3 = s.i2; s.b2 = s.b1; s.i2 = s.i1; s.b1 = d; s.i1 = k; }
        else if (d < s.b2 || (d == s.b2 && k < s.i2)) { s.b3 = s.b2; s.i3 = s.i2; s.b2 = d; s.i2 = k; }
        else { s.b3 = d; s.i3 = k; }
    }
}
}  // namespace

template <int LM>                 // levels held in registers (L <= LM; the bits of levels >= L are never set)
__global__ __launch_bounds__(NNN_T) void three_nn_nested_kernel(int b, int n, int m, int L, const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                                const int* __restrict__ local, const int* __restrict__ order, float* __restrict__ dist,
                                                                int* __restrict__ idx) {
    __shared__ float4 tile[NNN_TILE + NNN_B];
    __shared__ int tmask[NNN_TILE + NNN_B];
    __shared__ int tbatch[NNN_TILE / NNN_B];              // union of the level masks of each batch
    __shared__ int tloc[LM][NNN_TILE];
    __shared__ float tile_pm[NNN_T / 64];
    const int scene = blockIdx.x % b;                     // scene <-> XCD affinity for the known cloud
    const int t = threadIdx.x;
    int j = (blockIdx.x / b) * NNN_T + t;
    const bool live = j < n;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) {
        if (order) j = order[(size_t)scene * n + j];      // spatially coherent lanes: their rejections coincide
        const float* q = xyz1 + ((size_t)scene * n + j) * 3;
        qx = q[0]; qy = q[1]; qz = q[2];
    }
    const float qx2 = -2.f * qx, qy2 = -2.f * qy, qz2 = -2.f * qz;
    const float qq = __builtin_fmaf(qx, qx, __builtin_fmaf(qy, qy, qz * qz));
    const float qn = sqrtf(qq);
    Top3 s[LM];
    float thr[LM];
#pragma unroll
    for (int l = 0; l < LM; ++l) { s[l] = Top3{INFINITY, INFINITY, INFINITY, 0, 0, 0}; thr[l] = INFINITY; }
    const float* sp = xyz2 + (size_t)scene * m * 3;
    for (int k0 = 0; k0 < m; k0 += NNN_TILE) {
        const int cnt = min(NNN_TILE, m - k0);
        const int nb = (cnt + NNN_B - 1) / NNN_B;
        __syncthreads();
        float pm = 0.f;
        for (int u = t; u < nb * NNN_B; u += NNN_T) {
            if (u < cnt) {
                const size_t k = (size_t)(k0 + u);
                const float px = sp[k * 3 + 0], py = sp[k * 3 + 1], pz = sp[k * 3 + 2];
                const float pw = __builtin_fmaf(px, px, __builtin_fmaf(py, py, pz * pz));
                int mask = 0;
                for (int l = 0; l < L; ++l) {
                    const int loc = local[((size_t)l * b + scene) * m + k];
                    tloc[l][u] = loc;
                    mask |= (loc >= 0) << l;
                }
                tile[u] = make_float4(px, py, pz, mask ? pw : INFINITY);    // a point of no level never passes
                tmask[u] = mask;
                if (mask) pm = fmaxf(pm, pw);
            } else {
                tile[u] = make_float4(0.f, 0.f, 0.f, INFINITY);            // pad to a whole batch
                tmask[u] = 0;
            }
        }
        for (int s_ = 32; s_ >= 1; s_ >>= 1) pm = fmaxf(pm, __shfl_xor(pm, s_, 64));
        if ((t & 63) == 0) tile_pm[t >> 6] = pm;
        __syncthreads();
        for (int v = t; v < nb; v += NNN_T) {
            int u = 0;
#pragma unroll
            for (int w = 0; w < NNN_B; ++w) u |= tmask[v * NNN_B + w];
            tbatch[v] = u;
        }
        pm = fmaxf(fmaxf(tile_pm[0], tile_pm[1]), fmaxf(tile_pm[2], tile_pm[3]));
        const float r = sqrtf(pm) + qn;
        const float margin = __builtin_fmaf(4e-6f * r, r, NN_MARGIN_FLOOR);      // >> 8 ulp of (|p| + |q|)^2, 2^-149 each where that is subnormal (as three_nn_kernel)
#pragma unroll
        for (int l = 0; l < LM; ++l) thr[l] = (s[l].b3 - qq) + margin;
        __syncthreads();
        for (int v = 0; v < nb; ++v) {
            const int bm = __builtin_amdgcn_readfirstlane(tbatch[v]);      // uniform over the workgroup
            if (!bm) continue;
            float tb = -INFINITY;
#pragma unroll
            for (int l = 0; l < LM; ++l)
                if (bm & (1 << l)) tb = fmaxf(tb, thr[l]);
            const int kb = v * NNN_B;
            float4 p[NNN_B];
            float sd[NNN_B];
#pragma unroll
            for (int w = 0; w < NNN_B; ++w) {
                p[w] = tile[kb + w];
                sd[w] = __builtin_fmaf(p[w].x, qx2, __builtin_fmaf(p[w].y, qy2, __builtin_fmaf(p[w].z, qz2, p[w].w)));
            }
            float smin = sd[0];
#pragma unroll
            for (int w = 1; w < NNN_B; ++w) smin = fminf(smin, sd[w]);
            if (!(smin <= tb)) continue;
#pragma unroll
            for (int w = 0; w < NNN_B; ++w) {
                if (!(sd[w] <= tb)) continue;
                const int mk = tmask[kb + w];
                const float d = dist2_host(p[w].x - qx, p[w].y - qy, p[w].z - qz);      // tf_interpolate.cpp:74, the reference's expression
#pragma unroll
                for (int l = 0; l < LM; ++l) {
                    if ((mk & (1 << l)) && (d < s[l].b3 || (d == s[l].b3 && tloc[l][kb + w] < s[l].i3))) {
                        top3_insert(s[l], d, tloc[l][kb + w]);
                        thr[l] = (s[l].b3 - qq) + margin;
                    }
                }
            }
        }
    }
    if (live) {
        for (int l = 0; l < L; ++l) {
            Top3 o = s[0];
#pragma unroll
            for (int u = 1; u < LM; ++u)
                if (u == l) o = s[u];                     // (register arrays: select, no scratch)
            const size_t row = (((size_t)l * b + scene) * n + j) * 3;
            dist[row + 0] = o.b1; dist[row + 1] = o.b2; dist[row + 2] = o.b3;
            idx[row + 0] = o.i1; idx[row + 1] = o.i2; idx[row + 2] = o.i3;
        }
    }
}

extern "C" int gspn_threenn_nested(int b, int n, int m, int L, const float* xyz1, const float* xyz2, const int* local, const int* order, float* dist,
                                   int* idx, void* stream) {
    if (b < 0 || n < 0 || m < 0 || L < 1) return GSPN_ERR_ARG;
    if (L > NNN_MAX_L) return GSPN_ERR_UNSUPPORTED;
    if (b == 0 || n == 0) return 0;
    if (!xyz1 || !dist || !idx || (m > 0 && (!xyz2 || !local))) return GSPN_ERR_ARG;
    // every index below is formed in size_t; what must fit an int is the grid and the per-scene row counts the kernel keeps in ints
    const long long blocks = (long long)b * ((n + NNN_T - 1) / NNN_T);
    if (blocks > 0x7FFFFFFFll || (long long)n * 3 > 0x7FFFFFFFll || (long long)m * 3 > 0x7FFFFFFFll) return GSPN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(NNN_T);
    if (L <= 1) hipLaunchKernelGGL(three_nn_nested_kernel<1>, grid, block, 0, st, b, n, m, L, xyz1, xyz2, local, order, dist, idx);
    else if (L <= 2) hipLaunchKernelGGL(three_nn_nested_kernel<2>, grid, block, 0, st, b, n, m, L, xyz1, xyz2, local, order, dist, idx);
    else if (L <= 4) hipLaunchKernelGGL(three_nn_nested_kernel<4>, grid, block, 0, st, b, n, m, L, xyz1, xyz2, local, order, dist, idx);
    else hipLaunchKernelGGL(three_nn_nested_kernel<8>, grid, block, 0, st, b, n, m, L, xyz1, xyz2, local, order, dist, idx);
    return gspn_launch_status();
}
