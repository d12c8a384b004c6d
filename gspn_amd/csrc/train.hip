// train.hip -- the compute of the reference's train.py that is not a network (ABI 20).
//
//   gspn_batch_assemble      get_batch (train.py:221-240) over dataset.py:143-190 for a whole batch from a scene cache that lives on the
//                            device: the point permutation, the padding of the instance sets, the rotation about z + translation and
//                            bbox_ins.  Three launches, nothing read back:
//                              batch_draw_kernel      one thread per batch slot draws R and t (float64) into the `rotation` / `translation`
//                                                     outputs.  BOTH kernels below read them from there, so the transform of pc and the
//                                                     transform of pc_ins are the same bits by construction, and so are the outputs.
//                              batch_points_kernel    one workgroup per tile of 256 output points: out[i] = in[perm(i)].  The read side is a
//                                                     random gather by construction; the four arrays of one point stay in one thread and the
//                                                     writes are coalesced.
//                              batch_instances_kernel one wave per (slot, group) row, as points_bbox_kernel: the row is read once, transformed,
//                                                     written and reduced to its box in the same pass.
//   gspn_adam_tf_flat        tf.train.AdamOptimizer's rule over one flat buffer (optim.hip's gspn_adam_flat is torch.optim.Adam's)
//   gspn_momentum_flat       tf.train.MomentumOptimizer's
//   gspn_scalars_accumulate  running sums of up to 16 device scalars, so that a step ends without a host read
//
// The translation unit is compiled with -ffp-contract=off like the box kernels: the float64 transform below is dataset._rigid's order of
// operations, nothing fused.
#include "box_common.h"
#include "rand32.h"

#define BA_THREADS 256
#define BA_WAVES (BA_THREADS / GSPN_WAVE)

namespace {

// ---------------------------------------------------------------------------------------------------- the permutation
// gspn_batch_perm of include/gspn_hip.h: a 4-round balanced Feistel network over `bits` (even) bits, cycle-walked into [0, n)
struct PermKey {
    unsigned k[4];
    int half;               // bits / 2, 1..16
};
__device__ __forceinline__ int perm_half_bits(long n) {
    int half = 1;
    while (half < 16 && (1ll << (2 * half)) < n) ++half;
    return half;
}
__device__ __forceinline__ unsigned perm_fmix32(unsigned h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ unsigned perm_encrypt(const PermKey& key, unsigned x) {
    const unsigned mask = (1u << key.half) - 1u;
    unsigned l = x >> key.half, r = x & mask;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned f = perm_fmix32(r ^ key.k[i]) >> (32 - key.half);
        const unsigned t = l ^ f;
        l = r;
        r = t;
    }
    return (l << key.half) | r;
}
// a bijection of [0, 2^bits) restricted to the cycle through i: the walk ends, and distinct i end on distinct values
__device__ __forceinline__ unsigned perm_index(const PermKey& key, unsigned i, unsigned long long n) {
    unsigned x = perm_encrypt(key, i);
    while ((unsigned long long)x >= n) x = perm_encrypt(key, x);
    return x;
}

// ---------------------------------------------------------------------------------------------------- R and t
// grid (ceil(b / 64)), one thread per slot
__global__ __launch_bounds__(GSPN_WAVE) void batch_draw_kernel(int b, const long long* __restrict__ seed_dev, int augment,
                                                               double* __restrict__ rotation, double* __restrict__ translation) {
    const int s = blockIdx.x * GSPN_WAVE + threadIdx.x;
    if (s >= b) return;
    double* R = rotation + (long)s * 9;
    double* t = translation + (long)s * 3;
    if (!augment) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        t[0] = t[1] = t[2] = 0.0;
        return;
    }
    const unsigned long long st = roi_rand_scene(seed_dev[0], s);
    const double two_pi = 6.283185307179586, inv32 = 1.0 / 4294967296.0;
    const double angle = (two_pi * (double)roi_rand32(st, GSPN_AUGMENT_STREAM, 0u)) * inv32;
    const double c = cos(angle), sn = sin(angle);
    R[0] = c;    R[1] = sn;  R[2] = 0.0;                             // dataset.py:131-133
    R[3] = -sn;  R[4] = c;   R[5] = 0.0;
    R[6] = 0.0;  R[7] = 0.0; R[8] = 1.0;
    // Box-Muller: pair p uses draws 1 + 2p (u1 in (0, 1]) and 2 + 2p (u2 in [0, 1)); t = (z0 of pair 0, z1 of pair 0, z0 of pair 1)
    double z[4];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const double u1 = ((double)roi_rand32(st, GSPN_AUGMENT_STREAM, 1u + 2u * p) + 1.0) * inv32;
        const double u2 = (double)roi_rand32(st, GSPN_AUGMENT_STREAM, 2u + 2u * p) * inv32;
        const double radius = sqrt(-2.0 * log(u1)), phi = two_pi * u2;
        z[2 * p] = radius * cos(phi);
        z[2 * p + 1] = radius * sin(phi);
    }
    t[0] = z[0];
    t[1] = z[1];
    t[2] = z[2];
}

// float((x0*R0 + x1*R1) + x2*R2 + t), dataset._rigid's order
__device__ __forceinline__ void rigid(const double (&R)[9], const double (&t)[3], const float (&x)[3], float (&y)[3]) {
    const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) y[a] = (float)(((x0 * R[a] + x1 * R[3 + a]) + x2 * R[6 + a]) + t[a]);
}

// ---------------------------------------------------------------------------------------------------- the points
// grid (ceil(n / BA_THREADS), b)
__global__ __launch_bounds__(BA_THREADS) void batch_points_kernel(int nscene, long n, const float* __restrict__ pc_all,
                                                                  const float* __restrict__ color_all, const int* __restrict__ group_all,
                                                                  const int* __restrict__ seg_all, const int* __restrict__ scene_idx,
                                                                  const long long* __restrict__ seed_dev, int permute, int augment,
                                                                  const double* __restrict__ rotation, const double* __restrict__ translation,
                                                                  float* __restrict__ pc, float* __restrict__ color, int* __restrict__ group_label,
                                                                  int* __restrict__ seg_label, float* __restrict__ smpw) {
    const int s = blockIdx.y;
    const long i = (long)blockIdx.x * BA_THREADS + threadIdx.x;
    if (i >= n) return;
    const int k = min(max(scene_idx[s], 0), nscene - 1);             // a bad scene index reads a wrong scene, never out of bounds
    long j = i;
    if (permute) {
        const unsigned long long st = roi_rand_scene(seed_dev[0], s);
        PermKey key;
#pragma unroll
        for (int r = 0; r < 4; ++r) key.k[r] = roi_rand32(st, GSPN_PERM_STREAM, (unsigned)r);
        key.half = perm_half_bits(n);
        j = (long)perm_index(key, (unsigned)i, (unsigned long long)n);
    }
    const long src = (long)k * n + j, dst = (long)s * n + i;
    float x[3] = {pc_all[3 * src], pc_all[3 * src + 1], pc_all[3 * src + 2]};
    const float c0 = color_all[3 * src], c1 = color_all[3 * src + 1], c2 = color_all[3 * src + 2];
    const int g = group_all[src], sg = seg_all[src];
    if (augment) {
        double R[9], t[3];
#pragma unroll
        for (int a = 0; a < 9; ++a) R[a] = rotation[(long)s * 9 + a];         // uniform across the workgroup
#pragma unroll
        for (int a = 0; a < 3; ++a) t[a] = translation[(long)s * 3 + a];
        float y[3];
        rigid(R, t, x, y);
        x[0] = y[0]; x[1] = y[1]; x[2] = y[2];
    }
    pc[3 * dst] = x[0];
    pc[3 * dst + 1] = x[1];
    pc[3 * dst + 2] = x[2];
    color[3 * dst] = c0;
    color[3 * dst + 1] = c1;
    color[3 * dst + 2] = c2;
    group_label[dst] = g;
    seg_label[dst] = sg;
    smpw[dst] = 1.0f;
}

// ---------------------------------------------------------------------------------------------------- the instance sets
// one wave per (slot, group) row, BA_WAVES rows per workgroup; the reduction is points_bbox_kernel's, in its order
__global__ __launch_bounds__(BA_THREADS) void batch_instances_kernel(int nscene, int b, int g, int m, const float* __restrict__ pc_ins_all,
                                                                     const int* __restrict__ ngroup_all, const int* __restrict__ scene_idx,
                                                                     int augment, const double* __restrict__ rotation,
                                                                     const double* __restrict__ translation, float* __restrict__ pc_ins,
                                                                     int* __restrict__ group_indicator, float* __restrict__ bbox_ins) {
    const int lane = threadIdx.x % GSPN_WAVE;
    const long r = (long)blockIdx.x * BA_WAVES + threadIdx.x / GSPN_WAVE;
    if (r >= (long)b * g) return;                                    // whole waves leave; no barrier below
    const int s = (int)(r / g), j = (int)(r % g);
    const int k = min(max(scene_idx[s], 0), nscene - 1);
    const float* p = pc_ins_all + ((long)k * g + j) * m * 3;
    float* q = pc_ins + r * m * 3;
    double R[9], t[3];
#pragma unroll
    for (int a = 0; a < 9; ++a) R[a] = rotation[(long)s * 9 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = translation[(long)s * 3 + a];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = lane; i < m; i += GSPN_WAVE) {
        float x[3] = {p[3 * (long)i], p[3 * (long)i + 1], p[3 * (long)i + 2]};
        if (augment) {
            float y[3];
            rigid(R, t, x, y);
            x[0] = y[0]; x[1] = y[1]; x[2] = y[2];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            q[3 * (long)i + a] = x[a];
            mx[a] = fmaxf(mx[a], x[a]);
            mn[a] = fminf(mn[a], x[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mx[a] = wave_max_f32(mx[a]);
        mn[a] = wave_min_f32(mn[a]);
    }
    if (lane == 0) {
        float* o = bbox_ins + r * 6;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            o[a] = (mx[a] + mn[a]) / 2.0f;
            o[3 + a] = mx[a] - mn[a];
        }
        group_indicator[r] = j < ngroup_all[k] ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------- the optimisers
// tf.train.AdamOptimizer: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t) (on the host, in double);  p -= lr_t * m / (sqrt(v) + eps)
__global__ void adam_tf_flat_kernel(long n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                    float lr_t, float b1, float b2, float eps, float grad_scale) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float gi = g[i] * grad_scale;
        const float mi = m[i] + (gi - m[i]) * (1.f - b1);                   // training_ops: m += (g - m) * (1 - beta1)
        const float vi = v[i] + (gi * gi - v[i]) * (1.f - b2);
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - (mi * lr_t) / (sqrtf(vi) + eps);
    }
}

// tf.train.MomentumOptimizer (use_nesterov=False): accum = momentum * accum + g;  p -= lr * accum
__global__ void momentum_flat_kernel(long n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ accum, float lr,
                                     float momentum, float grad_scale) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float ai = momentum * accum[i] + g[i] * grad_scale;
        accum[i] = ai;
        p[i] = p[i] - lr * ai;
    }
}

// ---------------------------------------------------------------------------------------------------- the running sums
struct ScalarPtrs {
    const float* p[GSPN_SCALARS_MAX];
};
__global__ __launch_bounds__(GSPN_WAVE) void scalars_accumulate_kernel(int k, ScalarPtrs ptrs, double* __restrict__ sums, long long* __restrict__ count) {
    const int i = threadIdx.x;
    if (i < k) sums[i] = sums[i] + (double)ptrs.p[i][0];
    if (i == 0) count[0] = count[0] + 1;
}

}  // namespace

extern "C" int gspn_batch_assemble(int nscene, int b, long n, int g, int m, const float* pc_all, const float* color_all, const int* group_all,
                                   const int* seg_all, const float* pc_ins_all, const int* ngroup_all, const int* scene_idx,
                                   const long long* seed_dev, int permute, int augment, float* pc, float* color, int* group_label,
                                   int* seg_label, float* pc_ins, int* group_indicator, float* bbox_ins, float* smpw, double* rotation,
                                   double* translation, void* stream) {
    if (nscene <= 0 || b <= 0 || n <= 0 || g <= 0 || m <= 0) return GSPN_ERR_ARG;
    if (!pc_all || !color_all || !group_all || !seg_all || !pc_ins_all || !ngroup_all || !scene_idx || !seed_dev || !pc || !color ||
        !group_label || !seg_label || !pc_ins || !group_indicator || !bbox_ins || !smpw || !rotation || !translation)
        return GSPN_ERR_ARG;
    if (n > (1l << 31) || b > 65535 || (long)b * g > (1l << 31) - BA_WAVES) return GSPN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    batch_draw_kernel<<<(b + GSPN_WAVE - 1) / GSPN_WAVE, GSPN_WAVE, 0, st>>>(b, seed_dev, augment, rotation, translation);
    batch_points_kernel<<<dim3((unsigned)((n + BA_THREADS - 1) / BA_THREADS), b), BA_THREADS, 0, st>>>(
        nscene, n, pc_all, color_all, group_all, seg_all, scene_idx, seed_dev, permute, augment, rotation, translation, pc, color, group_label,
        seg_label, smpw);
    const long rows = (long)b * g;
    batch_instances_kernel<<<(unsigned)((rows + BA_WAVES - 1) / BA_WAVES), BA_THREADS, 0, st>>>(
        nscene, b, g, m, pc_ins_all, ngroup_all, scene_idx, augment, rotation, translation, pc_ins, group_indicator, bbox_ins);
    return gspn_launch_status();
}

// step >= 1 is the number of this update; the bias terms are computed here in double, as gspn_adam_flat does
extern "C" int gspn_adam_tf_flat(long n, float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps, float grad_scale,
                                 long step, void* stream) {
    if (n < 0 || step < 1) return GSPN_ERR_ARG;
    if (n == 0) return 0;
    if (!p || !g || !m || !v) return GSPN_ERR_ARG;
    const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
    const float lr_t = (float)((double)lr * sqrt(bc2) / bc1);
    hipLaunchKernelGGL(adam_tf_flat_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, n, p, g, m, v, lr_t, b1, b2, eps, grad_scale);
    return gspn_launch_status();
}

extern "C" int gspn_momentum_flat(long n, float* p, const float* g, float* accum, float lr, float momentum, float grad_scale, void* stream) {
    if (n < 0) return GSPN_ERR_ARG;
    if (n == 0) return 0;
    if (!p || !g || !accum) return GSPN_ERR_ARG;
    hipLaunchKernelGGL(momentum_flat_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, n, p, g, accum, lr, momentum, grad_scale);
    return gspn_launch_status();
}

// ptrs: k device pointers in HOST memory; they travel to the kernel by value
extern "C" int gspn_scalars_accumulate(int k, const float* const* ptrs, double* sums, long long* count, void* stream) {
    if (k < 1 || k > GSPN_SCALARS_MAX || !ptrs || !sums || !count) return GSPN_ERR_ARG;
    ScalarPtrs a;
    for (int i = 0; i < GSPN_SCALARS_MAX; ++i) {
        a.p[i] = i < k ? ptrs[i] : nullptr;
        if (i < k && !a.p[i]) return GSPN_ERR_ARG;
    }
    hipLaunchKernelGGL(scalars_accumulate_kernel, dim3(1), dim3(GSPN_WAVE), 0, (hipStream_t)stream, k, a, sums, count);
    return gspn_launch_status();
}
