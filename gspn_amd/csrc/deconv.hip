// deconv.hip -- tf_util.conv2d_transpose (tf.layers.conv2d_transpose, VALID, NHWC, fp32) on the FP32 MFMA (ABI 11).
//
//   Ho = Hi*sh + max(kh - sh, 0)   (Wo alike)
//   Y[n, oy, ox, co] = bias[co] + sum over (iy, ix, ky, kx) with iy*sh + ky == oy, ix*sw + kx == ox of X[n, iy, ix, ci] * K[ky, kx, co, ci]
//   K is (kh, kw, Cout, Cin), no flip.  Output pixels no tap reaches (k < s) hold bias only.
//
// All three kernels are implicit GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32 products, a k-ordered fma chain) through one LDS-tiled
// kernel body (dc_gemm_kernel); an operand "op" only says how a tile element is fetched and where a result goes.  Nothing is expanded to
// an im2col / col2im buffer.
//   forward     one GEMM per output phase (py, px) = (oy mod sh, ox mod sw), blockIdx.z: the taps ky = py + sh*ty form a dense stride-1
//               correlation, M = n * phase pixels, N = Cout, K = Cin * phase taps; input rows that fall outside the map read as 0.
//               (A 1-pixel input dimension is run with stride max(k, s): the same output, one tap per phase instead of k masked ones.)
//   grad-input  dX[n, iy, ix, ci] = sum over (ky, kx, co) of dY[n, iy*sh + ky, ix*sw + kx, co] * K[ky, kx, co, ci]:
//               M = n*Hi*Wi, N = Cin, K = kh*kw*Cout; every tap lands inside dY, and B is K itself read as a (kh*kw*Cout, Cin) matrix.
//   grad-kernel per tap dK[ky, kx]^T (Cin x Cout) = X^T . dY[tap-shifted pixels], the reduction over n*Hi*Wi rows cut into S splits
//               (blockIdx.z = tap*S + split); S > 1 writes partial tiles to the workspace and a second kernel adds them split by split.
//               dbias = column sums of dY over fixed row chunks, then the chunks in order.
// No atomics anywhere: every sum has a fixed order, so two identical calls give identical bits.
#include <stdint.h>

#include "mlp_common.h"

#define DC_TK 16                  // k per LDS stage
#define DC_THREADS 256            // 4 waves

namespace {

struct DcShape { int n, hi, wi, cin, cout, kh, kw, sh, sw, ho, wo; };
struct DcArgs {
    DcShape s;
    const float* A;               // forward: X;  grad-input: dY;  grad-kernel: X
    const float* B;               // forward / grad-input: K;  grad-kernel: dY
    const float* bias;            // forward only (may be NULL)
    float* out;                   // Y / dX / dK or the partial tiles
    int S, kc;                    // grad-kernel: splits and rows per split
};

// which tile element thread t fetches as its i-th value: KC (contiguous along k, the channel dimension of NHWC rows) -> the 16 threads of a
// row read 16 consecutive floats;  otherwise contiguous along the tile's row dimension, each thread reading E consecutive k of one row.
template <bool KC, int R> struct DcMap {
    static constexpr int E = R * DC_TK / DC_THREADS;
    __device__ static int row(int t, int i) { return KC ? t / DC_TK + (DC_THREADS / DC_TK) * i : t % R; }
    __device__ static int kk(int t, int i) { return KC ? t % DC_TK : (t / R) * E + i; }
};

// ---------------------------------------------------------------------------------------------------- forward, one output phase
template <int BM, int BN> struct FwdOp {
    static constexpr bool A_KC = true, B_KC = true;
    using MA = DcMap<true, BM>;
    using MB = DcMap<true, BN>;
    DcArgs a;
    int t, py, px, hq, wq, tyn, txn, M, kdepth;
    int qy[MA::E], qx[MA::E];
    long xb[MA::E];               // first pixel of the row's image in X; -1: row outside M
    int co[MB::E];                // -1: outside Cout

    __device__ bool begin(const DcArgs& args, int z, int m0, int n0, int tid) {
        a = args; t = tid;
        const DcShape& s = a.s;
        py = z / s.sw; px = z - py * s.sw;
        hq = (s.ho - py + s.sh - 1) / s.sh;
        wq = (s.wo - px + s.sw - 1) / s.sw;
        tyn = py < s.kh ? (s.kh - py + s.sh - 1) / s.sh : 0;
        txn = px < s.kw ? (s.kw - px + s.sw - 1) / s.sw : 0;
        M = s.n * hq * wq;
        if (m0 >= M || n0 >= s.cout) return false;
        kdepth = tyn * txn * s.cin;
        const int pp = hq * wq;
#pragma unroll
        for (int i = 0; i < MA::E; ++i) {
            const int m = m0 + MA::row(t, i);
            const int img = m / pp, rem = m - img * pp;
            qy[i] = rem / wq;
            qx[i] = rem - qy[i] * wq;
            xb[i] = m < M ? (long)img * s.hi * s.wi : -1;
        }
#pragma unroll
        for (int i = 0; i < MB::E; ++i) {
            const int c = n0 + MB::row(t, i);
            co[i] = c < s.cout ? c : -1;
        }
        return true;
    }
    __device__ void load(int k0, float* ra, float* rb) const {
        const DcShape& s = a.s;
        const int k = k0 + t % DC_TK;                       // the one k of this thread in both operands
        const bool kok = k < kdepth;
        const int tap = kok ? k / s.cin : 0, ci = k - tap * s.cin;
        const int ty = tap / txn, tx = tap - ty * txn;
#pragma unroll
        for (int i = 0; i < MA::E; ++i) {
            const int iy = qy[i] - ty, ix = qx[i] - tx;
            const bool ok = kok && xb[i] >= 0 && (unsigned)iy < (unsigned)s.hi && (unsigned)ix < (unsigned)s.wi;
            ra[i] = ok ? a.A[(xb[i] + (long)iy * s.wi + ix) * s.cin + ci] : 0.f;
        }
        const long kb = (long)((py + s.sh * ty) * s.kw + px + s.sw * tx) * s.cout;
#pragma unroll
        for (int i = 0; i < MB::E; ++i) rb[i] = (kok && co[i] >= 0) ? a.B[(kb + co[i]) * s.cin + ci] : 0.f;
    }
    __device__ void put(int m, int c, float v) const {
        const DcShape& s = a.s;
        if (m >= M || c >= s.cout) return;
        const int pp = hq * wq;
        const int img = m / pp, rem = m - img * pp, y = rem / wq, x = rem - y * wq;
        const long pix = ((long)img * s.ho + py + s.sh * y) * s.wo + px + s.sw * x;
        a.out[pix * s.cout + c] = v + (a.bias ? a.bias[c] : 0.f);
    }
};

// ---------------------------------------------------------------------------------------------------- grad-input
template <int BM, int BN> struct BwdInOp {
    static constexpr bool A_KC = true, B_KC = false;
    using MA = DcMap<true, BM>;
    using MB = DcMap<false, BN>;
    DcArgs a;
    int t, M, kdepth, ci;
    long pb[MA::E];               // dY pixel of tap (0, 0) for the row; -1: row outside M

    __device__ bool begin(const DcArgs& args, int z, int m0, int n0, int tid) {
        a = args; t = tid;
        const DcShape& s = a.s;
        M = s.n * s.hi * s.wi;
        if (m0 >= M || n0 >= s.cin) return false;
        kdepth = s.kh * s.kw * s.cout;
        const int pp = s.hi * s.wi;
#pragma unroll
        for (int i = 0; i < MA::E; ++i) {
            const int m = m0 + MA::row(t, i);
            const int img = m / pp, rem = m - img * pp, iy = rem / s.wi, ix = rem - iy * s.wi;
            pb[i] = m < M ? ((long)img * s.ho + (long)iy * s.sh) * s.wo + (long)ix * s.sw : -1;
        }
        ci = n0 + MB::row(t, 0);
        return true;
    }
    __device__ void load(int k0, float* ra, float* rb) const {
        const DcShape& s = a.s;
        const int k = k0 + t % DC_TK;
        const bool kok = k < kdepth;
        const int tap = kok ? k / s.cout : 0, co = k - tap * s.cout;
        const int ky = tap / s.kw, kx = tap - ky * s.kw;
        const long kp = (long)ky * s.wo + kx;
#pragma unroll
        for (int i = 0; i < MA::E; ++i) ra[i] = (kok && pb[i] >= 0) ? a.A[(pb[i] + kp) * s.cout + co] : 0.f;
#pragma unroll
        for (int i = 0; i < MB::E; ++i) {
            const int kb = k0 + MB::kk(t, i);
            rb[i] = (kb < kdepth && ci < s.cin) ? a.B[(long)kb * s.cin + ci] : 0.f;
        }
    }
    __device__ void put(int m, int c, float v) const {
        if (m < M && c < a.s.cin) a.out[(long)m * a.s.cin + c] = v;
    }
};

// ---------------------------------------------------------------------------------------------------- grad-kernel: one (tap, split)
template <int BM, int BN> struct BwdKOp {
    static constexpr bool A_KC = false, B_KC = false;
    using MA = DcMap<false, BM>;
    using MB = DcMap<false, BN>;
    DcArgs a;
    int t, tap, split, ky, kx, kbeg, kdepth, ci, co;

    __device__ bool begin(const DcArgs& args, int z, int m0, int n0, int tid) {
        a = args; t = tid;
        const DcShape& s = a.s;
        if (m0 >= s.cin || n0 >= s.cout) return false;
        tap = z / a.S; split = z - tap * a.S;
        ky = tap / s.kw; kx = tap - ky * s.kw;
        const int R = s.n * s.hi * s.wi;
        kbeg = split * a.kc;
        kdepth = min(a.kc, R - kbeg);
        ci = m0 + MA::row(t, 0);
        co = n0 + MB::row(t, 0);
        return true;
    }
    __device__ void load(int k0, float* ra, float* rb) const {
        const DcShape& s = a.s;
        const int ka = k0 + MA::kk(t, 0);
#pragma unroll
        for (int i = 0; i < MA::E; ++i)
            ra[i] = (ka + i < kdepth && ci < s.cin) ? a.A[(long)(kbeg + ka + i) * s.cin + ci] : 0.f;
        const int kb = k0 + MB::kk(t, 0);
        int r = kbeg + kb;                                  // (n, iy, ix) of the first row, then stepped
        const int pp = s.hi * s.wi;
        int img = r / pp, rem = r - img * pp, iy = rem / s.wi, ix = rem - iy * s.wi;
#pragma unroll
        for (int i = 0; i < MB::E; ++i) {
            const bool ok = kb + i < kdepth && co < s.cout;
            const long pix = ((long)img * s.ho + (long)iy * s.sh + ky) * s.wo + (long)ix * s.sw + kx;
            rb[i] = ok ? a.B[pix * s.cout + co] : 0.f;
            if (++ix == s.wi) { ix = 0; if (++iy == s.hi) { iy = 0; ++img; } }
        }
    }
    __device__ void put(int m, int c, float v) const {
        const DcShape& s = a.s;
        if (m >= s.cin || c >= s.cout) return;
        const long T = (long)s.kh * s.kw * s.cout * s.cin;
        a.out[(a.S > 1 ? split * T : 0) + ((long)tap * s.cout + c) * s.cin + m] = v;
    }
};

// ---------------------------------------------------------------------------------------------------- the GEMM body
// 4 waves as WGM x WGN, each owning FM x FN tiles of 32x32; block tile BM x BN = (WGM*FM*32) x (WGN*FN*32).  Both operands are staged
// K-major in LDS ([k][row], pitch +1); the next stage's global loads are in flight while the current stage's MFMAs run.
template <class Op, int WGM, int WGN, int FM, int FN>
__global__ __launch_bounds__(DC_THREADS) void dc_gemm_kernel(DcArgs args) {
    constexpr int BM = WGM * FM * 32, BN = WGN * FN * 32;
    constexpr int LDA = BM + 1, LDB = BN + 1;
    static_assert(WGM * WGN == 4, "four waves");
    using MA = DcMap<Op::A_KC, BM>;
    using MB = DcMap<Op::B_KC, BN>;
    __shared__ float sA[DC_TK * LDA];
    __shared__ float sB[DC_TK * LDB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int wm = (wave / WGN) * FM * 32, wn = (wave % WGN) * FN * 32;
    Op op;
    if (!op.begin(args, blockIdx.z, m0, n0, t)) return;          // (block-uniform)
    const int nch = (op.kdepth + DC_TK - 1) / DC_TK;
    float ra[MA::E], rb[MB::E];
    f32x16 acc[FM][FN];
#pragma unroll
    for (int x = 0; x < FM; ++x)
#pragma unroll
        for (int y = 0; y < FN; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < MA::E; ++i) sA[MA::kk(t, i) * LDA + MA::row(t, i)] = ra[i];
#pragma unroll
        for (int i = 0; i < MB::E; ++i) sB[MB::kk(t, i) * LDB + MB::row(t, i)] = rb[i];
    };
    if (nch > 0) {
        op.load(0, ra, rb);
        stage();
    }
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) op.load((c + 1) * DC_TK, ra, rb);
#pragma unroll
        for (int kp = 0; kp < DC_TK; kp += 2) {
            const int kr = kp + (lane >> 5);
            float av[FM], bv[FN];
#pragma unroll
            for (int x = 0; x < FM; ++x) av[x] = sA[kr * LDA + wm + x * 32 + (lane & 31)];
#pragma unroll
            for (int y = 0; y < FN; ++y) bv[y] = sB[kr * LDB + wn + y * 32 + (lane & 31)];
#pragma unroll
            for (int x = 0; x < FM; ++x)
#pragma unroll
                for (int y = 0; y < FN; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[x], bv[y], acc[x][y], 0, 0, 0);
        }
        __syncthreads();
        if (c + 1 < nch) {
            stage();
            __syncthreads();
        }
    }
#pragma unroll
    for (int x = 0; x < FM; ++x)
#pragma unroll
        for (int y = 0; y < FN; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) op.put(m0 + wm + x * 32 + c_row(r, lane), n0 + wn + y * 32 + (lane & 31), acc[x][y][r]);
}

// out[i] = sum over p = 0 .. nparts-1 of part[p*total + i], in that order
__global__ void dc_sum_parts_kernel(long total, int nparts, const float* __restrict__ part, float* __restrict__ out) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int p = 0; p < nparts; ++p) v += part[p * total + i];
        out[i] = v;
    }
}

// part[blockIdx.x][c] = sum of dY[r][c] over the block's chunk of rows: each thread sums a strided run of one column, the runs of a
// column are then added in lane order
__global__ __launch_bounds__(256) void dc_bias_part_kernel(long rows, int c, long rchunk, const float* __restrict__ dY, float* __restrict__ part) {
    __shared__ float red[256];
    const int t = threadIdx.x;
    const long r0 = blockIdx.x * rchunk, r1 = min(rows, r0 + rchunk);
    for (int cb = 0; cb < c; cb += 256) {
        const int cw = min(256, c - cb), lanes = 256 / cw;
        const int col = t % cw, rl = t / cw;
        float s = 0.f;
        if (rl < lanes)
            for (long r = r0 + rl; r < r1; r += lanes) s += dY[r * c + cb + col];
        red[t] = s;
        __syncthreads();
        if (t < cw) {
            float v = 0.f;
            for (int l = 0; l < lanes; ++l) v += red[l * cw + t];
            part[(long)blockIdx.x * c + cb + t] = v;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------- host side
int dc_shape(int n, int hi, int wi, int cin, int cout, int kh, int kw, int sh, int sw, DcShape* s) {
    if (n < 1 || hi < 1 || wi < 1 || cin < 1 || cout < 1 || kh < 1 || kw < 1 || sh < 1 || sw < 1) return GSPN_ERR_ARG;
    const long long ho = (long long)hi * sh + (kh > sh ? kh - sh : 0), wo = (long long)wi * sw + (kw > sw ? kw - sw : 0);
    const long long lim = 1ll << 30;                   // every row / k index of the kernels stays far inside an int
    if (ho * wo * n > lim || (long long)kh * kw * cin * cout > lim || (long long)sh * sw > 65535 || (long long)kh * kw > 65535)
        return GSPN_ERR_UNSUPPORTED;
    *s = DcShape{n, hi, wi, cin, cout, kh, kw, sh, sw, (int)ho, (int)wo};
    return 0;
}

template <class Op, int WGM, int WGN, int FM, int FN>
void dc_launch(const DcArgs& a, int M, int N, int Z, hipStream_t st) {
    constexpr int BM = WGM * FM * 32, BN = WGN * FN * 32;
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((N + BN - 1) / BN), (unsigned)Z);
    hipLaunchKernelGGL((dc_gemm_kernel<Op, WGM, WGN, FM, FN>), grid, dim3(DC_THREADS), 0, st, a);
}

// tile choice: 128 x 32 for N <= 32 (the 3-channel layers), 64 x 64 where 128 x 128 tiles would not fill the GPU once, else 128 x 128
template <template <int, int> class OpT>
void dc_run(const DcArgs& a, int M, int N, int Z, bool allow_mid, hipStream_t st) {
    if (N <= 32) dc_launch<OpT<128, 32>, 4, 1, 1, 1>(a, M, N, Z, st);
    else if (allow_mid && (long)((M + 127) / 128) * ((N + 127) / 128) * Z < 256) dc_launch<OpT<64, 64>, 2, 2, 1, 1>(a, M, N, Z, st);
    else dc_launch<OpT<128, 128>, 2, 2, 2, 2>(a, M, N, Z, st);
}

// grad-kernel plan, a function of the shape alone: splits S of the n*Hi*Wi reduction rows (about 512 workgroups, at least 256 rows each),
// and the row chunks of the bias reduction
struct DcKPlan { int S, kc, P; long rchunk; long part_floats, bias_floats; };
DcKPlan dc_kplan(const DcShape& s) {
    DcKPlan p;
    const long R = (long)s.n * s.hi * s.wi;
    const long taps = (long)s.kh * s.kw;
    const long base = taps * ((s.cin + 127) / 128) * (s.cout <= 32 ? 1 : (s.cout + 127) / 128);
    long S = (512 + base - 1) / base;
    const long smax = R / 256 > 1 ? R / 256 : 1;
    if (S > smax) S = smax;
    if (S * taps > 65535) S = 65535 / taps;
    if (S < 1) S = 1;
    long kc = (R + S - 1) / S;
    kc = (kc + DC_TK - 1) / DC_TK * DC_TK;
    p.kc = (int)kc;
    p.S = (int)((R + kc - 1) / kc);
    const long rows = (long)s.n * s.ho * s.wo;
    long P = rows / 64;
    P = P < 1 ? 1 : (P > 256 ? 256 : P);
    p.rchunk = (rows + P - 1) / P;
    p.P = (int)((rows + p.rchunk - 1) / p.rchunk);
    p.part_floats = p.S > 1 ? (long)p.S * taps * s.cout * s.cin : 0;
    p.bias_floats = (long)p.P * s.cout;
    return p;
}

}  // namespace

extern "C" int gspn_deconv_fwd(int n, int hi, int wi, int cin, int cout, int kh, int kw, int sh, int sw, const float* X, const float* K,
                               const float* bias, float* Y, void* stream) {
    DcShape s;
    const int rc = dc_shape(n, hi, wi, cin, cout, kh, kw, sh, sw, &s);
    if (rc) return rc;
    if (!X || !K || !Y) return GSPN_ERR_ARG;
    // a 1-pixel input dimension: oy = ky whatever the stride, so run it with stride max(k, s) -- one tap per phase, nothing masked
    if (s.hi == 1 && s.kh > s.sh) s.sh = s.kh;
    if (s.wi == 1 && s.kw > s.sw) s.sw = s.kw;
    DcArgs a{s, X, K, bias, Y, 1, 0};
    const int M = s.n * ((s.ho + s.sh - 1) / s.sh) * ((s.wo + s.sw - 1) / s.sw);     // phase (0, 0), the largest
    dc_run<FwdOp>(a, M, s.cout, s.sh * s.sw, true, (hipStream_t)stream);
    return gspn_launch_status();
}

extern "C" int gspn_deconv_bwd_input(int n, int hi, int wi, int cin, int cout, int kh, int kw, int sh, int sw, const float* dY, const float* K,
                                     float* dX, void* stream) {
    DcShape s;
    const int rc = dc_shape(n, hi, wi, cin, cout, kh, kw, sh, sw, &s);
    if (rc) return rc;
    if (!dY || !K || !dX) return GSPN_ERR_ARG;
    DcArgs a{s, dY, K, nullptr, dX, 1, 0};
    dc_run<BwdInOp>(a, s.n * s.hi * s.wi, s.cin, 1, true, (hipStream_t)stream);
    return gspn_launch_status();
}

extern "C" long gspn_deconv_bwd_kernel_work_bytes(int n, int hi, int wi, int cin, int cout, int kh, int kw, int sh, int sw) {
    DcShape s;
    if (dc_shape(n, hi, wi, cin, cout, kh, kw, sh, sw, &s)) return 0;
    const DcKPlan p = dc_kplan(s);
    return (p.part_floats + p.bias_floats) * (long)sizeof(float);
}

extern "C" int gspn_deconv_bwd_kernel(int n, int hi, int wi, int cin, int cout, int kh, int kw, int sh, int sw, const float* dY, const float* X,
                                      float* dK, float* dbias, void* ws, void* stream) {
    DcShape s;
    const int rc = dc_shape(n, hi, wi, cin, cout, kh, kw, sh, sw, &s);
    if (rc) return rc;
    if (!dY || !X || (!dK && !dbias) || !ws) return GSPN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const DcKPlan p = dc_kplan(s);
    float* part = static_cast<float*>(ws);
    float* bpart = part + p.part_floats;
    if (dK) {
        DcArgs a{s, X, dY, nullptr, p.S > 1 ? part : dK, p.S, p.kc};
        dc_run<BwdKOp>(a, s.cin, s.cout, s.kh * s.kw * p.S, false, st);
        if (p.S > 1) {
            const long T = (long)s.kh * s.kw * s.cout * s.cin;
            hipLaunchKernelGGL(dc_sum_parts_kernel, dim3(grid_for(T, 256)), dim3(256), 0, st, T, p.S, (const float*)part, dK);
        }
    }
    if (dbias) {
        const long rows = (long)s.n * s.ho * s.wo;
        hipLaunchKernelGGL(dc_bias_part_kernel, dim3(p.P), dim3(256), 0, st, rows, s.cout, p.rchunk, dY, bpart);
        hipLaunchKernelGGL(dc_sum_parts_kernel, dim3(grid_for(s.cout, 256)), dim3(256), 0, st, (long)s.cout, p.P, (const float*)bpart, dbias);
    }
    return gspn_launch_status();
}
