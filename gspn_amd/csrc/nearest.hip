// nearest.hip -- nearest_point: the exact one-nearest neighbour of every query among the known points of its scene, over a cell grid that
// lives in GLOBAL memory and is built once per call.  The result is the first column of gspn_threenn bit for bit: the
// distance is the reference's unfused fp32 (dx*dx + dy*dy) + dz*dz (dist2_host, tf_interpolate.cpp:71-74), the lowest index wins among
// equal distances, a NaN or +inf distance never wins, a query without a winner keeps (+inf, 0) (the reference's 1e40 initialisation).
//
// three_nn's LDS grid (interpolate.hip) rebuilds its grid in every workgroup and stops at 8192 known points; a scene has 18 000 to 32 768
// and a scan's mesh brings several hundred thousand queries to it.  Here the build is six short launches over the workspace:
//   init     zero the cell counters, reset the bounding-box keys                                  (grid-stride)
//   bbox     bounding box per scene: a workgroup reduces its share, integer atomicMin / atomicMax on order-preserving keys of the floats
//   plan     one thread per scene: cells per axis (they differ: near-cubic cells for an 8 x 8 x 3 m room), lo / inv / h
//   hist     cell of every known point and its rank inside the cell from the counter's integer atomicAdd, both kept
//   scan     exclusive scan of the counters into the (cells + 1) start table, one workgroup per scene (the table has at most NP_MAX_CELLS entries)
//   scatter  (x, y, z, bits of k) as float4 to start[cell] + rank: sorted by cell (the cell hist kept, so the two cannot disagree)
// bbox, hist and scatter spread over ceil(m / 1024) workgroups per scene.  Integer atomics only; the order of the points inside a cell is
// whatever the atomics gave, so the query compares (d, k) pairs explicitly and its result does not depend on that order.
//
// Query: one thread per query, 256 per workgroup.  It scans the 3 x 3 x 3 block of cells around the query's clamped cell and accepts iff the
// best distance is strictly below the squared, 0.999-shrunk distance to every face of the block that has cells behind it (three_nn_grid_kernel's
// test with one candidate); otherwise it goes on over every cell the ball of radius sqrt(b1) * 1.001 touches, or, when the block was empty,
// over blocks of twice the reach until one holds a point or every cell was read.  The query's own row of cells goes first and what it finds
// prunes the rest: a cell whose shrunk distance from the query exceeds the best one is not read.  Box-relative arithmetic throughout: q - lo is the subtraction the cell assignment performs, never lo + c * h (ADVICE r04:
// coordinates around 5e5 with a small extent).  A flat or non-finite axis puts every point in cell 0 of that axis and contributes no face.
// A query far outside the box, or in a hollow of the cloud, finds its block empty or its ball wide and degrades towards a scan of all known
// points; it stays correct.
// About NP_CELL_POINTS points per cell, at most NP_MAX_CELLS cells per scene (beyond 2^18 known points the cells simply hold more).
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "float_keys.h"                  // np_key, np_unkey

#define NP_T 256
#define NP_SCAN_T 1024
#define NP_CELL_POINTS 4                 // the target of GSPN_NN_CELL_POINTS (interpolate.hip)
#define NP_MAX_CELLS (1 << 16)           // the cap of the start table: 256 KiB of counters and of starts per scene, one workgroup scans it
#define NP_BUILD_PPT 4                   // known points per thread of bbox / hist / scatter
#define NP_BUILD_MAX_WPS 2048            // workgroups per scene of those three at most (they stride beyond)

// per scene, 128 bytes of the workspace
struct NpPlan {
    int klo[3], khi[3];                  // bounding box as order-preserving integer keys (bbox)
    float lo[3], inv[3], h[3];           // plan: box origin, cells per unit (0 on a flat / non-finite / single-cell axis), cell size
    int G[3];                            // cells per axis, G[0] * G[1] * G[2] <= cells
    float eps;                           // 1e-6 of the largest extent: above the rounding of (x - lo) * inv for a point of the box
    int pad[13];
};
static_assert(sizeof(NpPlan) == 128, "NpPlan is 32 words");

static inline int np_cells(int m) {
    const int c = m / NP_CELL_POINTS;
    return c < 1 ? 1 : (c > NP_MAX_CELLS ? NP_MAX_CELLS : c);
}
struct NpLayout { size_t pts, hdr, cnt, start, slot, bytes; int cells; };
static inline NpLayout np_layout(int b, int m) {
    NpLayout l;
    l.cells = np_cells(m);
    l.pts = 0;                                                               // float4[b][m], sorted by cell
    l.hdr = l.pts + sizeof(float4) * (size_t)b * m;                          // NpPlan[b]
    l.cnt = l.hdr + sizeof(NpPlan) * (size_t)b;                              // int[b][cells]
    l.start = l.cnt + sizeof(int) * (size_t)b * l.cells;                     // int[b][cells + 1]
    l.slot = (l.start + sizeof(int) * (size_t)b * (l.cells + 1) + 7) & ~(size_t)7;          // int2[b][m]: (cell, rank inside it) of known point k
    l.bytes = l.slot + sizeof(int2) * (size_t)b * m;
    return l;
}
static inline int np_build_wps(int m) {
    const int w = (m + NP_T * NP_BUILD_PPT - 1) / (NP_T * NP_BUILD_PPT);
    return w < 1 ? 1 : (w > NP_BUILD_MAX_WPS ? NP_BUILD_MAX_WPS : w);
}


__global__ __launch_bounds__(NP_T) void nearest_init_kernel(int b, long ncnt, NpPlan* __restrict__ hdr, int* __restrict__ cnt) {
    for (long i = blockIdx.x * (long)NP_T + threadIdx.x; i < ncnt; i += (long)gridDim.x * NP_T) {
        cnt[i] = 0;
        if (i < b) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { hdr[i].klo[a] = INT_MAX; hdr[i].khi[a] = INT_MIN; }
        }
    }
}

__global__ __launch_bounds__(NP_T) void nearest_bbox_kernel(int m, int wps, const float* __restrict__ xyz2, NpPlan* __restrict__ hdr) {
    __shared__ float s_red[6][NP_T / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int scene = blockIdx.x / wps, w = blockIdx.x - scene * wps;
    const float* sp = xyz2 + (size_t)scene * m * 3;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = w * NP_T + t; k < m; k += wps * NP_T) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = sp[(size_t)k * 3 + a];                           // fminf / fmaxf pass over a NaN
            lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int sft = 32; sft >= 1; sft >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], sft, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], sft, 64)); }
        if (lane == 0) { s_red[a][wave] = lo[a]; s_red[3 + a][wave] = hi[a]; }
    }
    __syncthreads();
    if (t < 3) {
        const float l = fminf(fminf(s_red[t][0], s_red[t][1]), fminf(s_red[t][2], s_red[t][3]));
        const float h = fmaxf(fmaxf(s_red[3 + t][0], s_red[3 + t][1]), fmaxf(s_red[3 + t][2], s_red[3 + t][3]));
        if (l <= h) {                                                        // this workgroup saw a coordinate that is not NaN
            atomicMin(&hdr[scene].klo[t], np_key(l));
            atomicMax(&hdr[scene].khi[t], np_key(h));
        }
    }
}

// Cells per axis for a box of extents ext and a budget of `cells`: cells of side s = (volume / cells)^(1/axes) over the axes that have an
// extent, floor(ext / s) of them per axis -- the product stays within the budget --; an axis shorter than one such cell is taken out
// (one cell) and the side recomputed over the others.
__global__ void nearest_plan_kernel(int b, int cells, NpPlan* __restrict__ hdr) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= b) return;
    float lo[3], ext[3];
    bool act[3];
    int G[3] = {1, 1, 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = np_unkey(hdr[s].klo[a]);
        ext[a] = np_unkey(hdr[s].khi[a]) - lo[a];
        act[a] = ext[a] > 0.f && isfinite(ext[a]);
    }
    for (int pass = 0; pass < 3; ++pass) {
        const int na = (int)act[0] + (int)act[1] + (int)act[2];
        if (na == 0) break;
        double vol = 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) if (act[a]) vol *= (double)ext[a];
        const double r = vol / (double)cells;
        const double side = na == 3 ? cbrt(r) : (na == 2 ? sqrt(r) : r);
        bool dropped = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!act[a]) continue;
            const double g = floor((double)ext[a] / side);
            if (!(g >= 1.0)) { act[a] = false; G[a] = 1; dropped = true; }
            else G[a] = (int)fmin(g, (double)cells);
        }
        if (!dropped) break;
    }
    while ((long long)G[0] * G[1] * G[2] > (long long)cells) {               // (rounding of side: never more cells than the table holds)
        const int a = G[0] >= G[1] && G[0] >= G[2] ? 0 : (G[1] >= G[2] ? 1 : 2);
        --G[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool on = act[a] && G[a] > 1;
        hdr[s].lo[a] = lo[a];
        hdr[s].inv[a] = on ? (float)G[a] / ext[a] : 0.f;
        hdr[s].h[a] = on ? ext[a] / (float)G[a] : 0.f;
        hdr[s].G[a] = on ? G[a] : 1;
    }
    float top = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) if (act[a]) top = fmaxf(top, ext[a]);
    hdr[s].eps = 1e-6f * top;
}

// cell coordinate along one axis: clamped in float, so that NaN (a NaN coordinate, inf * 0) and values beyond int land in a cell
__device__ __forceinline__ int np_axis_cell(float rel, float inv, int G) {
    return (int)fminf(fmaxf(floorf(rel * inv), 0.f), (float)(G - 1));
}
__device__ __forceinline__ int np_cell(const NpPlan& P, float x, float y, float z) {
    const int cx = np_axis_cell(x - P.lo[0], P.inv[0], P.G[0]);
    const int cy = np_axis_cell(y - P.lo[1], P.inv[1], P.G[1]);
    const int cz = np_axis_cell(z - P.lo[2], P.inv[2], P.G[2]);
    return (cz * P.G[1] + cy) * P.G[0] + cx;
}

__global__ __launch_bounds__(NP_T) void nearest_hist_kernel(int m, int wps, int cells, const float* __restrict__ xyz2, const NpPlan* __restrict__ hdr,
                                                            int* __restrict__ cnt, int2* __restrict__ slot) {
    const int scene = blockIdx.x / wps, w = blockIdx.x - scene * wps;
    const NpPlan P = hdr[scene];
    const float* sp = xyz2 + (size_t)scene * m * 3;
    int* c = cnt + (size_t)scene * cells;
    int2* r = slot + (size_t)scene * m;
    for (int k = w * NP_T + threadIdx.x; k < m; k += wps * NP_T) {
        const int cell = np_cell(P, sp[(size_t)k * 3], sp[(size_t)k * 3 + 1], sp[(size_t)k * 3 + 2]);
        r[k] = make_int2(cell, atomicAdd(&c[cell], 1));
    }
}

__global__ __launch_bounds__(NP_SCAN_T) void nearest_scan_kernel(int cells, const NpPlan* __restrict__ hdr, const int* __restrict__ cnt, int* __restrict__ start) {
    __shared__ int s_wsum[NP_SCAN_T / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int scene = blockIdx.x;
    const int ncell = hdr[scene].G[0] * hdr[scene].G[1] * hdr[scene].G[2];
    const int* c = cnt + (size_t)scene * cells;
    int* st = start + (size_t)scene * (cells + 1);
    const int per = (ncell + NP_SCAN_T - 1) / NP_SCAN_T;                     // consecutive cells per thread
    const int c0 = min(t * per, ncell), c1 = min(c0 + per, ncell);
    int local = 0;
    for (int i = c0; i < c1; ++i) local += c[i];
    int incl = local;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) { const int u = __shfl_up(incl, sft, 64); if (lane >= sft) incl += u; }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int run = incl - local;
    for (int w = 0; w < wave; ++w) run += s_wsum[w];
    for (int i = c0; i < c1; ++i) { st[i] = run; run += c[i]; }
    if (t == NP_SCAN_T - 1) st[ncell] = run;                                 // == m
}

__global__ __launch_bounds__(NP_T) void nearest_scatter_kernel(int m, int wps, int cells, const float* __restrict__ xyz2, const int* __restrict__ start,
                                                               const int2* __restrict__ slot, float4* __restrict__ pts) {
    const int scene = blockIdx.x / wps, w = blockIdx.x - scene * wps;
    const float* sp = xyz2 + (size_t)scene * m * 3;
    const int* st = start + (size_t)scene * (cells + 1);
    const int2* r = slot + (size_t)scene * m;
    float4* out = pts + (size_t)scene * m;
    for (int k = w * NP_T + threadIdx.x; k < m; k += wps * NP_T) {
        const int2 cr = r[k];
        out[st[cr.x] + cr.y] = make_float4(sp[(size_t)k * 3], sp[(size_t)k * 3 + 1], sp[(size_t)k * 3 + 2], __int_as_float(k));
    }
}

// the reference's strict '<' over ascending k leaves the smallest (d, k) pair; (+inf, 0) is below no pair whose d is +inf or NaN
__device__ __forceinline__ void np_take(float& b1, int& i1, float d, int k) {
    if (d < b1 || (d == b1 && k < i1)) { b1 = d; i1 = k; }
}

__global__ __launch_bounds__(NP_T) void nearest_query_kernel(int b, int n, int m, int cells, const float* __restrict__ xyz1, const float4* __restrict__ pts,
                                                             const NpPlan* __restrict__ hdr, const int* __restrict__ start, float* __restrict__ dist,
                                                             int* __restrict__ idx) {
    const int scene = blockIdx.x % b;                                        // scene <-> XCD affinity for the sorted points
    const int j = (blockIdx.x / b) * NP_T + threadIdx.x;
    if (j >= n) return;
    const size_t o = (size_t)scene * n + j;
    const float qx = xyz1[o * 3], qy = xyz1[o * 3 + 1], qz = xyz1[o * 3 + 2];
    // a non-finite query: every distance is +inf or NaN, nothing wins (tf_interpolate.cpp:66, :75)
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) { dist[o] = INFINITY; idx[o] = 0; return; }
    const NpPlan P = hdr[scene];
    const int* st = start + (size_t)scene * (cells + 1);
    const float4* sp = pts + (size_t)scene * m;
    const float qv[3] = {qx, qy, qz};
    float b1 = INFINITY;
    int i1 = 0;
    int c[3], c0[3], c1[3];
    float rel[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        rel[a] = qv[a] - P.lo[a];                                            // box-relative: the subtraction np_cell performs
        c[a] = np_axis_cell(rel[a], P.inv[a], P.G[a]);
        c0[a] = max(c[a] - 1, 0);
        c1[a] = min(c[a] + 1, P.G[a] - 1);
    }
    // distance to the nearest face of the block c0..c1 that has cells behind it; +inf when the block is all cells (a flat axis has one cell and no face)
    auto face_bound = [&]() -> float {
        float bound = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (c0[a] > 0) bound = fminf(bound, rel[a] - (float)c0[a] * P.h[a]);
            if (c1[a] < P.G[a] - 1) bound = fminf(bound, (float)(c1[a] + 1) * P.h[a] - rel[a]);
        }
        return bound;
    };
    // Shrunk distance along axis a from the query to the slab of cells cc, 0 for the query's own: a lower bound for every point sorted into
    // that slab (same shrink and eps as the accept test below).  Cells whose three gaps, squared, add up to more than b1 hold nothing that
    // can win or tie, and are not read: the query's own row goes first, and what it finds prunes most of the rest of the block.
    auto gap = [&](int a, int cc) -> float {
        if (cc == c[a]) return 0.f;
        const float g = cc > c[a] ? (float)cc * P.h[a] - rel[a] : rel[a] - (float)(cc + 1) * P.h[a];
        return fmaxf(g * 0.999f - P.eps, 0.f);
    };
    auto scan_row = [&](int cz, int cy, float gyz) {
        int x0 = c0[0], x1 = c1[0];
        for (; x0 < c[0]; ++x0) { const float g = gap(0, x0); if (!(g * g + gyz > b1)) break; }
        for (; x1 > c[0]; --x1) { const float g = gap(0, x1); if (!(g * g + gyz > b1)) break; }
        const int row = (cz * P.G[1] + cy) * P.G[0];
        const int e1 = st[row + x1 + 1];
        int e = st[row + x0];
        for (; e + 3 < e1; e += 4) {                                         // four candidates in flight
            const float4 p0 = sp[e], p1 = sp[e + 1], p2 = sp[e + 2], p3 = sp[e + 3];
            const float d0 = dist2_host(p0.x - qx, p0.y - qy, p0.z - qz), d1 = dist2_host(p1.x - qx, p1.y - qy, p1.z - qz);     // :71-74, the reference's expression
            const float d2 = dist2_host(p2.x - qx, p2.y - qy, p2.z - qz), d3 = dist2_host(p3.x - qx, p3.y - qy, p3.z - qz);
            if (fminf(fminf(d0, d1), fminf(d2, d3)) <= b1) {
                np_take(b1, i1, d0, __float_as_int(p0.w)); np_take(b1, i1, d1, __float_as_int(p1.w));
                np_take(b1, i1, d2, __float_as_int(p2.w)); np_take(b1, i1, d3, __float_as_int(p3.w));
            }
        }
        for (; e < e1; ++e) {
            const float4 p = sp[e];
            np_take(b1, i1, dist2_host(p.x - qx, p.y - qy, p.z - qz), __float_as_int(p.w));
        }
    };
    auto scan_block = [&]() {                                                // rows c0..c1 of y and z; the own row is inside every such range
        scan_row(c[2], c[1], 0.f);
        for (int cz = c0[2]; cz <= c1[2]; ++cz) {
            const float gz = gap(2, cz);
            for (int cy = c0[1]; cy <= c1[1]; ++cy) {
                if (cz == c[2] && cy == c[1]) continue;
                const float gy = gap(1, cy);
                const float gyz = gy * gy + gz * gz;
                if (!(gyz > b1)) scan_row(cz, cy, gyz);
            }
        }
    };
    for (int reach = 1;; reach *= 2) {
        scan_block();
        // accepted iff no point outside the block can be as close as the one found: along the axis of the face it lies behind it is at least
        // `bound` away (cells are assigned with the same lo / inv, one rounding: the 1e-3 shrink covers it many times over; eps covers a
        // point that this rounding put across a face the query all but touches, where a shrink relative to `bound` covers nothing)
        const float bound = face_bound();
        const float safe = bound * 0.999f - P.eps;
        if (safe > 0.f && b1 < safe * safe) break;
        if (!(bound < INFINITY)) break;                                      // that was every cell: nothing finite anywhere
        if (b1 < INFINITY) {
            // go on over every cell the ball of radius sqrt(b1) touches; the nearest point lies inside it.  What was found stays: it is
            // a pair of the known set, and taking a pair twice changes nothing.
            // The ball holds the answer as long as a point beyond the cell of slack is strictly farther than b1 IN FP32: true of a normal
            // b1 (r * r > b1), and of a subnormal or zero one only while a shrunk cell edge, squared, still exceeds it (b1 = 0 at any
            // ordinary scale: a query on a known point).  Where the squared distances of a tiny cloud all underflow to one value the
            // lowest index wins from anywhere: every cell.
            const float r = sqrtf(b1) * 1.001f;
            float hs = INFINITY;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (P.inv[a] > 0.f) hs = fminf(hs, P.h[a] * 0.999f - P.eps);
            const bool ball = b1 >= GSPN_FLT_MIN || (hs > 0.f && hs * hs > b1);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!ball) { c0[a] = 0; c1[a] = P.G[a] - 1; }
                else if (P.inv[a] > 0.f) {
                    c0[a] = min(max(np_axis_cell(rel[a] - r, P.inv[a], P.G[a]) - 1, 0), c[a]);        // (one cell of slack on both sides)
                    c1[a] = max(min(np_axis_cell(rel[a] + r, P.inv[a], P.G[a]) + 1, P.G[a] - 1), c[a]);
                }
            }
            scan_block();
            break;
        }
        // an empty block (a query in a hollow of the cloud, or far outside its box): twice the reach, until something is found or every cell was read
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c0[a] = max(c[a] - 2 * reach, 0);
            c1[a] = min(c[a] + 2 * reach, P.G[a] - 1);
        }
    }
    dist[o] = b1;
    idx[o] = i1;
}

extern "C" long gspn_nearest_point_ws_bytes(int b, int m) {
    if (b < 1 || m < 1 || m > GSPN_NEAREST_MAX_M) return 0;
    return (long)np_layout(b, m).bytes;
}

extern "C" int gspn_nearest_point(int b, int n, int m, const float* xyz1, const float* xyz2, void* ws, float* dist, int* idx, void* stream) {
    if (b < 0 || n < 0 || m < 0) return GSPN_ERR_ARG;
    if (b == 0 || n == 0) return 0;
    if (m == 0 || !xyz1 || !xyz2 || !ws || !dist || !idx) return GSPN_ERR_ARG;
    if (m > GSPN_NEAREST_MAX_M) return GSPN_ERR_UNSUPPORTED;
    const int wps = np_build_wps(m);
    const long long qblocks = (long long)b * ((n + NP_T - 1) / NP_T), bblocks = (long long)b * wps;
    if (qblocks > 0x7FFFFFFFll || bblocks > 0x7FFFFFFFll || (reinterpret_cast<uintptr_t>(ws) & 15) != 0) return GSPN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const NpLayout l = np_layout(b, m);
    char* base = static_cast<char*>(ws);
    float4* pts = reinterpret_cast<float4*>(base + l.pts);
    NpPlan* hdr = reinterpret_cast<NpPlan*>(base + l.hdr);
    int* cnt = reinterpret_cast<int*>(base + l.cnt);
    int* start = reinterpret_cast<int*>(base + l.start);
    int2* slot = reinterpret_cast<int2*>(base + l.slot);
    const long ncnt = (long)b * l.cells;                                     // >= b
    hipLaunchKernelGGL(nearest_init_kernel, dim3(grid_for(ncnt, NP_T)), dim3(NP_T), 0, st, b, ncnt, hdr, cnt);
    hipLaunchKernelGGL(nearest_bbox_kernel, dim3((unsigned)bblocks), dim3(NP_T), 0, st, m, wps, xyz2, hdr);
    hipLaunchKernelGGL(nearest_plan_kernel, dim3((unsigned)((b + 63) / 64)), dim3(64), 0, st, b, l.cells, hdr);
    hipLaunchKernelGGL(nearest_hist_kernel, dim3((unsigned)bblocks), dim3(NP_T), 0, st, m, wps, l.cells, xyz2, hdr, cnt, slot);
    hipLaunchKernelGGL(nearest_scan_kernel, dim3((unsigned)b), dim3(NP_SCAN_T), 0, st, l.cells, hdr, cnt, start);
    hipLaunchKernelGGL(nearest_scatter_kernel, dim3((unsigned)bblocks), dim3(NP_T), 0, st, m, wps, l.cells, xyz2, start, slot, pts);
    hipLaunchKernelGGL(nearest_query_kernel, dim3((unsigned)qblocks), dim3(NP_T), 0, st, b, n, m, l.cells, xyz1, pts, hdr, start, dist, idx);
    return gspn_launch_status();
}
