// components.hip -- mask components (additive at ABI 21): the connected components of every mask row on the scan's mesh, and
// the rows with their small components dropped.  r mask rows of v bytes (any nonzero byte set), f triangles; the components of row k are
// those of its set vertices under the mesh edges whose two ends are both set in row k; comp[k][x] = the smallest vertex of x's component.
//
// Lock-free union-find, the parent array being comp itself.  INVARIANT: parent[x] <= x, with equality at a root alone.  Every write keeps
// it -- init writes x, the hook writes a smaller root over a root, halving, compress and flatten write over a NON-root a vertex of its own
// tree that was its ancestor when read, which is smaller; a root is only ever written by the compare-and-swap --, so every walk strictly
// descends, there is no cycle, no tree is ever split, and the root of a tree is its minimum.  A read may be STALE (a CU's L1 and an XCD's
// L2 are not refreshed by another's writes): a stale parent is an earlier parent, that is x itself or a vertex of x's tree below x, so a
// walk over stale values still descends inside x's component and ends on a vertex that WAS a root; the compare-and-swap, which executes
// at the memory side, is what decides, and it fails on a vertex that no longer is one.
//
//   init     grid (chunks of 16 bytes / 256, r) over the ADDRESS of the row (the walk of mask_rows.h), one chunk per lane;
//            parent[k][x] = set ? x : -1, size[k][x] = 0, written 64 consecutive vertices per wave and pass (the lanes trade their 16 bits
//            by shuffles), and the row's counters zeroed
//   table    grid (v / 256, words): the VERTEX-MAJOR bit table, words = ceil(r / 64) 64-bit words per vertex, bit k = set in row k, read
//            from parent (coalesced dwords) so that rows need no alignment
//   hook     one lane per face, grid-stride: the face is read ONCE, not r times; each of its three edges ANDs its ends' words and does one
//            union per common bit: find both roots, atomicCAS the larger root's parent from itself to the smaller, on failure go on from
//            the returned value.  find halves the path (a vertex passed over takes its grandparent)
//   compress one lane per (row, vertex): a set vertex walks to its root, halving, and takes what it found, in place.  Another lane's late
//            halving store may put an ancestor back over that value, so this pass only SHORTENS the trees: they end two or three deep
//   flatten  one lane per (row, vertex): a set vertex walks to its root WITHOUT writing on the way and takes it: the only stores of this
//            pass are roots, so what it leaves is final.  The lanes of a wave that share a root add their number to size[k][root] with
//            one integer atomicAdd
//   stats    one lane per (row, vertex), roots alone (comp == x): ncomp += 1, largest = max(size), one atomic of each per wave
//   finish   (components) / apply (filter): ncomp[k] = -1 for a row in which a loop reached its bound
//   apply    grid over the ADDRESS of out's row (mask_rows.h), one chunk written per lane, comp read 64 consecutive vertices per wave and pass
//            and the decisions traded by ballots: out = the component of the vertex is kept,
//            size >= min_vertices and (double)size >= min_share * (double)largest; nkept and mask_points summed over the kept roots.  It
//            reads comp and size and never masks, so out may be masks
//
// TERMINATION: a walk from x visits x > x1 > x2 > ... >= 0, at most v vertices; a failed compare-and-swap on hi returns a parent below hi,
// the next attempt's larger root lies below that, so the attempts of one union have strictly descending targets, at most v.  Both loops
// carry the bound v all the same, and every value read as an index is range-checked: a loop that reaches its bound or reads a value
// outside [0, v) stops and marks the row (ncomp = -1), which a correct build never does.  No grid-wide wait, no cooperative launch, no host
// read.  Integer atomics only: sizes are counts, so the bits do not depend on the order of the atomics.  Row offsets are 64-bit.  Nothing
// is read from ws that the call did not write.
#include "common.h"
#include "components_args.h"
#include "mask_rows.h"

#define MC_T 256

typedef unsigned long long u64;

namespace {

// past the L1, which nobody refreshes; what the L2 holds may still be stale (see above)
__device__ __forceinline__ int mc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mc_store(int* p, int x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the root of x in the row's parent array p, halving the path on the way; -1 when a value outside [0, v) turns up or after v steps
__device__ __forceinline__ int mc_find(int* p, int x, int v) {
    if ((unsigned)x >= (unsigned)v) return -1;
    int prev = x, cur = mc_load(p + x);
    if (cur == x) return x;
    for (int n = 0; n < v; ++n) {                                    // cur descends strictly: fewer than v rounds
        if ((unsigned)cur >= (unsigned)prev) return -1;              // the invariant, and cur >= 0
        const int next = mc_load(p + cur);
        if (next == cur) return cur;
        mc_store(p + prev, next);                                    // an ancestor of prev below it (checked in the next round, before it is used)
        prev = cur;
        cur = next;
    }
    return -1;
}

__device__ __forceinline__ bool mc_union(int* p, int a, int b, int v) {
    for (int n = 0; n < v; ++n) {                                    // the targets descend strictly: fewer than v failures
        a = mc_find(p, a, v);
        b = mc_find(p, b, v);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(p + hi, hi, lo);
        if (old == hi) return true;
        if ((unsigned)old >= (unsigned)hi) return false;             // hi was hooked meanwhile: its parent is below it
        a = old;
        b = lo;
    }
    return false;
}

// grid (ceil(chunks / MC_T), r) over the address of the row
__global__ __launch_bounds__(MC_T) void mc_init_kernel(int v, const unsigned char* masks, int* __restrict__ parent, int* __restrict__ size,
                                                       int* __restrict__ bad, int* __restrict__ ncomp, int* __restrict__ largest,
                                                       int* __restrict__ nkept, int* __restrict__ mask_points) {
    const int row = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        bad[row] = 0;
        ncomp[row] = 0;
        largest[row] = 0;
        if (nkept) {
            nkept[row] = 0;
            mask_points[row] = 0;
        }
    }
    const unsigned char* p = masks + (long)row * v;
    const int i0 = (blockIdx.x * MC_T + threadIdx.x) * MASK_ROW_VEC - mask_row_a0(p);    // >= -15; < 2^24 + 16 * MC_T
    const unsigned bits = mask_row_load(p, i0, v);                   // (nobody returns: the lanes trade their bits below)
    // The wave's 64 chunks are 1024 consecutive vertices.  A lane that wrote its own 16 would put 64 bytes between one lane's dword and
    // the next (454 us at 100 x 500 000, measured); in pass t the wave writes the 64 consecutive vertices 64 t .. 64 t + 63 instead, lane l
    // taking bit l % 16 of the chunk of lane 4 t + l / 16.
    const int lane = lane_id();
    const int first = i0 - lane * MASK_ROW_VEC;                      // the first vertex of the wave's chunks, >= -15
    int* par = parent + (long)row * v;
    int* sz = size + (long)row * v;
#pragma unroll
    for (int t = 0; t < MASK_ROW_VEC; ++t) {
        const unsigned theirs = (unsigned)__shfl((int)bits, 4 * t + (lane >> 4), GSPN_WAVE);
        const int i = first + GSPN_WAVE * t + lane;
        if (i >= 0 && i < v) {
            par[i] = (theirs >> (lane & 15)) & 1u ? i : -1;
            sz[i] = 0;
        }
    }
}

// grid (ceil(v / MC_T), words)
__global__ __launch_bounds__(MC_T) void mc_table_kernel(int r, int v, int words, const int* __restrict__ parent, u64* __restrict__ table) {
    const int x = blockIdx.x * MC_T + threadIdx.x;
    if (x >= v) return;
    const int k0 = blockIdx.y * 64, k1 = min(r, k0 + 64);
    u64 word = 0ull;
    for (int k = k0; k < k1; ++k)
        if (parent[(long)k * v + x] >= 0) word |= 1ull << (k - k0);
    table[(long)x * words + blockIdx.y] = word;
}

// grid-stride over the faces.  parent is read and written by every lane: no __restrict__
__global__ __launch_bounds__(MC_T) void mc_hook_kernel(int v, int f, int words, const int* __restrict__ faces, const u64* __restrict__ table,
                                                       int* parent, int* __restrict__ bad) {
    for (long t = blockIdx.x * (long)MC_T + threadIdx.x; t < f; t += (long)gridDim.x * MC_T) {
        const int a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
        const int eu[3] = {a, b, a}, ew[3] = {b, c, c};
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int u = eu[e], w = ew[e];
            if ((unsigned)u >= (unsigned)v || (unsigned)w >= (unsigned)v || u == w) continue;        // an end outside [0, v): no edge
            for (int j = 0; j < words; ++j) {
                u64 m = table[(long)u * words + j] & table[(long)w * words + j];
                while (m != 0ull) {
                    const int k = j * 64 + __ffsll((long long)m) - 1;                                 // < r: the table has no bit beyond
                    m &= m - 1ull;
                    if (!mc_union(parent + (long)k * v, u, w, v)) bad[k] = 1;
                }
            }
        }
    }
}

// grid (ceil(v / MC_T), r)
__global__ __launch_bounds__(MC_T) void mc_compress_kernel(int v, int* parent, int* __restrict__ bad) {
    const int row = blockIdx.y, x = blockIdx.x * MC_T + threadIdx.x;
    int* par = parent + (long)row * v;
    if (x >= v || mc_load(par + x) < 0) return;
    const int root = mc_find(par, x, v);
    if (root >= 0) mc_store(par + x, root);
    else bad[row] = 1;
}

// grid (ceil(v / MC_T), r)
__global__ __launch_bounds__(MC_T) void mc_flatten_kernel(int v, int* parent, int* __restrict__ size, int* __restrict__ bad) {
    const int row = blockIdx.y, x = blockIdx.x * MC_T + threadIdx.x;
    int* par = parent + (long)row * v;
    int root = -1;
    if (x < v && mc_load(par + x) >= 0) {
        int cur = x;
        for (int n = 0; n < v; ++n) {                                // reads alone: cur descends strictly, fewer than v rounds
            const int next = mc_load(par + cur);
            if (next == cur) {
                root = cur;
                break;
            }
            if ((unsigned)next >= (unsigned)cur) break;              // the invariant, and next >= 0
            cur = next;
        }
        if (root >= 0) mc_store(par + x, root);                      // a root: the only kind of value this pass stores
        else bad[row] = 1;
    }
    // the lanes of the wave that share a root add their number once (every lane of the wave is here: nobody returned)
    const int lane = lane_id();
    int* sz = size + (long)row * v;
    u64 todo = __ballot(root >= 0);
    while (todo != 0ull) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lr = __shfl(root, leader, GSPN_WAVE);
        const u64 same = __ballot(root == lr);
        if (lane == leader) atomicAdd(&sz[lr], __popcll(same));
        todo &= ~same;
    }
}

// grid (ceil(v / MC_T), r): the roots alone
__global__ __launch_bounds__(MC_T) void mc_stats_kernel(int v, const int* __restrict__ comp, const int* __restrict__ size, int* __restrict__ ncomp,
                                                        int* __restrict__ largest) {
    const int row = blockIdx.y, x = blockIdx.x * MC_T + threadIdx.x;
    const bool root = x < v && comp[(long)row * v + x] == x;
    const int s = root ? size[(long)row * v + x] : 0;
    const u64 roots = __ballot(root);
    if (roots == 0ull) return;                                       // uniform over the wave
    const int big = wave_max_i32(s);
    if (lane_id() == 0) {
        atomicAdd(&ncomp[row], __popcll(roots));
        atomicMax(&largest[row], big);
    }
}

// grid (ceil(r / MC_T))
__global__ __launch_bounds__(MC_T) void mc_finish_kernel(int r, const int* __restrict__ bad, int* __restrict__ ncomp) {
    const int row = blockIdx.x * MC_T + threadIdx.x;
    if (row < r && bad[row] != 0) ncomp[row] = -1;
}

// grid (ceil(chunks / MC_T), r) over the ADDRESS of out's row
__global__ __launch_bounds__(MC_T) void mc_apply_kernel(int v, int min_vertices, double min_share, const int* __restrict__ comp,
                                                        const int* __restrict__ size, const int* __restrict__ largest, const int* __restrict__ bad,
                                                        unsigned char* out, int* __restrict__ mask_points, int* __restrict__ ncomp,
                                                        int* __restrict__ nkept) {
    const int row = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0 && bad[row] != 0) ncomp[row] = -1;      // the stats pass is over: nobody adds to it any more
    unsigned char* p = out + (long)row * v;
    const int i0 = (blockIdx.x * MC_T + threadIdx.x) * MASK_ROW_VEC - mask_row_a0(p);    // >= -15; < 2^24 + 16 * MC_T
    const int* c = comp + (long)row * v;
    const int* sz = size + (long)row * v;
    const double floor_share = min_share * (double)largest[row];
    // As in init, the wave's 64 chunks are 1024 consecutive vertices: in pass t lane l decides vertex 64 t + l of them (one coalesced read of
    // comp; a lane that read its own 16 took 135 us at 100 x 500 000, measured), the ballot of the pass holds the bits of four chunks, and
    // the lane whose chunk is among them keeps its 16.
    const int lane = lane_id();
    const int first = i0 - lane * MASK_ROW_VEC;                      // the first vertex of the wave's chunks, >= -15
    unsigned bits = 0u;
    int kept_roots = 0, kept_points = 0;
#pragma unroll
    for (int t = 0; t < MASK_ROW_VEC; ++t) {
        const int i = first + GSPN_WAVE * t + lane;
        bool on = false;
        if (i >= 0 && i < v) {
            const int root = c[i];
            if ((unsigned)root < (unsigned)v) {                      // -1: not set
                const int s = sz[root];
                on = s >= min_vertices && (double)s >= floor_share;
                if (on && root == i) {                               // summed over the roots, never per vertex
                    ++kept_roots;
                    kept_points += s;
                }
            }
        }
        const u64 word = __ballot(on);
        if ((lane >> 2) == t) bits = (unsigned)(word >> (16 * (lane & 3))) & 0xFFFFu;
    }
    mask_row_store(p, i0, v, bits);
    kept_roots = wave_sum_lane0(kept_roots);
    kept_points = wave_sum_lane0(kept_points);                       // <= v <= 2^24
    if (lane_id() == 0 && kept_roots != 0) {
        atomicAdd(&nkept[row], kept_roots);
        atomicAdd(&mask_points[row], kept_points);
    }
}

// init .. stats: comp (= parent), ncomp and largest of every row
void mc_label(hipStream_t st, int r, int v, int f, const McLayout& l, const unsigned char* masks, const int* faces, char* base, int* comp,
              int* ncomp, int* largest, int* nkept, int* mask_points) {
    u64* table = reinterpret_cast<u64*>(base + l.table);
    int* size = reinterpret_cast<int*>(base + l.size);
    int* bad = reinterpret_cast<int*>(base + l.bad);
    const dim3 by_vector((unsigned)((mask_row_chunks(v) + MC_T - 1) / MC_T), (unsigned)r), by_vertex((unsigned)((v + MC_T - 1) / MC_T), (unsigned)r);
    hipLaunchKernelGGL(mc_init_kernel, by_vector, dim3(MC_T), 0, st, v, masks, comp, size, bad, ncomp, largest, nkept, mask_points);
    if (f > 0) {
        hipLaunchKernelGGL(mc_table_kernel, dim3(by_vertex.x, (unsigned)l.words), dim3(MC_T), 0, st, r, v, l.words, comp, table);
        hipLaunchKernelGGL(mc_hook_kernel, dim3(grid_for(f, MC_T)), dim3(MC_T), 0, st, v, f, l.words, faces, table, comp, bad);
    }
    if (f > 0) hipLaunchKernelGGL(mc_compress_kernel, by_vertex, dim3(MC_T), 0, st, v, comp, bad);       // without faces every vertex is a root
    hipLaunchKernelGGL(mc_flatten_kernel, by_vertex, dim3(MC_T), 0, st, v, comp, size, bad);
    hipLaunchKernelGGL(mc_stats_kernel, by_vertex, dim3(MC_T), 0, st, v, comp, size, ncomp, largest);
}

}  // namespace

extern "C" long gspn_mask_components_ws_bytes(int r, int v, int f) { return mc_ws_bytes(r, v, f); }

extern "C" int gspn_mask_components(int r, int v, int f, const unsigned char* masks, const int* faces, void* ws, int* comp, int* ncomp,
                                    int* largest, void* stream) {
    const int rc = mc_check(r, v, f, masks, faces, ws, comp, ncomp, largest);
    if (rc != 0) return rc;
    if (r == 0 || v == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const McLayout l = mc_layout(r, v, false);
    char* base = static_cast<char*>(ws);
    mc_label(st, r, v, f, l, masks, faces, base, comp, ncomp, largest, nullptr, nullptr);
    hipLaunchKernelGGL(mc_finish_kernel, dim3((unsigned)((r + MC_T - 1) / MC_T)), dim3(MC_T), 0, st, r, reinterpret_cast<int*>(base + l.bad), ncomp);
    return gspn_launch_status();
}

extern "C" long gspn_mask_component_filter_ws_bytes(int r, int v, int f) { return mf_ws_bytes(r, v, f); }

extern "C" int gspn_mask_component_filter(int r, int v, int f, const unsigned char* masks, const int* faces, int min_vertices, double min_share,
                                          void* ws, unsigned char* out, int* mask_points, int* ncomp, int* nkept, void* stream) {
    const int rc = mf_check(r, v, f, masks, faces, min_vertices, min_share, ws, out, mask_points, ncomp, nkept);
    if (rc != 0) return rc;
    if (r == 0 || v == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const McLayout l = mc_layout(r, v, true);
    char* base = static_cast<char*>(ws);
    int* comp = reinterpret_cast<int*>(base + l.parent);
    int* largest = reinterpret_cast<int*>(base + l.largest);
    mc_label(st, r, v, f, l, masks, faces, base, comp, ncomp, largest, nkept, mask_points);
    hipLaunchKernelGGL(mc_apply_kernel, dim3((unsigned)((mask_row_chunks(v) + MC_T - 1) / MC_T), (unsigned)r), dim3(MC_T), 0, st, v, min_vertices, min_share,
                       comp, reinterpret_cast<int*>(base + l.size), largest, reinterpret_cast<int*>(base + l.bad), out, mask_points, ncomp, nkept);
    return gspn_launch_status();
}
