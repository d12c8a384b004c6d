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
//   init     grid (chunks of 16 bytes / 256, r) over the ADDRESS of the row, one chunk per lane (the address walk and the wave walk of
//            mask_rows.h): parent[k][x] = set ? x : -1, size[k][x] = 0, and the row's counters zeroed
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
//   apply    grid over the ADDRESS of out's row, one chunk written per lane (both walks of mask_rows.h): out = the component of the vertex
//            is kept, size >= min_vertices and (double)size >= min_share * (double)largest; nkept and mask_points summed over the kept
//            roots.  It reads comp and size and never masks, so out may be masks
//
// TERMINATION: a walk from x visits x > x1 > x2 > ... >= 0, at most v vertices; a failed compare-and-swap on hi returns a parent below hi,
// the next attempt's larger root lies below that, so the attempts of one union have strictly descending targets, at most v.  Both loops
// carry the bound v all the same, and every value read as an index is range-checked: a loop that reaches its bound or reads a value
// outside [0, v) stops and marks the row (ncomp = -1), which a correct build never does.  No grid-wide wait, no cooperative launch, no host
// read.  Integer atomics only: sizes are counts, so the bits do not depend on the order of the atomics.  Row offsets are 64-bit.  Nothing
// is read from ws that the call did not write.
#include "common.h"
#include "components_args.h"
#include "float_keys.h"
#include "holes_args.h"
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
    const unsigned bits = mask_row_load(p, i0, v);                   // (nobody returns: the wave walk needs every lane)
    int* par = parent + (long)row * v;
    int* sz = size + (long)row * v;
    mask_wave_read(bits, i0, v, [&](int i, bool set) {
        par[i] = set ? i : -1;
        sz[i] = 0;
    });
}

// grid (ceil(v / MC_T), words): table bit k = parent[k][x] >= 0 and, with SETS (the holes), set bit k = parent[k][x] == -2, in one read
template <bool SETS>
__global__ __launch_bounds__(MC_T) void mc_table_kernel(int r, int v, int words, const int* __restrict__ parent, u64* __restrict__ table,
                                                        u64* __restrict__ set) {
    const int x = blockIdx.x * MC_T + threadIdx.x;
    if (x >= v) return;
    const int k0 = blockIdx.y * 64, k1 = min(r, k0 + 64);
    u64 c = 0ull, s = 0ull;
    for (int k = k0; k < k1; ++k) {
        const int p = parent[(long)k * v + x];
        if (p >= 0) c |= 1ull << (k - k0);
        if (SETS && p == -2) s |= 1ull << (k - k0);
    }
    table[(long)x * words + blockIdx.y] = c;
    if (SETS) set[(long)x * words + blockIdx.y] = s;
}

// Face t, read once.  edge(e, v, u, w) -> the ends of edge e of {a,b}, {b,c}, {a,c}; false where one lies outside [0, v) or u == w: no edge
struct McFace {
    int a, b, c;
    __device__ __forceinline__ McFace(const int* __restrict__ faces, long t) : a(faces[3 * t]), b(faces[3 * t + 1]), c(faces[3 * t + 2]) {}
    __device__ __forceinline__ bool edge(int e, int v, int& u, int& w) const {
        const int eu[3] = {a, b, a}, ew[3] = {b, c, c};
        u = eu[e];
        w = ew[e];
        return (unsigned)u < (unsigned)v && (unsigned)w < (unsigned)v && u != w;
    }
};

// grid-stride over the faces.  parent is read and written by every lane: no __restrict__
__global__ __launch_bounds__(MC_T) void mc_hook_kernel(int v, int f, int words, const int* __restrict__ faces, const u64* __restrict__ table,
                                                       int* parent, int* __restrict__ bad) {
    for (long t = blockIdx.x * (long)MC_T + threadIdx.x; t < f; t += (long)gridDim.x * MC_T) {
        const McFace face(faces, t);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            int u, w;
            if (!face.edge(e, v, u, w)) continue;
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
    unsigned bits = 0u;
    int kept_roots = 0, kept_points = 0;
#pragma unroll
    for (int t = 0; t < MASK_ROW_VEC; ++t) {
        const int i = mask_wave_vertex(i0, t);
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
        mask_wave_write(on, t, bits);
    }
    mask_row_store(p, i0, v, bits);
    kept_roots = wave_sum_lane0(kept_roots);
    kept_points = wave_sum_lane0(kept_points);                       // <= v <= 2^24
    if (lane_id() == 0 && kept_roots != 0) {
        atomicAdd(&nkept[row], kept_roots);
        atomicAdd(&mask_points[row], kept_points);
    }
}

// the two grid shapes of the per-row kernels: one chunk of the address walk per lane, and one vertex per lane
dim3 mc_by_vector(int r, int v) { return dim3((unsigned)((mask_row_chunks(v) + MC_T - 1) / MC_T), (unsigned)r); }
dim3 mc_by_vertex(int r, int v) { return dim3((unsigned)((v + MC_T - 1) / MC_T), (unsigned)r); }

// table, hook, compress over f > 0 faces: the trees of parent joined along the edges; set is the holes' second table, or null
void mc_join(hipStream_t st, int r, int v, int f, int words, const int* faces, int* parent, u64* table, u64* set, int* bad) {
    const dim3 by_word(mc_by_vertex(r, v).x, (unsigned)words);
    if (set) hipLaunchKernelGGL(mc_table_kernel<true>, by_word, dim3(MC_T), 0, st, r, v, words, parent, table, set);
    else hipLaunchKernelGGL(mc_table_kernel<false>, by_word, dim3(MC_T), 0, st, r, v, words, parent, table, set);
    hipLaunchKernelGGL(mc_hook_kernel, dim3(grid_for(f, MC_T)), dim3(MC_T), 0, st, v, f, words, faces, table, parent, bad);
    hipLaunchKernelGGL(mc_compress_kernel, mc_by_vertex(r, v), dim3(MC_T), 0, st, v, parent, bad);
}

// init .. stats: comp (= parent), ncomp and largest of every row
void mc_label(hipStream_t st, int r, int v, int f, const McLayout& l, const unsigned char* masks, const int* faces, char* base, int* comp,
              int* ncomp, int* largest, int* nkept, int* mask_points) {
    int* size = reinterpret_cast<int*>(base + l.size);
    int* bad = reinterpret_cast<int*>(base + l.bad);
    hipLaunchKernelGGL(mc_init_kernel, mc_by_vector(r, v), dim3(MC_T), 0, st, v, masks, comp, size, bad, ncomp, largest, nkept, mask_points);
    if (f > 0) mc_join(st, r, v, f, l.words, faces, comp, reinterpret_cast<u64*>(base + l.table), nullptr, bad);      // without faces every vertex is a root
    hipLaunchKernelGGL(mc_flatten_kernel, mc_by_vertex(r, v), dim3(MC_T), 0, st, v, comp, size, bad);
    hipLaunchKernelGGL(mc_stats_kernel, mc_by_vertex(r, v), dim3(MC_T), 0, st, v, comp, size, ncomp, largest);
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
    hipLaunchKernelGGL(mc_apply_kernel, mc_by_vector(r, v), dim3(MC_T), 0, st, v, min_vertices, min_share, comp, reinterpret_cast<int*>(base + l.size),
                       largest, reinterpret_cast<int*>(base + l.bad), out, mask_points, ncomp, nkept);
    return gspn_launch_status();
}

// ---------------- mask holes (additive at ABI 21): the gaps a mask row encloses on the mesh are filled ----------------------
//
// The mirror of the filter.  The graph of row k is its CANDIDATES, the unset vertices inside the closed box of its set vertices with finite
// coordinates, under the edges whose two ends are both candidates; a candidate component is a HOLE iff no edge joins it to an unset vertex
// outside the box (it is not OPEN), some edge joins it to a set vertex (it TOUCHES), and its size is within max_vertices and
// max_share * points_in.  The union-find above runs unchanged on a parent array that holds -2 at a set vertex, -1 at an unset vertex that
// is no candidate, and x at a candidate: every mc_* kernel treats a negative parent as "not in the graph".
//
//   prime    grid (r / 256): the box keys to (INT_MAX, INT_MIN), which decode to NaN; the row's counters and marks zeroed
//   box      grid over the ADDRESS of the row (mask_rows.h): the set vertices counted (points_in), lo and hi of those whose three coordinates
//            are finite reduced per wave and landed with integer atomicMin / atomicMax on the keys of float_keys.h
//   init     grid over the address of the row: parent = set ? -2 : (inside ? x : -1), size = 0; inside is lo <= c && c <= hi on the three
//            axes as float compares, so a NaN coordinate, and every vertex of a row without a box, is outside
//   table    grid (v / 256, words): mc_table_kernel<true>, both vertex-major tables in one read of parent, cand (parent >= 0) and set (parent == -2)
//   hook, compress, flatten   the kernels above on the cand table: parent[k][x] = the root, size[k][root] = the component's vertices
//   mark     one face per lane, grid ceil(f / 256): per edge and word, cand[u] & set[w] are the rows in which u's component touches,
//            cand[u] & ~cand[w] & ~set[w] those in which it is open, and the same with the ends swapped; per bit one integer atomicOr of
//            the flag into size[k][parent[k][u]], skipped where a read past the L1 shows it set already
//   apply    grid over the ADDRESS of out's row: out = set or in a hole; nholes, nfilled and mask_points summed over the hole roots, one
//            atomic of each per wave.  It reads parent, size and points_in and never masks, so out may be masks
//
// STALE READS: mark runs in a later kernel than every union and than flatten, whose only stores are roots; a kernel boundary makes them
// visible, so parent[k][u] is the final root and no walk is needed.  The flags are ORed by integer atomics into words nobody else writes
// in that kernel; the early-out read may miss a flag another lane has just set, which costs one more atomicOr of the same bit.  No loop
// but the table words and their bits; every index read from memory (a face's vertex, a root) is range-checked; a root outside [0, v) marks
// the row, whose nholes comes back -1.
#define HF_TOUCH (1 << 30)
#define HF_OPEN (1 << 29)
#define HF_COUNT (HF_OPEN - 1)           // sizes are at most 2^24

namespace {

// grid (ceil(r / MC_T))
__global__ __launch_bounds__(MC_T) void hf_prime_kernel(int r, int* __restrict__ box, int* __restrict__ points_in, int* __restrict__ bad,
                                                        int* __restrict__ mask_points, int* __restrict__ nholes, int* __restrict__ nfilled) {
    const int row = blockIdx.x * MC_T + threadIdx.x;
    if (row >= r) return;
    for (int a = 0; a < 3; ++a) {
        box[6 * row + a] = 0x7FFFFFFF;
        box[6 * row + 3 + a] = -0x7FFFFFFF - 1;
    }
    points_in[row] = 0;
    bad[row] = 0;
    mask_points[row] = 0;
    nholes[row] = 0;
    nfilled[row] = 0;
}

// grid (ceil(chunks / MC_T), r) over the address of the row
__global__ __launch_bounds__(MC_T) void hf_box_kernel(int v, const unsigned char* masks, const float* __restrict__ xyz, int* __restrict__ box,
                                                      int* __restrict__ points_in) {
    const int row = blockIdx.y;
    const unsigned char* p = masks + (long)row * v;
    const int i0 = (blockIdx.x * MC_T + threadIdx.x) * MASK_ROW_VEC - mask_row_a0(p);    // >= -15; < 2^24 + 16 * MC_T
    const unsigned bits = mask_row_load(p, i0, v);                   // (nobody returns: the wave walk needs every lane)
    if (__ballot(bits != 0u) == 0ull) return;                        // uniform over the wave: nothing set in its 1024 vertices
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int count = 0;
    mask_wave_read(bits, i0, v, [&](int i, bool set) {
        if (!set) return;
        ++count;
        const float c[3] = {xyz[3l * i], xyz[3l * i + 1], xyz[3l * i + 2]};
        if (fabsf(c[0]) < INFINITY && fabsf(c[1]) < INFINITY && fabsf(c[2]) < INFINITY) {             // a NaN fails the compare
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(lo[a], c[a]);
                hi[a] = fmaxf(hi[a], c[a]);
            }
        }
    });
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = wave_min_f32(lo[a]);
        hi[a] = wave_max_f32(hi[a]);
    }
    count = wave_sum_lane0(count);
    if (lane_id() == 0) {
        atomicAdd(&points_in[row], count);
        if (lo[0] <= hi[0]) {                                        // the wave saw a finite vertex: all three axes have one
            // (Reading the six keys first, past the L1, and landing only what would change them was measured and is slower: the wave then
            // waits for the reads, while an atomic whose value nobody uses does not hold it.)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(&box[6 * row + a], np_key(lo[a]));
                atomicMax(&box[6 * row + 3 + a], np_key(hi[a]));
            }
        }
    }
}

// grid (ceil(chunks / MC_T), r) over the address of the row
__global__ __launch_bounds__(MC_T) void hf_init_kernel(int v, const unsigned char* masks, const float* __restrict__ xyz, const int* __restrict__ box,
                                                       int* __restrict__ parent, int* __restrict__ size) {
    const int row = blockIdx.y;
    const unsigned char* p = masks + (long)row * v;
    const int i0 = (blockIdx.x * MC_T + threadIdx.x) * MASK_ROW_VEC - mask_row_a0(p);    // >= -15; < 2^24 + 16 * MC_T
    const unsigned bits = mask_row_load(p, i0, v);                   // (nobody returns: the wave walk needs every lane)
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = np_unkey(box[6 * row + a]);                          // NaN for a row without a box: nothing is inside
        hi[a] = np_unkey(box[6 * row + 3 + a]);
    }
    const bool boxed = lo[0] <= hi[0];
    int* par = parent + (long)row * v;
    int* sz = size + (long)row * v;
    mask_wave_read(bits, i0, v, [&](int i, bool set) {
        int value = -2;
        if (!set) {
            value = -1;
            if (boxed) {
                const float x = xyz[3l * i], y = xyz[3l * i + 1], z = xyz[3l * i + 2];
                if (lo[0] <= x && x <= hi[0] && lo[1] <= y && y <= hi[1] && lo[2] <= z && z <= hi[2]) value = i;
            }
        }
        par[i] = value;
        sz[i] = 0;
    });
}

// the flag ORed into the size word of u's root in every row of m
__device__ __forceinline__ void hf_flag(u64 m, int j, int u, int v, int flag, const int* __restrict__ parent, int* size, int* __restrict__ bad) {
    while (m != 0ull) {
        const int k = j * 64 + __ffsll((long long)m) - 1;                                             // < r: the tables have no bit beyond
        m &= m - 1ull;
        const int root = parent[(long)k * v + u];                    // final: flatten is over
        if ((unsigned)root >= (unsigned)v) {
            bad[k] = 1;
            continue;
        }
        int* word = size + (long)k * v + root;
        if ((mc_load(word) & flag) == 0) atomicOr(word, flag);
    }
}

// grid (ceil(f / MC_T)): one face per lane
__global__ __launch_bounds__(MC_T) void hf_mark_kernel(int v, int f, int words, const int* __restrict__ faces, const u64* __restrict__ cand,
                                                       const u64* __restrict__ set, const int* __restrict__ parent, int* size, int* __restrict__ bad) {
    const long t = blockIdx.x * (long)MC_T + threadIdx.x;
    if (t >= f) return;
    const McFace face(faces, t);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        int u, w;
        if (!face.edge(e, v, u, w)) continue;
        for (int j = 0; j < words; ++j) {
            const u64 cu = cand[(long)u * words + j], cw = cand[(long)w * words + j];
            if ((cu | cw) == 0ull) continue;
            const u64 su = set[(long)u * words + j], sw = set[(long)w * words + j];
            hf_flag(cu & sw, j, u, v, HF_TOUCH, parent, size, bad);
            hf_flag(cu & ~cw & ~sw, j, u, v, HF_OPEN, parent, size, bad);
            hf_flag(cw & su, j, w, v, HF_TOUCH, parent, size, bad);
            hf_flag(cw & ~cu & ~su, j, w, v, HF_OPEN, parent, size, bad);
        }
    }
}

// grid (ceil(chunks / MC_T), r) over the ADDRESS of out's row
__global__ __launch_bounds__(MC_T) void hf_apply_kernel(int v, int max_vertices, double max_share, const int* __restrict__ parent,
                                                        const int* __restrict__ size, const int* __restrict__ points_in, const int* __restrict__ bad,
                                                        unsigned char* out, int* __restrict__ mask_points, int* __restrict__ nholes,
                                                        int* __restrict__ nfilled) {
    const int row = blockIdx.y;
    const bool marked = bad[row] != 0;                               // mark is over: nobody writes it any more
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (marked) nholes[row] = -1;                                // (nobody adds to it in a marked row)
        atomicAdd(&mask_points[row], points_in[row]);                // once a row: the waves below add what they fill
    }
    unsigned char* p = out + (long)row * v;
    const int i0 = (blockIdx.x * MC_T + threadIdx.x) * MASK_ROW_VEC - mask_row_a0(p);    // >= -15; < 2^24 + 16 * MC_T
    const int* par = parent + (long)row * v;
    const int* sz = size + (long)row * v;
    const double ceiling_share = max_share * (double)points_in[row];
    unsigned bits = 0u;
    int holes = 0, filled = 0;
#pragma unroll
    for (int t = 0; t < MASK_ROW_VEC; ++t) {
        const int i = mask_wave_vertex(i0, t);
        bool on = false;
        if (i >= 0 && i < v) {
            const int root = par[i];
            if (root == -2) on = true;
            else if ((unsigned)root < (unsigned)v) {                 // -1: unset and no candidate
                const int word = sz[root], s = word & HF_COUNT;
                on = (word & (HF_TOUCH | HF_OPEN)) == HF_TOUCH && s <= max_vertices && (double)s <= ceiling_share;
                if (on && root == i) {                               // summed over the roots, never per vertex
                    ++holes;
                    filled += s;
                }
            }
        }
        mask_wave_write(on, t, bits);
    }
    mask_row_store(p, i0, v, bits);
    holes = wave_sum_lane0(holes);
    filled = wave_sum_lane0(filled);                                 // <= v <= 2^24
    if (lane_id() == 0 && holes != 0 && !marked) {
        atomicAdd(&nholes[row], holes);
        atomicAdd(&nfilled[row], filled);
        atomicAdd(&mask_points[row], filled);
    }
}

}  // namespace

extern "C" long gspn_mask_hole_fill_ws_bytes(int r, int v, int f) { return hf_ws_bytes(r, v, f); }

extern "C" int gspn_mask_hole_fill(int r, int v, int f, const unsigned char* masks, const int* faces, const float* xyz, int max_vertices,
                                   double max_share, void* ws, unsigned char* out, int* mask_points, int* nholes, int* nfilled, int* label,
                                   void* stream) {
    const int rc = hf_check(r, v, f, masks, faces, xyz, max_vertices, max_share, ws, out, mask_points, nholes, nfilled);
    if (rc != 0) return rc;
    if (r == 0 || v == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const HfLayout l = hf_layout(r, v);
    char* base = static_cast<char*>(ws);
    u64* cand = reinterpret_cast<u64*>(base + l.cand);
    u64* set = reinterpret_cast<u64*>(base + l.set);
    int* size = reinterpret_cast<int*>(base + l.size);
    int* bad = reinterpret_cast<int*>(base + l.bad);
    int* box = reinterpret_cast<int*>(base + l.box);
    int* points_in = reinterpret_cast<int*>(base + l.points);
    int* parent = label ? label : reinterpret_cast<int*>(base + l.parent);
    hipLaunchKernelGGL(hf_prime_kernel, dim3((unsigned)((r + MC_T - 1) / MC_T)), dim3(MC_T), 0, st, r, box, points_in, bad, mask_points, nholes, nfilled);
    hipLaunchKernelGGL(hf_box_kernel, mc_by_vector(r, v), dim3(MC_T), 0, st, v, masks, xyz, box, points_in);
    hipLaunchKernelGGL(hf_init_kernel, mc_by_vector(r, v), dim3(MC_T), 0, st, v, masks, xyz, box, parent, size);
    if (f > 0) {                                                     // without faces nothing touches: no holes
        mc_join(st, r, v, f, l.words, faces, parent, cand, set, bad);
        hipLaunchKernelGGL(mc_flatten_kernel, mc_by_vertex(r, v), dim3(MC_T), 0, st, v, parent, size, bad);
        hipLaunchKernelGGL(hf_mark_kernel, dim3((unsigned)((f + MC_T - 1) / MC_T)), dim3(MC_T), 0, st, v, f, l.words, faces, cand, set, parent, size, bad);
    }
    hipLaunchKernelGGL(hf_apply_kernel, mc_by_vector(r, v), dim3(MC_T), 0, st, v, max_vertices, max_share, parent, size, points_in, bad, out, mask_points,
                       nholes, nfilled);
    return gspn_launch_status();
}
