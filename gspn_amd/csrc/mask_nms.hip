// mask_nms.hip -- mask NMS (additive at ABI 21): duplicate instance masks suppressed by pairwise IoU.  b scenes, each r
// mask rows of v bytes in priority order (row 0 the best, any nonzero byte set).  size[k] = the set bytes of row k, inter[i][j] = the
// vertices set in both rows.
//
//   gspn_mask_overlaps  init    zero sizes and inter                                                                    (grid-stride)
//                       pack    grid (blocks of 4096 vertices, r, b): the bytes become 64-bit words, ceil(v / 64) per row.  A block's 4096
//                               bytes start at an arbitrary address: the block reads the 257 chunks that cover them (the walk of
//                               mask_rows.h, begun at the block's first byte), one per lane, each giving its 16 bits to LDS; the bits
//                               outside the row's [0, v) are zero, so the bits beyond v in the last word are zero.  64 lanes then cut
//                               the 64 words out of that bit string at the block's misalignment; their popcounts, added by shuffles, go
//                               to sizes[row] with one integer atomicAdd per block
//                       gram    grid (chunk groups, pairs of 32-row tiles on or above the diagonal, b): both tiles' words of a chunk of 64
//                               words are staged in LDS (rows padded to 65 words: the 8 rows a half-wave reads fall on 8 different bank
//                               pairs), a lane accumulates __popcll(a & b) of 4 pairs over the chunks of its group and adds what is not
//                               zero to inter[i][j] and, off the diagonal tile, to inter[j][i] with integer atomicAdd
//   gspn_mask_nms       the three above into ws, then
//                       greedy  one workgroup per scene, the suppressed flags in LDS: live sequential steps; in step k, if row k is kept,
//                               the lanes spread over j > k test (double)inter[k][j] > iou_th * (double)(size[k] + size[j] - inter[k][j]),
//                               one IEEE multiply and a strict compare; the rows of inter are loaded 8 steps at a time, one block of 8
//                               ahead, sizes and labels come from LDS, and a slot of 256 rows none of which is live is passed over
//                               (75 live rows: 34.5 us with a load per step, 30.0 with the blocks, 21.6 with the slots skipped).  It writes
//                               keep and mask_points (size[k], or 0 for a suppressed row): the apply pass counts nothing
//                       apply   grid (chunks of 16 bytes / 256, r, b) over the ADDRESS of out's row (mask_rows.h): a lane cuts the 16 bits
//                               of its chunk out of the packed row -- zero for a suppressed row -- and writes the chunk.  It reads the
//                               packed words and never masks, so out may be masks
//
// Integer atomics only: the same bits on every call.  Row offsets are 64-bit (b * r * v exceeds 2^31).  No host synchronisation, nothing
// allocated; nothing is read from ws that the call did not write.
#include "common.h"
#include "mask_nms_args.h"
#include "mask_rows.h"

#define MN_T 256
#define MN_BLOCK_WORDS 64                // words a pack block writes: 4096 vertices, 256 chunks (+ 1 for the misalignment)
#define MN_TILE 32                       // rows per Gram tile
#define MN_CHUNK 64                      // words per Gram chunk
#define MN_PAD (MN_CHUNK + 1)
#define MN_GRAM_GROUPS 1024              // workgroups the Gram pass aims at; a group of chunks shares one set of atomics
#define MN_J 4                           // MN_MAX_R / MN_T: rows per lane of the greedy pass
#define MN_KB 8                          // steps of the greedy pass whose rows of inter are loaded together, one block ahead

typedef unsigned long long u64;

namespace {

__global__ __launch_bounds__(MN_T) void mn_init_kernel(long nsizes, long ninter, int* __restrict__ sizes, int* __restrict__ inter) {
    for (long i = blockIdx.x * (long)MN_T + threadIdx.x; i < nsizes; i += (long)gridDim.x * MN_T) sizes[i] = 0;
    for (long i = blockIdx.x * (long)MN_T + threadIdx.x; i < ninter; i += (long)gridDim.x * MN_T) inter[i] = 0;
}

// grid (ceil(words / 64), r, b)
__global__ __launch_bounds__(MN_T) void mn_pack_kernel(int r, int v, int words, const unsigned char* masks, u64* __restrict__ packed,
                                                       int* __restrict__ sizes) {
    __shared__ unsigned short sm[MN_T + 4];                          // 257 chunks' bits; a word reads 5 of them
    const long rr = (long)blockIdx.z * r + blockIdx.y;
    const unsigned char* p = masks + rr * v;
    const int vb = blockIdx.x * (MN_BLOCK_WORDS * 64);               // the block's first vertex, < v <= 2^24
    const int a0 = mask_row_a0(p + vb);
    const int tid = threadIdx.x;
    for (int q = tid; q <= MN_T; q += MN_T)                          // lane 0 takes the 257th chunk
        sm[q] = (unsigned short)mask_row_load(p, vb - a0 + MASK_ROW_VEC * q, v);
    __syncthreads();
    if (tid >= GSPN_WAVE) return;
    const int w = blockIdx.x * MN_BLOCK_WORDS + tid;
    int n = 0;
    if (w < words) {                                                 // bit a0 + 64 tid + j of the string is vertex vb + 64 tid + j
        const unsigned short* s = sm + 4 * tid;
        const u64 lo = (u64)s[0] | ((u64)s[1] << 16) | ((u64)s[2] << 32) | ((u64)s[3] << 48);
        const u64 word = a0 == 0 ? lo : (lo >> a0) | ((u64)s[4] << (64 - a0));
        packed[rr * words + w] = word;
        n = __popcll(word);
    }
    n = wave_sum_lane0(n);
    if (tid == 0 && n != 0) atomicAdd(&sizes[rr], n);
}

// grid (groups, tiles * (tiles + 1) / 2, b), tiles = ceil(r / 32); group g takes the chunks g, g + groups, ...
__global__ __launch_bounds__(MN_T) void mn_gram_kernel(int r, int words, int tiles, const u64* __restrict__ packed, int* __restrict__ inter) {
    __shared__ u64 sa[MN_TILE][MN_PAD];
    __shared__ u64 sb[MN_TILE][MN_PAD];
    int ti = 0, rest = blockIdx.y;                                   // pair number -> (ti, tj), tj >= ti
    while (rest >= tiles - ti) {
        rest -= tiles - ti;
        ++ti;
    }
    const int tj = ti + rest;
    const bool diag = ti == tj;
    const int tid = threadIdx.x;
    const u64* base = packed + (long)blockIdx.z * r * words;
    const int i = tid / 8, j0 = (tid % 8) * 4;
    int acc[4] = {0, 0, 0, 0};
    const int chunks = (words + MN_CHUNK - 1) / MN_CHUNK;
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int w0 = c * MN_CHUNK;
        for (int e = tid; e < MN_TILE * MN_CHUNK; e += MN_T) {
            const int row = e / MN_CHUNK, w = e % MN_CHUNK;
            const bool inside = w0 + w < words;
            const int ga = ti * MN_TILE + row, gb = tj * MN_TILE + row;
            sa[row][w] = inside && ga < r ? base[(long)ga * words + w0 + w] : 0ull;
            if (!diag) sb[row][w] = inside && gb < r ? base[(long)gb * words + w0 + w] : 0ull;
        }
        __syncthreads();
        const u64(*tb)[MN_PAD] = diag ? sa : sb;
#pragma unroll 4
        for (int w = 0; w < MN_CHUNK; ++w) {
            const u64 a = sa[i][w];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += __popcll(a & tb[j0 + k][w]);
        }
        __syncthreads();
    }
    int* out = inter + (long)blockIdx.z * r * r;
    const int gi = ti * MN_TILE + i;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int gj = tj * MN_TILE + j0 + k;
        if (gi < r && gj < r && acc[k] != 0) {
            atomicAdd(&out[(long)gi * r + gj], acc[k]);
            if (!diag) atomicAdd(&out[(long)gj * r + gi], acc[k]);   // a diagonal tile computes both halves itself
        }
    }
}

// grid (b): one workgroup per scene
__global__ __launch_bounds__(MN_T) void mn_greedy_kernel(int r, const int* __restrict__ count, const int* __restrict__ labels, double iou_th,
                                                         const int* __restrict__ sizes, const int* __restrict__ inter,
                                                         unsigned char* __restrict__ keep, int* __restrict__ mask_points) {
    __shared__ unsigned char supp[MN_MAX_R];
    const int bi = blockIdx.x, tid = threadIdx.x;
    const int* sz = sizes + (long)bi * r;
    const int* in = inter + (long)bi * r * r;
    const int* lb = labels ? labels + (long)bi * r : nullptr;
    const int live = min(max(count[bi], 0), r);
    __shared__ int size_s[MN_MAX_R], label_s[MN_MAX_R];
    int size_j[MN_J], label_j[MN_J], next[MN_KB][MN_J];
#pragma unroll
    for (int u = 0; u < MN_J; ++u) {
        const int j = u * MN_T + tid;
        size_j[u] = j < live ? sz[j] : 0;
        label_j[u] = j < live && lb ? lb[j] : 0;
        if (j < r) {
            supp[j] = 0;
            size_s[j] = size_j[u];
            label_s[j] = label_j[u];
        }
#pragma unroll
        for (int kk = 0; kk < MN_KB; ++kk) next[kk][u] = kk < live && j < live ? in[(long)kk * r + j] : 0;       // the first MN_KB rows of inter
    }
    __syncthreads();
    // The loads of inter do not depend on the flags: the rows of the NEXT block of MN_KB steps are requested before this block's steps
    // run, so the walk waits for memory once per block at most, not once per step.
    for (int k0 = 0; k0 < live; k0 += MN_KB) {
        int cur[MN_KB][MN_J];
#pragma unroll
        for (int kk = 0; kk < MN_KB; ++kk) {
            const int kn = k0 + MN_KB + kk;
#pragma unroll
            for (int u = 0; u < MN_J; ++u) {
                const int j = u * MN_T + tid;
                cur[kk][u] = next[kk][u];
                next[kk][u] = kn < live && j < live ? in[(long)kn * r + j] : 0;
            }
        }
#pragma unroll
        for (int kk = 0; kk < MN_KB; ++kk) {
            const int k = k0 + kk;
            if (k >= live) break;                                    // uniform
            if (!supp[k]) {                                          // uniform: a suppressed row suppresses nobody
                const int size_k = size_s[k], label_k = label_s[k];
#pragma unroll
                for (int u = 0; u < MN_J; ++u) {
                    if (u * MN_T >= live) break;                     // uniform: none of this slot's rows is live
                    const int j = u * MN_T + tid;
                    if (j > k && j < live && label_j[u] == label_k &&
                        (double)cur[kk][u] > iou_th * (double)(size_k + size_j[u] - cur[kk][u]))
                        supp[j] = 1;
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int u = 0; u < MN_J; ++u) {
        const int j = u * MN_T + tid;
        if (j < r) {
            const bool gone = j < live && supp[j];
            keep[(long)bi * r + j] = j < live && !gone ? 1 : 0;
            mask_points[(long)bi * r + j] = gone ? 0 : sz[j];
        }
    }
}

// grid (ceil(chunks / MN_T), r, b) over the address of out's row
__global__ __launch_bounds__(MN_T) void mn_apply_kernel(int r, int v, int words, const int* __restrict__ count, const unsigned char* __restrict__ keep,
                                                        const u64* __restrict__ packed, unsigned char* out) {
    const long rr = (long)blockIdx.z * r + blockIdx.y;
    unsigned char* p = out + rr * v;
    const int i0 = (blockIdx.x * MN_T + threadIdx.x) * MASK_ROW_VEC - mask_row_a0(p);    // >= -15; < 2^24 + 16 * MN_T
    if (i0 >= v) return;
    const int live = min(max(count[blockIdx.z], 0), r);
    const bool gone = (int)blockIdx.y < live && keep[rr] == 0;       // uniform over the workgroup
    unsigned bits = 0u;
    if (!gone) {                                                     // bit k = vertex i0 + k; the head chunk starts at vertex 0
        const u64* pw = packed + rr * words;
        const int j0 = max(i0, 0), w = j0 >> 6, sh = j0 & 63;
        u64 x = pw[w] >> sh;
        if (sh > 64 - MASK_ROW_VEC && w + 1 < words) x |= pw[w + 1] << (64 - sh);
        bits = ((unsigned)x << (j0 - i0)) & 0xFFFFu;                 // (the bits beyond v in the last word are zero)
    }
    mask_row_store(p, i0, v, bits);
}

void mn_overlaps(hipStream_t st, int b, int r, int v, const MnLayout& l, const unsigned char* masks, u64* packed, int* sizes, int* inter) {
    const long nsizes = (long)b * r, ninter = nsizes * r;
    const int tiles = (r + MN_TILE - 1) / MN_TILE, pairs = tiles * (tiles + 1) / 2;              // <= 528
    const int chunks = (l.words + MN_CHUNK - 1) / MN_CHUNK;
    long groups = MN_GRAM_GROUPS / ((long)pairs * b);
    groups = groups < 1 ? 1 : (groups > chunks ? chunks : groups);
    hipLaunchKernelGGL(mn_init_kernel, dim3(grid_for(ninter, MN_T)), dim3(MN_T), 0, st, nsizes, ninter, sizes, inter);
    hipLaunchKernelGGL(mn_pack_kernel, dim3((unsigned)((l.words + MN_BLOCK_WORDS - 1) / MN_BLOCK_WORDS), (unsigned)r, (unsigned)b), dim3(MN_T), 0, st,
                       r, v, l.words, masks, packed, sizes);
    hipLaunchKernelGGL(mn_gram_kernel, dim3((unsigned)groups, (unsigned)pairs, (unsigned)b), dim3(MN_T), 0, st, r, l.words, tiles, packed, inter);
}

}  // namespace

extern "C" long gspn_mask_overlaps_ws_bytes(int b, int r, int v) { return mo_ws_bytes(b, r, v); }

extern "C" int gspn_mask_overlaps(int b, int r, int v, const unsigned char* masks, void* ws, int* sizes, int* inter, void* stream) {
    const int rc = mo_check(b, r, v, masks, ws, sizes, inter);
    if (rc != 0) return rc;
    if (b == 0 || r == 0 || v == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const MnLayout l = mn_layout(b, r, v, false);
    mn_overlaps(st, b, r, v, l, masks, reinterpret_cast<u64*>(static_cast<char*>(ws) + l.packed), sizes, inter);
    return gspn_launch_status();
}

extern "C" long gspn_mask_nms_ws_bytes(int b, int r, int v) { return mn_ws_bytes(b, r, v); }

extern "C" int gspn_mask_nms(int b, int r, int v, const unsigned char* masks, const int* count, const int* labels, double iou_th, void* ws,
                             unsigned char* out, unsigned char* keep, int* mask_points, void* stream) {
    const int rc = mn_check(b, r, v, masks, count, iou_th, ws, out, keep, mask_points);
    if (rc != 0) return rc;
    if (b == 0 || r == 0 || v == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const MnLayout l = mn_layout(b, r, v, true);
    char* base = static_cast<char*>(ws);
    u64* packed = reinterpret_cast<u64*>(base + l.packed);
    int* sizes = reinterpret_cast<int*>(base + l.sizes);
    int* inter = reinterpret_cast<int*>(base + l.inter);
    mn_overlaps(st, b, r, v, l, masks, packed, sizes, inter);
    hipLaunchKernelGGL(mn_greedy_kernel, dim3((unsigned)b), dim3(MN_T), 0, st, r, count, labels, iou_th, sizes, inter, keep, mask_points);
    hipLaunchKernelGGL(mn_apply_kernel, dim3((unsigned)((mask_row_chunks(v) + MN_T - 1) / MN_T), (unsigned)r, (unsigned)b), dim3(MN_T), 0, st, r, v, l.words,
                       count, keep, packed, out);
    return gspn_launch_status();
}
