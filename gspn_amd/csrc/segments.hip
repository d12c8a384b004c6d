// segments.hip -- segment voting (additive at ABI 21): a scan's per-vertex masks and labels snapped to the segments of its
// mesh's over-segmentation.  One scan of v vertices, r mask rows of v bytes (any nonzero byte is set), seg[i] in [0, s) the segment of
// vertex i; a vertex whose seg lies outside [0, s) is unsegmented: it never votes, keeps its own byte (as 0 or 1) or label, and its id
// indexes nothing.
//
//   gspn_segment_vote        init     zero the (r + 1) * s counters and mask_points                                       (grid-stride)
//                            size     cnt[r][seg[i]] += 1 per segmented vertex, coalesced reads of seg
//                            count    grid (chunks of 16 bytes / 256, r) over the row's ADDRESS (the walk of mask_rows.h): a lane reads the 16
//                                     bits of one chunk and leaves when they are all zero (about one (row, vertex) pair in a hundred lies
//                                     inside a detection's box); a set byte reads seg and adds 1 to cnt[row][seg]
//                            decide   one lane per (row, segment): (double)cnt > vote_th * (double)size, one IEEE multiply and a strict
//                                     compare; the wave's ballot is the decision word of its 64 segments, and the sizes of its set segments,
//                                     added by shuffles, go to mask_points[row] with one integer atomicAdd: a set segment sets all its vertices
//                            apply    grid (tiles of 1024 vertices, groups of SV_ROWS rows): a lane keeps the seg of its four vertices in
//                                     registers across the group's rows, looks the row's bit up (a row's bitset is s / 8 bytes: it stays in
//                                     cache) and writes every byte of the tile.  Only the set bytes of UNSEGMENTED vertices are counted
//                                     here (shuffles, one atomicAdd per wave that has any): counting every set byte here put most waves of
//                                     a row on one counter, and that queue was two thirds of the call
//   gspn_segment_label_vote  init, count into cnt[seg][label], winner (one thread per segment: the first maximum over [0, c), -1 when
//                            nobody voted), gather
//
// Integer atomics only: the same bits on every call.  Row offsets are 64-bit (r * v exceeds 2^31).  out may be masks: the count pass is
// complete before the apply pass starts (stream order), and a lane of the apply pass reads only the bytes it writes.  No host
// synchronisation, nothing allocated; nothing is read from ws that the call did not write.
#include "common.h"
#include "mask_rows.h"
#include "segments_args.h"

#define SV_T 256
#define SV_Q 4                           // vertices per lane of the apply pass
#define SV_ROWS 8                        // rows per workgroup of the apply pass

namespace {

__global__ __launch_bounds__(SV_T) void sv_init_kernel(long ncnt, int npts, int* __restrict__ cnt, int* __restrict__ mask_points) {
    for (long i = blockIdx.x * (long)SV_T + threadIdx.x; i < ncnt; i += (long)gridDim.x * SV_T) cnt[i] = 0;
    for (long i = blockIdx.x * (long)SV_T + threadIdx.x; i < npts; i += (long)gridDim.x * SV_T) mask_points[i] = 0;
}

// size[seg] += 1 for every segmented vertex -- grid-stride over the vertices
__global__ __launch_bounds__(SV_T) void sv_size_kernel(int v, int s, const int* __restrict__ seg, int* __restrict__ size) {
    for (long i = blockIdx.x * (long)SV_T + threadIdx.x; i < v; i += (long)gridDim.x * SV_T) {
        const int sg = seg[i];
        if ((unsigned)sg < (unsigned)s) atomicAdd(&size[sg], 1);
    }
}

// grid (ceil(chunks / SV_T), r) over the row's address
__global__ __launch_bounds__(SV_T) void sv_count_kernel(int v, int s, const unsigned char* masks, const int* __restrict__ seg, int* __restrict__ cnt) {
    const int row = blockIdx.y;
    const unsigned char* p = masks + (long)row * v;
    const int i0 = (blockIdx.x * SV_T + threadIdx.x) * MASK_ROW_VEC - mask_row_a0(p);    // >= -15; < 2^24 + 16 * SV_T
    if (i0 >= v) return;
    const unsigned bits = mask_row_load(p, i0, v);
    if (bits == 0u) return;
    int* c = cnt + (long)row * s;
#pragma unroll
    for (int b = 0; b < MASK_ROW_VEC; ++b) {
        if ((bits >> b) & 1u) {                                      // a set byte lies inside [0, v)
            const int sg = seg[i0 + b];
            if ((unsigned)sg < (unsigned)s) atomicAdd(&c[sg], 1);
        }
    }
}

// one lane per (row, segment of a decision word); nwords = r * words
__global__ __launch_bounds__(SV_T) void sv_decide_kernel(long nwords, int words, int s, double vote_th, const int* __restrict__ cnt,
                                                         const int* __restrict__ size, unsigned long long* __restrict__ bits,
                                                         int* __restrict__ mask_points) {
    const long word = (blockIdx.x * (long)SV_T + threadIdx.x) / GSPN_WAVE;   // uniform over the wave
    if (word >= nwords) return;
    const int lane = threadIdx.x % GSPN_WAVE;
    const long row = word / words;
    const int sg = (int)(word - row * words) * GSPN_WAVE + lane;
    int members = 0;                                                 // the vertices this lane's segment sets in the row
    if (sg < s) {
        const int n = size[sg];
        if ((double)cnt[row * s + sg] > vote_th * (double)n) members = n;    // (cnt > 0 here, so n > 0)
    }
    const unsigned long long ballot = __ballot(members != 0);
    members = wave_sum_lane0(members);                                  // <= v <= 2^24
    if (lane == 0) {
        bits[word] = ballot;
        if (members != 0) atomicAdd(&mask_points[row], members);
    }
}

// grid (ceil(v / (SV_T * SV_Q)), ceil(r / SV_ROWS)).  in may be out: a lane reads only the bytes it then writes.
__global__ __launch_bounds__(SV_T) void sv_apply_kernel(int r, int v, int s, int words, const unsigned char* in, const int* __restrict__ seg,
                                                        const unsigned long long* __restrict__ bits, unsigned char* out,
                                                        int* __restrict__ mask_points) {
    const int tid = threadIdx.x, lane = tid % GSPN_WAVE;
    const int t0 = blockIdx.x * (SV_T * SV_Q);                       // < v <= 2^24
    int sg[SV_Q];
#pragma unroll
    for (int u = 0; u < SV_Q; ++u) {
        const int i = t0 + u * SV_T + tid;
        sg[u] = i < v ? seg[i] : -1;
    }
    const int row1 = min(r, ((int)blockIdx.y + 1) * SV_ROWS);
    for (int row = blockIdx.y * SV_ROWS; row < row1; ++row) {
        const unsigned long long* bw = bits + (long)row * words;
        const unsigned char* ip = in + (long)row * v;
        unsigned char* op = out + (long)row * v;
        int n = 0;
#pragma unroll
        for (int u = 0; u < SV_Q; ++u) {
            const int i = t0 + u * SV_T + tid;
            if (i < v) {
                const bool segmented = (unsigned)sg[u] < (unsigned)s;
                const bool set = segmented ? ((bw[sg[u] >> 6] >> (sg[u] & 63)) & 1ull) != 0ull : ip[i] != 0;
                op[i] = set ? 1 : 0;
                n += !segmented && set ? 1 : 0;                      // the segmented ones were counted by sv_decide_kernel
            }
        }
        n = wave_sum_lane0(n);
        if (lane == 0 && n != 0) atomicAdd(&mask_points[row], n);
    }
}

__global__ __launch_bounds__(SV_T) void sl_count_kernel(int v, int s, int c, const int* __restrict__ labels, const int* __restrict__ seg,
                                                        int* __restrict__ cnt) {
    for (long i = blockIdx.x * (long)SV_T + threadIdx.x; i < v; i += (long)gridDim.x * SV_T) {
        const int sg = seg[i], l = labels[i];
        if ((unsigned)sg < (unsigned)s && (unsigned)l < (unsigned)c) atomicAdd(&cnt[(long)sg * c + l], 1);
    }
}

// the first maximum of a segment's c counters, -1 when every one is zero
__global__ __launch_bounds__(SV_T) void sl_winner_kernel(int s, int c, const int* __restrict__ cnt, int* __restrict__ win) {
    for (long sg = blockIdx.x * (long)SV_T + threadIdx.x; sg < s; sg += (long)gridDim.x * SV_T) {
        const int* row = cnt + sg * c;
        int best = 0, arg = -1;
        for (int l = 0; l < c; ++l) {
            const int n = row[l];
            if (n > best) {                                          // strict: the lowest label among equal counts
                best = n;
                arg = l;
            }
        }
        win[sg] = arg;
    }
}

__global__ __launch_bounds__(SV_T) void sl_gather_kernel(int v, int s, const int* labels, const int* __restrict__ seg, const int* __restrict__ win,
                                                         int* out) {
    for (long i = blockIdx.x * (long)SV_T + threadIdx.x; i < v; i += (long)gridDim.x * SV_T) {
        const int sg = seg[i];
        int l = labels[i];
        if ((unsigned)sg < (unsigned)s) {
            const int w = win[sg];
            if (w >= 0) l = w;
        }
        out[i] = l;
    }
}

}  // namespace

extern "C" long gspn_segment_vote_ws_bytes(int r, int v, int s) { return sv_ws_bytes(r, v, s); }

extern "C" int gspn_segment_vote(int r, int v, int s, const unsigned char* masks, const int* seg, double vote_th, void* ws, unsigned char* out,
                                 int* mask_points, void* stream) {
    const int rc = sv_check(r, v, s, masks, seg, vote_th, ws, out, mask_points);
    if (rc != 0) return rc;
    if (r == 0 || v == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const SvLayout l = sv_layout(r, v, s);
    char* base = static_cast<char*>(ws);
    int* cnt = reinterpret_cast<int*>(base + l.cnt);
    int* size = cnt + (long)r * s;
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(base + l.bits);
    const long ncnt = ((long)r + 1) * s, nwords = (long)r * l.words;
    hipLaunchKernelGGL(sv_init_kernel, dim3(grid_for(ncnt > r ? ncnt : r, SV_T)), dim3(SV_T), 0, st, ncnt, r, cnt, mask_points);
    if (s > 0) {
        const int chunks = mask_row_chunks(v);
        hipLaunchKernelGGL(sv_size_kernel, dim3(grid_for(v, SV_T)), dim3(SV_T), 0, st, v, s, seg, size);
        hipLaunchKernelGGL(sv_count_kernel, dim3((unsigned)((chunks + SV_T - 1) / SV_T), (unsigned)r), dim3(SV_T), 0, st, v, s, masks, seg, cnt);
        hipLaunchKernelGGL(sv_decide_kernel, dim3((unsigned)((nwords * GSPN_WAVE + SV_T - 1) / SV_T)), dim3(SV_T), 0, st, nwords, l.words, s, vote_th,
                           cnt, size, bits, mask_points);
    }
    hipLaunchKernelGGL(sv_apply_kernel, dim3((unsigned)((v + SV_T * SV_Q - 1) / (SV_T * SV_Q)), (unsigned)((r + SV_ROWS - 1) / SV_ROWS)), dim3(SV_T), 0,
                       st, r, v, s, l.words, masks, seg, bits, out, mask_points);
    return gspn_launch_status();
}

extern "C" long gspn_segment_label_vote_ws_bytes(int v, int s, int c) { return sl_ws_bytes(v, s, c); }

extern "C" int gspn_segment_label_vote(int v, int s, int c, const int* labels, const int* seg, void* ws, int* out, void* stream) {
    const int rc = sl_check(v, s, c, labels, seg, ws, out);
    if (rc != 0) return rc;
    if (v == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const SlLayout l = sl_layout(v, s, c);
    char* base = static_cast<char*>(ws);
    int* cnt = reinterpret_cast<int*>(base + l.cnt);
    int* win = reinterpret_cast<int*>(base + l.win);
    if (s > 0) {
        const long ncnt = (long)s * c;
        hipLaunchKernelGGL(sv_init_kernel, dim3(grid_for(ncnt, SV_T)), dim3(SV_T), 0, st, ncnt, 0, cnt, (int*)nullptr);
        hipLaunchKernelGGL(sl_count_kernel, dim3(grid_for(v, SV_T)), dim3(SV_T), 0, st, v, s, c, labels, seg, cnt);
        hipLaunchKernelGGL(sl_winner_kernel, dim3(grid_for(s, SV_T)), dim3(SV_T), 0, st, s, c, cnt, win);
    }
    hipLaunchKernelGGL(sl_gather_kernel, dim3(grid_for(v, SV_T)), dim3(SV_T), 0, st, v, s, labels, seg, win, out);
    return gspn_launch_status();
}
