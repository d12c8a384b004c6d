// The host side of gspn_mask_hole_fill (gspn_amd/csrc/holes_args.h: the argument checks the launcher runs before anything is launched, and
// the workspace layout) as a stand-alone program, so that it can run under the host sanitizers without a device and without Python:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/holes_args_check.cpp -o tools/holes_args_check
//     tools/holes_args_check
//
// It walks the decline table of include/gspn_hip.h, the sizes at and one past every limit (where int arithmetic would overflow if the
// layout multiplied in int), and the layout at the largest legal sizes.  Exit status 0 and "ok" when every row holds.
#include "../gspn_amd/csrc/holes_args.h"
#include "args_check.h"

static long up16(long n) { return (n + 15) / 16 * 16; }

// p: masks, faces, xyz, ws, out, mask_points, nholes, nfilled
static int hf(int r, int v, int f, int mv, double sh, const void* const p[8]) {
    return hf_check(r, v, f, p[0], p[1], p[2], mv, sh, p[3], p[4], p[5], p[6], p[7]);
}

int main() {
    alignas(16) static char buf[64];
    const void *ok = buf, *odd = buf + 8, *null = nullptr;
    const int bigv = (1 << 24) + 1, bigf = (1 << 26) + 1, imax = 0x7FFFFFFF;
    const void* all[8] = {ok, ok, ok, ok, ok, ok, ok, ok};

    EXPECT("holes: plain", hf(3, 9, 5, 4, 0.5, all), 0);
    EXPECT("holes: r < 0", hf(-1, 9, 5, 4, 0.5, all), GSPN_ERR_ARG);
    EXPECT("holes: v < 0", hf(3, -1, 5, 4, 0.5, all), GSPN_ERR_ARG);
    EXPECT("holes: f < 0", hf(3, 9, -1, 4, 0.5, all), GSPN_ERR_ARG);
    EXPECT("holes: v = INT_MIN", hf(3, -imax - 1, 5, 4, 0.5, all), GSPN_ERR_ARG);
    const char* names[8] = {"holes: masks null", "holes: faces null", "holes: xyz null", "holes: ws null", "holes: out null",
                            "holes: mask_points null", "holes: nholes null", "holes: nfilled null"};
    for (int k = 0; k < 8; ++k) {
        const void* p[8] = {ok, ok, ok, ok, ok, ok, ok, ok};
        p[k] = null;
        EXPECT(names[k], hf(3, 9, 5, 4, 0.5, p), GSPN_ERR_ARG);
        EXPECT("holes: without faces only faces may be null", hf(3, 9, 0, 4, 0.5, p), k == 1 ? 0 : GSPN_ERR_ARG);
    }
    EXPECT("holes: max_vertices = 0", hf(3, 9, 5, 0, 0.5, all), 0);
    EXPECT("holes: max_vertices < 0", hf(3, 9, 5, -1, 0.5, all), GSPN_ERR_ARG);
    EXPECT("holes: max_vertices = INT_MIN", hf(3, 9, 5, -imax - 1, 0.5, all), GSPN_ERR_ARG);
    EXPECT("holes: max_vertices = INT_MAX", hf(3, 9, 5, imax, 0.5, all), 0);
    const double bad_share[] = {NAN, -NAN, -1e-300, -0.5, 1.0000000000000002, 2.0, INFINITY, -INFINITY};
    for (double s : bad_share) EXPECT("holes: max_share outside [0, 1]", hf(3, 9, 5, 4, s, all), GSPN_ERR_ARG);
    const double good_share[] = {0.0, -0.0, 5e-324, 0.25, 1.0 / 3.0, 0.5, 0.9999999999999999, 1.0};
    for (double s : good_share) EXPECT("holes: max_share inside [0, 1]", hf(3, 9, 5, 4, s, all), 0);
    const void* misplaced[8] = {ok, ok, ok, odd, ok, ok, ok, ok};
    EXPECT("holes: an argument error goes first", hf(1025, 9, 5, -1, 0.5, misplaced), GSPN_ERR_ARG);
    EXPECT("holes: a negative size goes first", hf(-1, bigv, bigf, 4, 0.5, misplaced), GSPN_ERR_ARG);
    EXPECT("holes: r = 1024", hf(1024, 9, 5, 4, 0.5, all), 0);
    EXPECT("holes: r > 1024", hf(1025, 9, 5, 4, 0.5, all), GSPN_ERR_UNSUPPORTED);
    EXPECT("holes: v = 2^24", hf(3, 1 << 24, 5, 4, 0.5, all), 0);
    EXPECT("holes: v > 2^24", hf(3, bigv, 5, 4, 0.5, all), GSPN_ERR_UNSUPPORTED);
    EXPECT("holes: f = 2^26", hf(3, 9, 1 << 26, 4, 0.5, all), 0);
    EXPECT("holes: f > 2^26", hf(3, 9, bigf, 4, 0.5, all), GSPN_ERR_UNSUPPORTED);
    EXPECT("holes: everything INT_MAX", hf(imax, imax, imax, 4, 0.5, all), GSPN_ERR_UNSUPPORTED);
    EXPECT("holes: a limit goes before the alignment", hf(1025, 9, 5, 4, 0.5, misplaced), GSPN_ERR_UNSUPPORTED);
    EXPECT("holes: ws not 16-byte aligned", hf(3, 9, 5, 4, 0.5, misplaced), GSPN_ERR_UNSUPPORTED);
    const void* nothing[8] = {ok, null, ok, ok, ok, ok, ok, ok};
    EXPECT("holes: nothing to do", hf(0, 0, 0, 4, 0.5, nothing), 0);

    // ---- the workspace: two tables of v * ceil(r / 64) words, then r * v, r, 6 r, r and r * v int32, each part 16-byte aligned ----
    EXPECT("ws: 1, 1", hf_ws_bytes(1, 1, 0), 16 + 16 + 16 + 16 + 32 + 16 + 4);
    EXPECT("ws: 3, 100", hf_ws_bytes(3, 100, 5), 800 + 800 + 1200 + 16 + 80 + 16 + 1200);
    EXPECT("ws: 65 rows have two words", hf_ws_bytes(65, 9, 5), 2 * 16 * 9 + up16(4 * 65 * 9) + up16(4 * 65) + up16(24 * 65) + up16(4 * 65) + 4 * 65 * 9);
    EXPECT("ws: 100, 500000", hf_ws_bytes(100, 500000, 1 << 20), 2 * 16L * 500000 + 8L * 100 * 500000 + 400 + 2400 + 400);
    EXPECT("ws: the largest", hf_ws_bytes(1024, 1 << 24, 1 << 26), 256L * (1 << 24) + 8L * 1024 * (1 << 24) + 8 * 4096);
    EXPECT("ws: f does not enter", hf_ws_bytes(3, 100, 0) == hf_ws_bytes(3, 100, 1 << 26), 1);
    const int declined[][3] = {{-1, 9, 5}, {3, -1, 5}, {3, 9, -1}, {0, 9, 5}, {3, 0, 5}, {1025, 9, 5}, {3, bigv, 5}, {3, 9, bigf}, {imax, imax, imax}};
    for (const auto& d : declined) EXPECT("ws: declined sizes", hf_ws_bytes(d[0], d[1], d[2]), 0);
    const HfLayout l = hf_layout(1023, (1 << 24) - 1);
    const size_t cells = 4u * 1023u * (size_t)((1 << 24) - 1), table = 8u * 16u * (size_t)((1 << 24) - 1);
    EXPECT("layout: words", l.words, 16);
    const size_t parts[7] = {l.cand, l.set, l.size, l.bad, l.box, l.points, l.parent};
    for (size_t part : parts) EXPECT("layout: every part is 16-byte aligned", part % 16, 0);
    EXPECT("layout: the set table follows the candidates", l.set >= l.cand + table, 1);
    EXPECT("layout: the counters follow the tables", l.size >= l.set + table, 1);
    EXPECT("layout: the marks follow the counters", l.bad >= l.size + cells, 1);
    EXPECT("layout: the boxes follow the marks", l.box >= l.bad + 4u * 1023u, 1);
    EXPECT("layout: the counts follow the boxes", l.points >= l.box + 24u * 1023u, 1);
    EXPECT("layout: the parents follow the counts", l.parent >= l.points + 4u * 1023u, 1);
    EXPECT("layout: the parents end the workspace", l.bytes == l.parent + cells, 1);
    EXPECT("layout: r = 64 has one word", hf_layout(64, 1).words, 1);
    EXPECT("layout: r = 65 has two", hf_layout(65, 1).words, 2);

    return args_check_done();
}
