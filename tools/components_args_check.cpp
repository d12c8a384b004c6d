// The host side of gspn_mask_components / gspn_mask_component_filter (gspn_amd/csrc/components_args.h: the argument checks the launchers
// run before anything is launched, and the workspace layouts) as a stand-alone program, so that it can run under the host sanitizers
// without a device and without Python:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/components_args_check.cpp -o tools/components_args_check
//     tools/components_args_check
//
// It walks the decline table of include/gspn_hip.h, the sizes at and one past every limit (where int arithmetic would overflow if the
// layout multiplied in int), and the layouts at the largest legal sizes.  Exit status 0 and "ok" when every row holds.
#include "../gspn_amd/csrc/components_args.h"
#include "args_check.h"

static long up16(long n) { return (n + 15) / 16 * 16; }

int main() {
    alignas(16) static char buf[64];
    const void *ok = buf, *odd = buf + 8, *null = nullptr;
    const int bigv = (1 << 24) + 1, bigf = (1 << 26) + 1, imax = 0x7FFFFFFF;

    // ---- gspn_mask_components ----
    EXPECT("components: plain", mc_check(3, 9, 5, ok, ok, ok, ok, ok, ok), 0);
    EXPECT("components: r < 0", mc_check(-1, 9, 5, ok, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("components: v < 0", mc_check(3, -1, 5, ok, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("components: f < 0", mc_check(3, 9, -1, ok, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("components: v = INT_MIN", mc_check(3, -imax - 1, 5, ok, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("components: masks null", mc_check(3, 9, 5, null, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("components: faces null", mc_check(3, 9, 5, ok, null, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("components: faces null without faces", mc_check(3, 9, 0, ok, null, ok, ok, ok, ok), 0);
    EXPECT("components: ws null", mc_check(3, 9, 5, ok, ok, null, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("components: comp null", mc_check(3, 9, 5, ok, ok, ok, null, ok, ok), GSPN_ERR_ARG);
    EXPECT("components: ncomp null", mc_check(3, 9, 5, ok, ok, ok, ok, null, ok), GSPN_ERR_ARG);
    EXPECT("components: largest null", mc_check(3, 9, 5, ok, ok, ok, ok, ok, null), GSPN_ERR_ARG);
    EXPECT("components: an argument error goes first", mc_check(-1, bigv, bigf, ok, ok, odd, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("components: r = 1024", mc_check(1024, 9, 5, ok, ok, ok, ok, ok, ok), 0);
    EXPECT("components: r > 1024", mc_check(1025, 9, 5, ok, ok, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("components: v = 2^24", mc_check(3, 1 << 24, 5, ok, ok, ok, ok, ok, ok), 0);
    EXPECT("components: v > 2^24", mc_check(3, bigv, 5, ok, ok, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("components: f = 2^26", mc_check(3, 9, 1 << 26, ok, ok, ok, ok, ok, ok), 0);
    EXPECT("components: f > 2^26", mc_check(3, 9, bigf, ok, ok, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("components: everything INT_MAX", mc_check(imax, imax, imax, ok, ok, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("components: ws not 16-byte aligned", mc_check(3, 9, 5, ok, ok, odd, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("components: nothing to do", mc_check(0, 0, 0, ok, null, ok, ok, ok, ok), 0);

    // ---- gspn_mask_component_filter ----
    EXPECT("filter: plain", mf_check(3, 9, 5, ok, ok, 1, 0.5, ok, ok, ok, ok, ok), 0);
    EXPECT("filter: r < 0", mf_check(-1, 9, 5, ok, ok, 1, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: v < 0", mf_check(3, -1, 5, ok, ok, 1, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: f < 0", mf_check(3, 9, -1, ok, ok, 1, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: masks null", mf_check(3, 9, 5, null, ok, 1, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: faces null", mf_check(3, 9, 5, ok, null, 1, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: faces null without faces", mf_check(3, 9, 0, ok, null, 1, 0.5, ok, ok, ok, ok, ok), 0);
    EXPECT("filter: ws null", mf_check(3, 9, 5, ok, ok, 1, 0.5, null, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: out null", mf_check(3, 9, 5, ok, ok, 1, 0.5, ok, null, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: mask_points null", mf_check(3, 9, 5, ok, ok, 1, 0.5, ok, ok, null, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: ncomp null", mf_check(3, 9, 5, ok, ok, 1, 0.5, ok, ok, ok, null, ok), GSPN_ERR_ARG);
    EXPECT("filter: nkept null", mf_check(3, 9, 5, ok, ok, 1, 0.5, ok, ok, ok, ok, null), GSPN_ERR_ARG);
    EXPECT("filter: min_vertices = 0", mf_check(3, 9, 5, ok, ok, 0, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: min_vertices < 0", mf_check(3, 9, 5, ok, ok, -imax - 1, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: min_vertices = INT_MAX", mf_check(3, 9, 5, ok, ok, imax, 0.5, ok, ok, ok, ok, ok), 0);
    const double bad_share[] = {NAN, -NAN, -1e-300, -0.5, 1.0000000000000002, 2.0, INFINITY, -INFINITY};
    for (double s : bad_share) EXPECT("filter: min_share outside [0, 1]", mf_check(3, 9, 5, ok, ok, 1, s, ok, ok, ok, ok, ok), GSPN_ERR_ARG);
    const double good_share[] = {0.0, -0.0, 5e-324, 0.25, 1.0 / 3.0, 0.5, 0.9999999999999999, 1.0};
    for (double s : good_share) EXPECT("filter: min_share inside [0, 1]", mf_check(3, 9, 5, ok, ok, 1, s, ok, ok, ok, ok, ok), 0);
    EXPECT("filter: an argument error goes first", mf_check(1025, 9, 5, ok, ok, 0, 0.5, odd, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("filter: r > 1024", mf_check(1025, 9, 5, ok, ok, 1, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("filter: v > 2^24", mf_check(3, bigv, 5, ok, ok, 1, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("filter: f > 2^26", mf_check(3, 9, bigf, ok, ok, 1, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("filter: everything INT_MAX", mf_check(imax, imax, imax, ok, ok, 1, 0.5, ok, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("filter: ws not 16-byte aligned", mf_check(3, 9, 5, ok, ok, 1, 0.5, odd, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("filter: nothing to do", mf_check(0, 0, 0, ok, null, 1, 0.5, ok, ok, ok, ok, ok), 0);

    // ---- the workspaces: v * ceil(r / 64) words, r * v and r int32; the filter r * v and r int32 more, each part 16-byte aligned ----
    EXPECT("components ws: 1, 1", mc_ws_bytes(1, 1, 0), 16 + 16 + 4);
    EXPECT("components ws: 3, 100", mc_ws_bytes(3, 100, 5), 800 + 1200 + 12);
    EXPECT("filter ws: 3, 100", mf_ws_bytes(3, 100, 5), up16(800 + 1200 + 12) + 1200 + 12);
    EXPECT("components ws: 65 rows have two words", mc_ws_bytes(65, 9, 5), 16 * 9 + up16(4 * 65 * 9) + 4 * 65);
    EXPECT("components ws: 100, 500000", mc_ws_bytes(100, 500000, 1 << 20), 16L * 500000 + 4L * 100 * 500000 + 400);
    EXPECT("components ws: the 2^31 case", mc_ws_bytes(129, 1 << 24, 7), 24L * (1 << 24) + 4L * 129 * (1 << 24) + 4 * 129);
    EXPECT("components ws: the largest", mc_ws_bytes(1024, 1 << 24, 1 << 26), 128L * (1 << 24) + 4L * 1024 * (1 << 24) + 4096);
    EXPECT("filter ws: the largest", mf_ws_bytes(1024, 1 << 24, 1 << 26), 128L * (1 << 24) + 8L * 1024 * (1 << 24) + 2 * 4096);
    EXPECT("ws: f does not enter", mc_ws_bytes(3, 100, 0) == mc_ws_bytes(3, 100, 1 << 26) && mf_ws_bytes(3, 100, 0) == mf_ws_bytes(3, 100, 1 << 26), 1);
    const int declined[][3] = {{-1, 9, 5}, {3, -1, 5}, {3, 9, -1}, {0, 9, 5}, {3, 0, 5}, {1025, 9, 5}, {3, bigv, 5}, {3, 9, bigf}, {imax, imax, imax}};
    for (const auto& d : declined) {
        EXPECT("components ws: declined sizes", mc_ws_bytes(d[0], d[1], d[2]), 0);
        EXPECT("filter ws: declined sizes", mf_ws_bytes(d[0], d[1], d[2]), 0);
    }
    const McLayout l = mc_layout(1023, (1 << 24) - 1, true);
    EXPECT("layout: words", l.words, 16);
    EXPECT("layout: the counters are 16-byte aligned", l.size % 16, 0);
    EXPECT("layout: the marks are 16-byte aligned", l.bad % 16, 0);
    EXPECT("layout: the parents are 16-byte aligned", l.parent % 16, 0);
    EXPECT("layout: the maxima are 16-byte aligned", l.largest % 16, 0);
    EXPECT("layout: the counters follow the table", l.size >= 8u * 16u * (size_t)((1 << 24) - 1), 1);
    EXPECT("layout: the marks follow the counters", l.bad >= l.size + 4u * 1023u * (size_t)((1 << 24) - 1), 1);
    EXPECT("layout: the parents follow the marks", l.parent >= l.bad + 4u * 1023u, 1);
    EXPECT("layout: the maxima follow the parents", l.largest >= l.parent + 4u * 1023u * (size_t)((1 << 24) - 1), 1);
    EXPECT("layout: r = 1 has one word", mc_layout(1, 1, true).words, 1);
    EXPECT("layout: r = 64 has one word", mc_layout(64, 1, true).words, 1);
    EXPECT("layout: r = 65 has two", mc_layout(65, 1, true).words, 2);

    return args_check_done();
}
