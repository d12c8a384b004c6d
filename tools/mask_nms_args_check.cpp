// The host side of gspn_mask_overlaps / gspn_mask_nms (gspn_amd/csrc/mask_nms_args.h: the argument checks the launchers run before anything
// is launched, and the workspace layouts) as a stand-alone program, so that it can run under the host sanitizers without a device and
// without Python:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mask_nms_args_check.cpp -o tools/mask_nms_args_check
//     tools/mask_nms_args_check
//
// It walks the decline table of include/gspn_hip.h, the sizes at and one past every limit (where int arithmetic would overflow if the
// layout multiplied in int), and the layouts at the largest legal sizes.  Exit status 0 and "ok" when every row holds.
#include "../gspn_amd/csrc/mask_nms_args.h"
#include "args_check.h"

int main() {
    alignas(16) static char buf[64];
    const void *ok = buf, *odd = buf + 8, *null = nullptr;
    const int big = (1 << 24) + 1, imax = 0x7FFFFFFF;

    // ---- gspn_mask_overlaps ----
    EXPECT("overlaps: plain", mo_check(2, 3, 9, ok, ok, ok, ok), 0);
    EXPECT("overlaps: b < 0", mo_check(-1, 3, 9, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("overlaps: r < 0", mo_check(2, -1, 9, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("overlaps: v < 0", mo_check(2, 3, -1, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("overlaps: v = INT_MIN", mo_check(2, 3, -imax - 1, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("overlaps: masks null", mo_check(2, 3, 9, null, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("overlaps: ws null", mo_check(2, 3, 9, ok, null, ok, ok), GSPN_ERR_ARG);
    EXPECT("overlaps: sizes null", mo_check(2, 3, 9, ok, ok, null, ok), GSPN_ERR_ARG);
    EXPECT("overlaps: inter null", mo_check(2, 3, 9, ok, ok, ok, null), GSPN_ERR_ARG);
    EXPECT("overlaps: an argument error goes first", mo_check(-1, 1025, big, ok, odd, ok, ok), GSPN_ERR_ARG);
    EXPECT("overlaps: r = 1024", mo_check(2, 1024, 9, ok, ok, ok, ok), 0);
    EXPECT("overlaps: r > 1024", mo_check(2, 1025, 9, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("overlaps: v = 2^24", mo_check(2, 3, 1 << 24, ok, ok, ok, ok), 0);
    EXPECT("overlaps: v > 2^24", mo_check(2, 3, big, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("overlaps: v = INT_MAX", mo_check(2, 3, imax, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("overlaps: b = 65535", mo_check(65535, 3, 9, ok, ok, ok, ok), 0);
    EXPECT("overlaps: b > 65535", mo_check(65536, 3, 9, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("overlaps: everything INT_MAX", mo_check(imax, imax, imax, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("overlaps: ws not 16-byte aligned", mo_check(2, 3, 9, ok, odd, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("overlaps: nothing to do", mo_check(0, 0, 0, ok, ok, ok, ok), 0);

    // ---- gspn_mask_nms ----
    EXPECT("nms: plain", mn_check(2, 3, 9, ok, ok, 0.5, ok, ok, ok, ok), 0);
    EXPECT("nms: b < 0", mn_check(-1, 3, 9, ok, ok, 0.5, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("nms: r < 0", mn_check(2, -1, 9, ok, ok, 0.5, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("nms: v < 0", mn_check(2, 3, -1, ok, ok, 0.5, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("nms: masks null", mn_check(2, 3, 9, null, ok, 0.5, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("nms: count null", mn_check(2, 3, 9, ok, null, 0.5, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("nms: ws null", mn_check(2, 3, 9, ok, ok, 0.5, null, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("nms: out null", mn_check(2, 3, 9, ok, ok, 0.5, ok, null, ok, ok), GSPN_ERR_ARG);
    EXPECT("nms: keep null", mn_check(2, 3, 9, ok, ok, 0.5, ok, ok, null, ok), GSPN_ERR_ARG);
    EXPECT("nms: mask_points null", mn_check(2, 3, 9, ok, ok, 0.5, ok, ok, ok, null), GSPN_ERR_ARG);
    const double bad_th[] = {NAN, -NAN, -1e-300, -0.5, 1.0, 1.0000000000000002, 2.0, INFINITY, -INFINITY};
    for (double th : bad_th) EXPECT("nms: iou_th outside [0, 1)", mn_check(2, 3, 9, ok, ok, th, ok, ok, ok, ok), GSPN_ERR_ARG);
    const double good_th[] = {0.0, -0.0, 5e-324, 0.25, 1.0 / 3.0, 0.5, 0.999, 0.9999999999999999};
    for (double th : good_th) EXPECT("nms: iou_th inside [0, 1)", mn_check(2, 3, 9, ok, ok, th, ok, ok, ok, ok), 0);
    EXPECT("nms: an argument error goes first", mn_check(2, 1025, 9, ok, ok, 1.0, odd, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("nms: r = 1024", mn_check(2, 1024, 9, ok, ok, 0.5, ok, ok, ok, ok), 0);
    EXPECT("nms: r > 1024", mn_check(2, 1025, 9, ok, ok, 0.5, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("nms: v = 2^24", mn_check(2, 3, 1 << 24, ok, ok, 0.5, ok, ok, ok, ok), 0);
    EXPECT("nms: v > 2^24", mn_check(2, 3, big, ok, ok, 0.5, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("nms: b > 65535", mn_check(65536, 3, 9, ok, ok, 0.5, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("nms: everything INT_MAX", mn_check(imax, imax, imax, ok, ok, 0.5, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("nms: ws not 16-byte aligned", mn_check(2, 3, 9, ok, ok, 0.5, odd, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("nms: nothing to do", mn_check(0, 0, 0, ok, ok, 0.5, ok, ok, ok, ok), 0);

    // ---- the workspaces ----
    EXPECT("overlaps ws: 1, 1, 1", mo_ws_bytes(1, 1, 1), 16);                                       // one word, rounded up to 16
    EXPECT("overlaps ws: 2, 3, 9", mo_ws_bytes(2, 3, 9), 48);
    EXPECT("overlaps ws: 1, 100, 500000", mo_ws_bytes(1, 100, 500000), 8L * 100 * 7813 + 0);
    EXPECT("overlaps ws: the 2 GiB case", mo_ws_bytes(1, 1024, (1 << 21) + 3), 8L * 1024 * 32769);
    EXPECT("overlaps ws: the largest", mo_ws_bytes(65535, 1024, 1 << 24), 8L * 65535 * 1024 * (1 << 18));
    EXPECT("nms ws: 1, 1, 1", mn_ws_bytes(1, 1, 1), 16 + 16 + 4);
    EXPECT("nms ws: 2, 3, 9", mn_ws_bytes(2, 3, 9), 48 + 32 + 4 * 2 * 9);
    EXPECT("nms ws: 1, 100, 500000", mn_ws_bytes(1, 100, 500000), 8L * 100 * 7813 + 400 + 40000);
    EXPECT("nms ws: the largest", mn_ws_bytes(65535, 1024, 1 << 24), 8L * 65535 * 1024 * (1 << 18) + (4L * 65535 * 1024 + 15) / 16 * 16 + 4L * 65535 * 1024 * 1024);
    const int declined[][3] = {{-1, 3, 9}, {2, -1, 9}, {2, 3, -1}, {0, 3, 9}, {2, 0, 9}, {2, 3, 0}, {2, 1025, 9}, {2, 3, big}, {65536, 3, 9},
                               {imax, imax, imax}};
    for (const auto& d : declined) {
        EXPECT("overlaps ws: declined sizes", mo_ws_bytes(d[0], d[1], d[2]), 0);
        EXPECT("nms ws: declined sizes", mn_ws_bytes(d[0], d[1], d[2]), 0);
    }
    const MnLayout l = mn_layout(65535, 1023, (1 << 24) - 1, true);
    EXPECT("layout: words", l.words, 1 << 18);
    EXPECT("layout: the sizes are 16-byte aligned", l.sizes % 16, 0);
    EXPECT("layout: the matrix is 16-byte aligned", l.inter % 16, 0);
    EXPECT("layout: the sizes follow the words", l.sizes >= 8u * (size_t)65535 * 1023u * (size_t)(1 << 18), 1);
    EXPECT("layout: the matrix follows the sizes", l.inter >= l.sizes + 4u * (size_t)65535 * 1023u, 1);
    EXPECT("layout: v = 1 has one word", mn_layout(1, 1, 1, true).words, 1);
    EXPECT("layout: v = 64 has one word", mn_layout(1, 1, 64, true).words, 1);
    EXPECT("layout: v = 65 has two", mn_layout(1, 1, 65, true).words, 2);
    EXPECT("layout: an odd word count rounds up", mn_layout(1, 3, 9, true).sizes, 32);

    return args_check_done();
}
