// The host side of gspn_segment_vote / gspn_segment_label_vote (gspn_amd/csrc/segments_args.h: the argument checks the launchers run before
// anything is launched, and the workspace layouts) as a stand-alone program, so that it can run under the host sanitizers without a device
// and without Python:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/segments_args_check.cpp -o tools/segments_args_check
//     tools/segments_args_check
//
// It walks the decline table of include/gspn_hip.h, the sizes at and one past every limit (where int arithmetic would overflow if the
// checks multiplied in int), and the layouts at the largest legal sizes.  Exit status 0 and "ok" when every row holds.
#include "../gspn_amd/csrc/segments_args.h"
#include "args_check.h"

int main() {
    alignas(16) static char buf[64];
    const void *ok = buf, *odd = buf + 8, *null = nullptr;
    const int big = (1 << 24) + 1, imax = 0x7FFFFFFF;

    // ---- gspn_segment_vote ----
    EXPECT("vote: plain", sv_check(3, 9, 4, ok, ok, 0.5, ok, ok, ok), 0);
    EXPECT("vote: in place", sv_check(3, 9, 4, ok, ok, 0.0, ok, ok, ok), 0);
    EXPECT("vote: r < 0", sv_check(-1, 9, 4, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("vote: v < 0", sv_check(3, -1, 4, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("vote: s < 0", sv_check(3, 9, -1, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("vote: s = INT_MIN", sv_check(3, 9, -imax - 1, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("vote: masks null", sv_check(3, 9, 4, null, ok, 0.5, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("vote: seg null", sv_check(3, 9, 4, ok, null, 0.5, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("vote: ws null", sv_check(3, 9, 4, ok, ok, 0.5, null, ok, ok), GSPN_ERR_ARG);
    EXPECT("vote: out null", sv_check(3, 9, 4, ok, ok, 0.5, ok, null, ok), GSPN_ERR_ARG);
    EXPECT("vote: mask_points null", sv_check(3, 9, 4, ok, ok, 0.5, ok, ok, null), GSPN_ERR_ARG);
    const double bad_th[] = {NAN, -NAN, -1e-300, -0.5, 1.0, 1.0000000000000002, 2.0, INFINITY, -INFINITY};
    for (double th : bad_th) EXPECT("vote: vote_th outside [0, 1)", sv_check(3, 9, 4, ok, ok, th, ok, ok, ok), GSPN_ERR_ARG);
    const double good_th[] = {0.0, -0.0, 5e-324, 0.25, 1.0 / 3.0, 0.5, 0.999, 0.9999999999999999};
    for (double th : good_th) EXPECT("vote: vote_th inside [0, 1)", sv_check(3, 9, 4, ok, ok, th, ok, ok, ok), 0);
    EXPECT("vote: an argument error goes first", sv_check(-1, big, 4, ok, ok, 0.5, odd, ok, ok), GSPN_ERR_ARG);
    EXPECT("vote: v = 2^24", sv_check(3, 1 << 24, 4, ok, ok, 0.5, ok, ok, ok), 0);
    EXPECT("vote: v > 2^24", sv_check(3, big, 4, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("vote: v = INT_MAX", sv_check(3, imax, 4, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("vote: r = 65535", sv_check(65535, 9, 4, ok, ok, 0.5, ok, ok, ok), 0);
    EXPECT("vote: r > 65535", sv_check(65536, 9, 4, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("vote: r = INT_MAX", sv_check(imax, 9, imax, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("vote: s = 2^24", sv_check(15, 9, 1 << 24, ok, ok, 0.5, ok, ok, ok), 0);
    EXPECT("vote: s > 2^24", sv_check(1, 9, big, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("vote: (r + 1) * s = 2^28", sv_check(15, 9, 1 << 24, ok, ok, 0.5, ok, ok, ok), 0);
    EXPECT("vote: (r + 1) * s > 2^28", sv_check(16, 9, 1 << 24, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("vote: (r + 1) * s > 2^28, 100 rows", sv_check(100, 9, (1 << 28) / 101 + 1, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("vote: (r + 1) * s <= 2^28, 100 rows", sv_check(100, 9, (1 << 28) / 101, ok, ok, 0.5, ok, ok, ok), 0);
    EXPECT("vote: (r + 1) * s past 2^31", sv_check(65535, 9, 1 << 24, ok, ok, 0.5, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("vote: ws not 16-byte aligned", sv_check(3, 9, 4, ok, ok, 0.5, odd, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("vote: nothing to do", sv_check(0, 0, 0, ok, ok, 0.5, ok, ok, ok), 0);

    EXPECT("vote ws: 3, 9, 4", sv_ws_bytes(3, 9, 4), 64 + 8 * 3);
    EXPECT("vote ws: 7, 33, 65", sv_ws_bytes(7, 33, 65), (4L * 8 * 65 + 15) / 16 * 16 + 8L * 7 * 2);
    EXPECT("vote ws: 100 x 500000 / 20000", sv_ws_bytes(100, 500000, 20000), 4L * 101 * 20000 + 8L * 100 * 313);
    EXPECT("vote ws: the largest table", sv_ws_bytes(15, 1 << 24, 1 << 24), 4L * (1 << 28) + 8L * 15 * (1 << 18));
    EXPECT("vote ws: 65535 rows", sv_ws_bytes(65535, 9, 4096), 4L * 65536 * 4096 + 8L * 65535 * 64);
    EXPECT("vote ws: s = 0", sv_ws_bytes(3, 9, 0), 0);
    const int declined[][3] = {{-1, 9, 4}, {3, -1, 4}, {3, 9, -1}, {0, 9, 4}, {3, 0, 4}, {3, big, 4}, {65536, 9, 4}, {3, 9, big},
                               {16, 9, 1 << 24}, {imax, imax, imax}};
    for (const auto& d : declined) EXPECT("vote ws: declined sizes", sv_ws_bytes(d[0], d[1], d[2]), 0);
    const SvLayout l = sv_layout(15, 1 << 24, 1 << 24);
    EXPECT("vote layout: the decision words are 16-byte aligned", l.bits % 16, 0);
    EXPECT("vote layout: they follow the counters", l.bits >= sizeof(int) * 16u * (size_t)(1 << 24), 1);
    EXPECT("vote layout: words", l.words, 1 << 18);
    EXPECT("vote layout: odd counters round up", sv_layout(2, 5, 1).bits, 16);

    // ---- gspn_segment_label_vote ----
    EXPECT("labels: plain", sl_check(9, 4, 19, ok, ok, ok, ok), 0);
    EXPECT("labels: v < 0", sl_check(-1, 4, 19, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("labels: s < 0", sl_check(9, -1, 19, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("labels: c = 0", sl_check(9, 4, 0, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("labels: c < 0", sl_check(9, 4, -imax - 1, ok, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("labels: labels null", sl_check(9, 4, 19, null, ok, ok, ok), GSPN_ERR_ARG);
    EXPECT("labels: seg null", sl_check(9, 4, 19, ok, null, ok, ok), GSPN_ERR_ARG);
    EXPECT("labels: ws null", sl_check(9, 4, 19, ok, ok, null, ok), GSPN_ERR_ARG);
    EXPECT("labels: out null", sl_check(9, 4, 19, ok, ok, ok, null), GSPN_ERR_ARG);
    EXPECT("labels: v = 2^24", sl_check(1 << 24, 4, 19, ok, ok, ok, ok), 0);
    EXPECT("labels: v > 2^24", sl_check(big, 4, 19, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("labels: s > 2^24", sl_check(9, big, 1, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("labels: s * c = 2^28", sl_check(9, 1 << 24, 16, ok, ok, ok, ok), 0);
    EXPECT("labels: s * c > 2^28", sl_check(9, 1 << 24, 17, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("labels: s * c past 2^31", sl_check(9, 1 << 24, imax, ok, ok, ok, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("labels: c = INT_MAX alone", sl_check(9, 0, imax, ok, ok, ok, ok), 0);
    EXPECT("labels: ws not 16-byte aligned", sl_check(9, 4, 19, ok, ok, odd, ok), GSPN_ERR_UNSUPPORTED);
    EXPECT("labels ws: 9, 4, 5", sl_ws_bytes(9, 4, 5), 4 * 4 * 5 + 4 * 4);
    EXPECT("labels ws: the largest table", sl_ws_bytes(9, 1 << 24, 16), 4L * (1 << 28) + 4L * (1 << 24));
    const int declined_l[][3] = {{-1, 4, 5}, {9, -1, 5}, {9, 4, 0}, {0, 4, 5}, {big, 4, 5}, {9, big, 5}, {9, 1 << 24, 17}, {imax, imax, imax}};
    for (const auto& d : declined_l) EXPECT("labels ws: declined sizes", sl_ws_bytes(d[0], d[1], d[2]), 0);

    return args_check_done();
}
