// What the *_args_check.cpp programs share: EXPECT(what, got, want) compares two values as longs, prints a FAIL line and counts it when
// they differ; main ends with `return args_check_done();`, which prints "ok" and gives exit status 0 when every row held.
#pragma once
#include <math.h>
#include <stdio.h>

static int failures = 0;
#define EXPECT(what, got, want)                                                                              \
    do {                                                                                                     \
        const long g_ = (long)(got), w_ = (long)(want);                                                      \
        if (g_ != w_) { printf("FAIL %s: got %ld, expected %ld (line %d)\n", what, g_, w_, __LINE__); ++failures; } \
    } while (0)

static inline int args_check_done() {
    if (failures == 0) printf("ok\n");
    return failures == 0 ? 0 : 1;
}
