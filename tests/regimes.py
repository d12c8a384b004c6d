"""Coordinate regimes for the geometry kernels: the inputs of tests/test_gpu_coordinate_regimes.py and tests/test_cpu_coordinate_regimes.py.

A regime moves a seeded base cloud off the unit scale on the host, in fp32: x' = fl32(fl32(x * s) + t).  The oracle and the kernel see the
same bits.  Five groups:
  rescale    s a power of two, t = 0: exact, so the oracle at scale s IS the oracle at scale 1 (same indices, distances times s^2)
  units      s = 1e-3, 1e3 (metres <-> millimetres): not exact
  underflow  s = 2^-60 .. 2^-80: squared distances subnormal, then zero
  placement  room-scale clouds (kind S) and a 1/16 raster far from the origin, and millimetres at an offset
  shape      a slab, a line, a tilted plane (the pre-passes choose cell counts per axis), at s = 1 and 2^10
The base clouds, the cases (shapes per kernel path) and the oracle's results live here, computed once per session and never written."""
import collections
import functools

import numpy as np

from oracle import oracle as O
from tests import data as D

POW2 = (2.0 ** -40, 2.0 ** -10, 2.0 ** 10, 2.0 ** 17)
UNITS = (1e-3, 1e3)
UNDERFLOW = (2.0 ** -60, 2.0 ** -62, 2.0 ** -66, 2.0 ** -70, 2.0 ** -80)
OFFSET_ROOM = (1000.25, -2000.5, 500.125)
OFFSET_FAR = (5e5, 5e5, 5e5)
SHAPES = ("slab", "line", "plane")
BALL_FLOOR = 1e-20            # the reference's max(sqrtf(d2), 1e-20f) < radius: a radius at or below it selects nothing

Regime = collections.namedtuple("Regime", "name group kind s t")


def _exp(s):
    return int(round(np.log2(s)))


REGIMES = ([Regime("rescale_2^%d" % _exp(s), "rescale", "U", s, None) for s in POW2]
           + [Regime("units_%g" % s, "units", "U", s, None) for s in UNITS]
           + [Regime("underflow_2^%d" % _exp(s), "underflow", "U", s, None) for s in UNDERFLOW]
           + [Regime("room_offset", "placement", "S", 1.0, OFFSET_ROOM), Regime("room_far", "placement", "S", 1.0, OFFSET_FAR),
              Regime("raster_far", "placement", "R", 1.0, OFFSET_FAR), Regime("room_mm_offset", "placement", "S", 1e3, OFFSET_ROOM)]
           + [Regime("%s_2^%d" % (k, _exp(s)), "shape", k, s, None) for k in SHAPES for s in (1.0, 2.0 ** 10)])
BY_NAME = {r.name: r for r in REGIMES}
# the ball query below 2^-62 has its radius under the reference's floor: one case of its own (BALL_BELOW_FLOOR) instead
BALL_REGIMES = [r for r in REGIMES if r.group != "underflow" or r.s >= 2.0 ** -62]
BALL_BELOW_FLOOR = BY_NAME["underflow_2^-70"]
# the box kernels carry absolute constants of the reference's own (box_shrink's 1e-3, the margins): units, placement and shape only
BOX_REGIMES = [r for r in REGIMES if r.group in ("units", "placement", "shape")]
ids = lambda regs: [r.name for r in regs]


def exact(reg):
    """the regime is an exact rescale of `unit_of(reg)`: a power of two in a range where nothing rounds, no offset"""
    return reg.t is None and reg.s != 1.0 and reg.s in POW2


def unit_of(reg):
    return Regime("unit_" + reg.kind, "unit", reg.kind, 1.0, None)


def kinds(reg):
    """the cloud kinds a kernel that asks for U and S is run on under this regime"""
    return ("U", "S") if reg.group in ("rescale", "units", "underflow") else (reg.kind,)


def shape_map(kind, x):
    """a unit-cube cloud x (..., 3) fp32 -> the same points as kind R (a 1/16 raster: exact far from the origin, ties survive), slab
    (extents 200 x 1 x 2^-7), line (only x varies) or plane (projected onto x + y + z = 1 in fp32); other kinds: unchanged"""
    x = np.asarray(x, np.float32)
    if kind == "R":
        return (np.floor(x * np.float32(64.0)) / np.float32(16.0)).astype(np.float32)
    if kind == "slab":
        return (x * np.array([200.0, 1.0, 2.0 ** -7], np.float32)).astype(np.float32)
    if kind == "line":
        y = x.copy()
        y[..., 1], y[..., 2] = np.float32(0.25), np.float32(0.5)
        return y
    if kind == "plane":
        return (x - (x.sum(-1, keepdims=True, dtype=np.float32) - np.float32(1.0)) / np.float32(3.0)).astype(np.float32)
    return x


def apply(reg, x):
    """x' = fl32(fl32(x * s) + t)"""
    y = (np.asarray(x, np.float32) * np.float32(reg.s)).astype(np.float32)
    if reg.t is not None:
        y = (y + np.array(reg.t, np.float32)).astype(np.float32)
    return np.ascontiguousarray(y)


def scaled(reg, v):
    """a length of the base cloud (a radius, a box size) under the regime: fl32(fl32(v) * s)"""
    return float(np.float32(v) * np.float32(reg.s))


@functools.lru_cache(maxsize=None)
def base(kind, b, n, seed, distinct=0):
    """the base cloud (b, n, 3) of a kind at unit scale; distinct > 0: every point drawn from the first `distinct` ones (FPS with more
    samples than distinct points ends in the max-min-dist == 0 tail, where only the tie rule picks)"""
    x = D.batch(kind, b, n, seed) if kind in ("U", "D", "S") else shape_map(kind, D.batch("U", b, n, seed))
    if distinct:
        rng = np.random.default_rng(1000 * seed + distinct)
        x = np.stack([x[i][rng.integers(0, distinct, size=n)] for i in range(b)])
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def cloud(reg, kind, b, n, seed, distinct=0):
    y = apply(reg, base(kind or reg.kind, b, n, seed, distinct))
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def queries(reg, kind, b, n, seed, m, push=0.0):
    """m points of cloud(...) at seeded positions; push: every second one moved by that much along x BEFORE the transform (a ball that
    hangs out of a dense cloud holds few points: such a row stays open through the ball query's prefix scan)"""
    x = base(kind or reg.kind, b, n, seed)
    rng = np.random.default_rng(7 * seed + m)
    q = np.stack([x[i][rng.permutation(n)[:m]] for i in range(b)]).astype(np.float32)
    if push:
        q[:, ::2, 0] += np.float32(push)
    y = apply(reg, q)
    y.setflags(write=False)
    return y


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- the cases: the smallest shape that selects each kernel path ---------------------------------------------------------------------

# farthest point sampling: (n, m, distinct); b = 2, seed 3
FPS_SMALL = [(2048, 256, 0), (1000, 300, 100)]                 # fps_small_kernel: n <= 2048; m > distinct points: the zero tail
FPS_ON_CHIP = [(4096, 512, 0), (4096, 512, 256)]               # resident / cells / cells_torch (FPS_MODE, FPS_CELLS_MIN_N = 64) and multi-CU
FPS_CELLS_OWN = [(9000, 1125, 0)]                              # the cell kernel in its own range (n >= 8192)
FPS_MULTI_G = (1, 2)

# ball query: (tag, kinds or None for the regime's own, n, m, r0, nsample, push)
BALL_CASES = [("scan", None, 4096, 256, 0.2, 16, 0.0), ("scan", None, 4096, 256, 0.2, 64, 0.0),
              ("ws", "US", 8192, 256, 0.2, 16, 0.0), ("ws", "US", 8192, 256, 0.2, 64, 0.0),      # U: grid declined at 16, taken at 64; S: taken
              ("cont", None, 9000, 256, 0.2, 16, 0.18), ("cont", None, 9000, 256, 0.2, 64, 0.18)]

# three_nn: known points m per kernel; n = 1500 queries, b = 2
NN_QUERIES = 1500
NN_KNOWN = [128, 1024, 1025, 3000, 8193]        # wave kernel (two instances), cell grid (two), thread per query (nn_grid_ok declines m > 8192)
NN_ORDERED = [3000, 8193]                       # the kernels that read `order`
NESTED_LEVELS = [1, 2, 4, 6]

KNN_CASES = [(3000, 100, 8), (3000, 100, 32)]                  # n, m, k
NND_CASES = [(2, 700, 300), (1024, 37, 40)]                    # b, n, m: one and two queries per lane (b * ceil(n / 512) >= 1024)
NEAREST_CASE = (5000, 3000)                                    # known m, queries n


def ball_kinds(reg, spec):
    return kinds(reg) if spec == "US" else (reg.kind,)


@functools.lru_cache(maxsize=None)
def fps_ref(reg, kind, n, m, distinct):
    return frozen(O.farthest_point_sample(m, cloud(reg, kind, 2, n, 3, distinct), mt=True))


@functools.lru_cache(maxsize=None)
def ball_ref(reg, kind, n, m, r0, ns, push):
    return frozen(*O.query_ball_point(scaled(reg, r0), ns, cloud(reg, kind, 2, n, 4), queries(reg, kind, 2, n, 4, m, push), mt=True))


def nn_inputs(reg, m):
    return cloud(reg, None, 2, NN_QUERIES, 10), cloud(reg, None, 2, m, 50)


@functools.lru_cache(maxsize=None)
def nn_ref(reg, m):
    O.set_mt(True)
    try:
        return frozen(*O.three_nn(*nn_inputs(reg, m)))
    finally:
        O.set_mt(False)


def knn_inputs(reg, n, m):
    return cloud(reg, None, 2, n, 12), cloud(reg, None, 2, m, 52)


@functools.lru_cache(maxsize=None)
def knn_ref(reg, n, m, k):
    return frozen(*O.knn_point(k, *knn_inputs(reg, n, m)))


def nnd_inputs(reg, b, n, m):
    return cloud(reg, None, b, n, 14), cloud(reg, None, b, m, 2000)


@functools.lru_cache(maxsize=None)
def nnd_ref(reg, b, n, m):
    O.set_mt(True)
    try:
        return frozen(*O.nn_distance(*nnd_inputs(reg, b, n, m)))
    finally:
        O.set_mt(False)


def nearest_inputs(reg):
    m, n = NEAREST_CASE
    return cloud(reg, None, 2, n, 16), cloud(reg, None, 2, m, 56)


@functools.lru_cache(maxsize=None)
def nearest_ref(reg):
    O.set_mt(True)
    try:
        d, i = O.three_nn(*nearest_inputs(reg))
    finally:
        O.set_mt(False)
    return frozen(np.ascontiguousarray(d[..., 0]), np.ascontiguousarray(i[..., 0]))


def times_s2(reg, d):
    """d * s^2 in fp32: exact for the power-of-two regimes (no result leaves the normal range), +inf stays +inf"""
    return (np.asarray(d, np.float32) * np.float32(reg.s * reg.s)).astype(np.float32)


def subnormal_fraction(d):
    d = np.asarray(d, np.float32)
    tiny = np.finfo(np.float32).tiny
    return float(((d > 0) & (d < tiny)).mean())
