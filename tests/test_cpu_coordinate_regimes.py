"""The premises of tests/test_gpu_coordinate_regimes.py, on the CPU oracle alone: for every input of that module the exact-rescale
identities hold in the reference (same indices and counts at a power-of-two scale as at scale 1, distances exactly d * s^2), and the
underflow regimes are what they are named for (at 2^-60 a quarter of the 3-NN distances subnormal, at 2^-66 nine tenths, at 2^-80 all
zero).  A change of seed or shape that loses a regime fails here, without a GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import regimes as R

EXACT = [r for r in R.REGIMES if R.exact(r)]


def test_the_regime_list_is_the_issue_s():
    groups = {g: [r for r in R.REGIMES if r.group == g] for g in ("rescale", "units", "underflow", "placement", "shape")}
    assert [r.s for r in groups["rescale"]] == [2.0 ** -40, 2.0 ** -10, 2.0 ** 10, 2.0 ** 17]
    assert [r.s for r in groups["units"]] == [1e-3, 1e3]
    assert [r.s for r in groups["underflow"]] == [2.0 ** -60, 2.0 ** -62, 2.0 ** -66, 2.0 ** -70, 2.0 ** -80]
    assert [(r.kind, r.s, r.t) for r in groups["placement"]] == [("S", 1.0, (1000.25, -2000.5, 500.125)), ("S", 1.0, (5e5, 5e5, 5e5)),
                                                                ("R", 1.0, (5e5, 5e5, 5e5)), ("S", 1e3, (1000.25, -2000.5, 500.125))]
    assert [(r.kind, r.s) for r in groups["shape"]] == [(k, s) for k in ("slab", "line", "plane") for s in (1.0, 1024.0)]
    assert len(EXACT) == 7 and all(r.group in ("rescale", "shape") for r in EXACT)
    assert [r.s for r in R.BALL_REGIMES if r.group == "underflow"] == [2.0 ** -60, 2.0 ** -62]
    assert all(R.scaled(r, 0.2) > R.BALL_FLOOR for r in R.BALL_REGIMES) and R.scaled(R.BALL_BELOW_FLOOR, 0.2) < R.BALL_FLOOR
    assert {r.group for r in R.BOX_REGIMES} == {"units", "placement", "shape"}


def test_the_transform_is_two_fp32_roundings_and_the_shapes_are_what_they_say():
    x = R.base("U", 1, 500, 1)
    for reg in R.REGIMES:
        y = R.apply(reg, x)
        assert y.dtype == np.float32 and np.isfinite(y).all()
        want = (x.astype(np.float64) * np.float64(np.float32(reg.s))).astype(np.float32)           # (a product of two floats is exact in double)
        if reg.t is not None:
            want = (want.astype(np.float64) + np.array(reg.t, np.float32).astype(np.float64)).astype(np.float32)
        np.testing.assert_array_equal(y, want)
        if R.exact(reg):                                                    # nothing rounded: the scale divides out again
            np.testing.assert_array_equal(y.astype(np.float64) / reg.s, x.astype(np.float64))
    slab, line, plane, raster = (R.base(k, 1, 4096, 2)[0] for k in ("slab", "line", "plane", "R"))
    ext = slab.max(0) - slab.min(0)
    assert 190 < ext[0] <= 200 and 0.9 < ext[1] <= 1 and 2.0 ** -8 < ext[2] <= 2.0 ** -7
    assert len(np.unique(line[:, 0])) > 4000 and len(np.unique(line[:, 1])) == 1 and len(np.unique(line[:, 2])) == 1
    assert np.abs(plane.astype(np.float64).sum(1) - 1.0).max() < 1e-6 and (plane.max(0) - plane.min(0)).min() > 1.0
    assert ((raster * 16) == np.round(raster * 16)).all()
    far = R.cloud(R.BY_NAME["raster_far"], None, 1, 4096, 2)[0]
    np.testing.assert_array_equal(far.astype(np.float64), raster.astype(np.float64) + 5e5)         # the raster is exact at 5e5
    assert len(np.unique(R.base("U", 2, 1000, 3, 100)[1], axis=0)) <= 100


@pytest.mark.parametrize("reg", EXACT, ids=R.ids(EXACT))
def test_exact_rescale_is_an_identity_of_the_oracle(reg):
    unit = R.unit_of(reg)
    for n, m, distinct in R.FPS_SMALL + R.FPS_ON_CHIP + R.FPS_CELLS_OWN:
        for kind in R.kinds(reg):
            np.testing.assert_array_equal(R.fps_ref(reg, kind, n, m, distinct), R.fps_ref(unit, kind, n, m, distinct))
    for tag, spec, n, m, r0, ns, push in R.BALL_CASES:
        for kind in R.ball_kinds(reg, spec):
            for got, want in zip(R.ball_ref(reg, kind, n, m, r0, ns, push), R.ball_ref(unit, kind, n, m, r0, ns, push)):
                np.testing.assert_array_equal(got, want)
    for m in R.NN_KNOWN:
        (d, i), (d1, i1) = R.nn_ref(reg, m), R.nn_ref(unit, m)
        np.testing.assert_array_equal(i, i1)
        np.testing.assert_array_equal(d, R.times_s2(reg, d1))
        assert R.subnormal_fraction(d) == 0
    for n, m, k in R.KNN_CASES:
        (v, i), (v1, i1) = R.knn_ref(reg, n, m, k), R.knn_ref(unit, n, m, k)
        np.testing.assert_array_equal(i, i1)
        np.testing.assert_array_equal(v, R.times_s2(reg, v1))
    for b, n, m in R.NND_CASES:
        for got, want in zip(R.nnd_ref(reg, b, n, m), R.nnd_ref(unit, b, n, m)):
            np.testing.assert_array_equal(got, want if want.dtype == np.int32 else R.times_s2(reg, want))
    (d, i), (d1, i1) = R.nearest_ref(reg), R.nearest_ref(unit)
    np.testing.assert_array_equal(i, i1)
    np.testing.assert_array_equal(d, R.times_s2(reg, d1))


def test_the_ball_cases_take_the_paths_they_are_named_for():
    """the volumetric estimate of ball_grid_build_kernel on the unit regime: U at r = 0.2 is dense at nsample 16 (the grid is declined) and
    sparse at 64, S is sparse at both; the pushed queries of the continuation cases leave rows with fewer than nsample hits in a cloud of
    more than 8192 points (a row the prefix scan cannot close)"""
    def expect(kind, n):
        x = R.base(kind, 2, n, 4)[0]
        ext = np.maximum(x.max(0) - x.min(0), 0.2)
        return n * 4.18879 * 0.2 ** 3 / float(np.prod(ext.astype(np.float64)))
    assert expect("U", 8192) >= 8 * 16 and expect("U", 8192) < 8 * 64 and expect("S", 8192) < 8 * 16
    unit = R.unit_of(R.BY_NAME["rescale_2^10"])
    for tag, spec, n, m, r0, ns, push in R.BALL_CASES:
        idx, cnt = R.ball_ref(unit, "U", n, m, r0, ns, push)
        if tag == "cont":
            assert n > 8192 and expect("U", n) >= 8 * 16 and (cnt < ns).any() and (cnt == ns).any()
    empty = R.ball_ref(R.BALL_BELOW_FLOOR, "U", 4096, 256, 0.2, 16, 0.0)
    assert not empty[0].any() and not empty[1].any()


def test_the_host_threshold_search_at_every_regime_s_radius():
    """gspn_ball_threshold(r) is the smallest float T with sqrtf(T) >= r, so that d2 < T is the reference's max(sqrtf(d2), 1e-20f) < r:
    held against that expression on the floats around T at the radius of every ball case -- r^2 is borderline at 2^-60 and subnormal at
    2^-62, where T steps by the fixed 2^-149 -- and 0 (nothing passes) below the floor"""
    import ctypes
    from gspn_amd import _lib
    lib = _lib.lib()
    for reg in R.BALL_REGIMES:
        r = np.float32(R.scaled(reg, 0.2))
        T = np.float32(lib.gspn_ball_threshold(ctypes.c_float(float(r))))
        assert T > 0
        near, lo, hi = [T], T, T
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(0), dtype=np.float32), np.nextafter(hi, np.float32(np.inf), dtype=np.float32)
            near += [lo, hi]
        for s in near:
            ref = max(np.sqrt(np.float32(s), dtype=np.float32), np.float32(1e-20)) < r
            assert (np.float32(s) < T) == bool(ref), (reg.name, r, s, T)
    tiny = np.finfo(np.float32).tiny
    assert np.float32(R.scaled(R.BY_NAME["underflow_2^-62"], 0.2)) ** 2 < tiny < np.float32(R.scaled(R.BY_NAME["underflow_2^-60"], 0.2)) ** 2 < 4 * tiny
    assert lib.gspn_ball_threshold(ctypes.c_float(R.scaled(R.BALL_BELOW_FLOOR, 0.2))) == 0.0
    b, n, m = R.NND_CASES[1]
    assert b * ((n + 511) // 512) >= 1024 and b * ((m + 511) // 512) >= 1024          # nm_distance_kernel<2> in both directions (nndistance.hip)
    assert R.NND_CASES[0][0] * ((R.NND_CASES[0][1] + 511) // 512) < 1024
    assert min(R.NN_KNOWN) <= 128 and 1024 in R.NN_KNOWN and 1025 in R.NN_KNOWN and max(R.NN_KNOWN) > 8192      # wave / grid / thread per query


@pytest.mark.parametrize("m", R.NN_KNOWN)
def test_the_underflow_regimes_are_subnormal_then_zero(m):
    frac = {r.s: R.subnormal_fraction(R.nn_ref(r, m)[0]) for r in R.REGIMES if r.group == "underflow"}
    zero = float((R.nn_ref(R.BY_NAME["underflow_2^-80"], m)[0] == 0).mean())
    print("m = %d: subnormal fractions %s, zero at 2^-80: %.3f" % (m, {R._exp(s): round(f, 3) for s, f in frac.items()}, zero))
    assert frac[2.0 ** -60] >= 0.25
    assert frac[2.0 ** -66] >= 0.9
    assert zero == 1.0


def test_the_issue_s_own_input_gives_its_figures():
    """D.batch("U", 2, 4096, 3), queries = the oracle's 256 FPS samples: 51 %, 98 % subnormal 3-NN distances at 2^-60, 2^-66; at 2^-70 some
    are exactly 0; at 2^-80 all 24576 are 0, and FPS at 2^-60 still picks what it picks at scale 1"""
    x = R.base("U", 2, 4096, 3)
    at = lambda s: (x * np.float32(s)).astype(np.float32)
    idx = O.farthest_point_sample(256, x)
    nn = lambda s: O.three_nn(at(s), O.gather_point(at(s), idx))[0]
    assert abs(R.subnormal_fraction(nn(2.0 ** -60)) - 12597 / 24576) < 1e-9
    assert abs(R.subnormal_fraction(nn(2.0 ** -66)) - 24064 / 24576) < 1e-9
    assert int((nn(2.0 ** -70) == 0).sum()) >= 768                      # the 768 queries' own points at the least
    assert (nn(2.0 ** -80) == 0).all()
    np.testing.assert_array_equal(O.farthest_point_sample(256, at(2.0 ** -60)), idx)
    assert not np.array_equal(O.farthest_point_sample(256, at(2.0 ** -66)), idx)
