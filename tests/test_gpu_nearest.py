"""GPU tests of nearest_point (gspn_amd/nearest.py, csrc/nearest.hip).  The expected pair is column 0 of oracle.three_nn --
the host loop of tf_interpolate.cpp:60-103 -- unless a test says otherwise; dist is compared by its bits and idx exactly, nothing has a
tolerance.  Sizes are the smallest that select each path: one known point, fewer than a cell's worth, one workgroup and several in the
build, one and several query workgroups, 18 000 known points (a scene), 300 000 (the capped cell table -- 2^16 cells where a quarter of the points is 75 000 -- and 293 build workgroups)."""
import ctypes

import numpy as np
import pytest
import torch

from gspn_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def nearest(q, known, ws=None):
    from gspn_amd.nearest import nearest_point
    d, i = nearest_point(torch.from_numpy(np.ascontiguousarray(q)).cuda(), torch.from_numpy(np.ascontiguousarray(known)).cuda(), ws)
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and tuple(d.shape) == tuple(i.shape) == q.shape[:2]
    return d.cpu().numpy(), i.cpu().numpy()


def expected(q, known):
    d, i = O.three_nn(q, known)
    return np.ascontiguousarray(d[:, :, 0]), np.ascontiguousarray(i[:, :, 0])


def same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    bad = np.nonzero((gd.view(np.int32) != wd.view(np.int32)) | (gi != wi))
    assert not len(bad[0]), "%s: %d of %d pairs differ, first at %s: (%r, %d) for (%r, %d)" % (
        what, len(bad[0]), gd.size, tuple(int(a[0]) for a in bad), gd[bad][0], gi[bad][0], wd[bad][0], wi[bad][0])


def against_oracle(q, known, what):
    got = nearest(q, known)
    same(got, expected(q, known), what)
    return got


# ---- clouds --------------------------------------------------------------------------------------------------------------------------------

def room(m, seed):
    return (np.random.default_rng(seed).random((m, 3), dtype=np.float32) * np.array([8, 8, 3], np.float32)).astype(np.float32)


def flat(m, seed):
    x = synth.cloud_u(m, seed)
    x[:, 2] = np.float32(0.375)
    return x


def identical(m, seed):
    return np.tile(synth.cloud_u(1, seed), (m, 1))


def copies(m, seed):
    """a quarter of the cloud (500 of 2500) is one point, scattered through the index range"""
    x = synth.cloud_u(m, seed)
    at = np.random.default_rng(seed + 1).permutation(m)[:max(m // 5, 1)]
    x[at] = x[at[0]]
    return x


KINDS = {"uniform": synth.cloud_u, "room": room, "flat": flat, "identical": identical, "copies": copies, "duplicates": synth.cloud_d,
         "faces": synth.cloud_s}


def queries(known, n, seed):
    """around the known cloud: a third uniform in its box grown by a tenth, a third known points moved a little, a third known points"""
    rng = np.random.default_rng(seed)
    lo, hi = known.min(0), known.max(0)
    ext = np.maximum(hi - lo, np.float32(0.05))
    u = (lo - 0.1 * ext + rng.random((n, 3), dtype=np.float32) * 1.2 * ext).astype(np.float32)
    pick = known[rng.integers(0, len(known), n)]
    moved = (pick + np.float32(0.01) * ext * rng.standard_normal((n, 3)).astype(np.float32)).astype(np.float32)
    which = rng.integers(0, 3, n)[:, None]
    return np.where(which == 0, u, np.where(which == 1, moved, pick)).astype(np.float32)


# every value of m in {1, 2, 3, 64, 65, 257, 1025, 8193, 18000}, of n in {1, 255, 256, 257, 5000} and of b in {1, 3}; every kind
SIZES = [
    (1, 1, 1, ("uniform",)), (1, 255, 2, ("uniform",)), (3, 256, 3, ("uniform", "room", "flat")), (1, 257, 64, ("identical",)),
    (1, 1, 65, ("flat",)), (3, 255, 257, ("duplicates", "identical", "copies")), (1, 256, 1025, ("room",)), (1, 5000, 2500, ("copies",)),
    (1, 257, 8193, ("faces",)), (3, 257, 8193, ("flat", "duplicates", "room")), (3, 5000, 18000, ("uniform", "faces", "duplicates")),
    (1, 5000, 18000, ("room",)),
]


@pytest.mark.parametrize("b,n,m,kinds", SIZES, ids=lambda v: "-".join(v) if isinstance(v, tuple) else str(v))
def test_sizes_and_cloud_kinds(b, n, m, kinds):
    assert len(kinds) == b
    known = np.stack([KINDS[k](m, 11 + s) for s, k in enumerate(kinds)]).astype(np.float32)
    q = np.stack([queries(known[s], n, 5 + s) for s in range(b)])
    d, i = against_oracle(q, known, "%d x %d <- %d %s" % (b, n, m, kinds))
    assert i.min() >= 0 and i.max() < m and np.isfinite(d).all()


def test_the_size_lists_hold_every_value_the_definition_names():
    assert {s[2] for s in SIZES} >= {1, 2, 3, 64, 65, 257, 1025, 8193, 18000} and {s[1] for s in SIZES} == {1, 255, 256, 257, 5000}
    assert {s[0] for s in SIZES} == {1, 3} and (3, 5000, 18000) in {s[:3] for s in SIZES}
    assert {k for s in SIZES for k in s[3]} == set(KINDS)


@pytest.mark.parametrize("shuffle", [0, 1, 2])
def test_ties_across_cells_go_to_the_lowest_index(shuffle):
    """the lattice {0..7}^3 in shuffled order: a query with h half-integer coordinates has 2^h nearest lattice points at exactly equal
    distance (every term is a multiple of 1/4), in up to 2^h different cells of the 5 x 5 x 5 grid 512 points get"""
    g = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    known = lattice[np.random.default_rng(shuffle).permutation(512)]
    half = np.arange(7, dtype=np.float32) + np.float32(0.5)
    groups = {8: (half, half, half), 4: (half, g, half), 2: (g, half, g), 1: (g, g, g)}
    for ways, axes in groups.items():
        q = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
        d, i = against_oracle(q[None], known[None], "%d-way ties, shuffle %d" % (ways, shuffle))
        exact = ((q[:, None].astype(np.float64) - known[None].astype(np.float64)) ** 2).sum(-1)
        tied = exact == exact.min(1, keepdims=True)
        assert (tied.sum(1) == ways).all() and np.array_equal(i[0], tied.argmax(1)) and np.array_equal(d[0].astype(np.float64), exact.min(1))


def test_large_absolute_coordinates():
    """coordinates around 5e5 with an extent of 4 -- an ulp is 1/16 there, the cells are a few of them wide"""
    rng = np.random.default_rng(3)
    known = (np.float32(5e5) + rng.random((2, 3000, 3), dtype=np.float32) * np.float32(4)).astype(np.float32)
    q = (np.float32(5e5) - np.float32(0.5) + rng.random((2, 1000, 3), dtype=np.float32) * np.float32(5)).astype(np.float32)
    against_oracle(q, known, "offset 5e5")
    known[1, :, 0] -= np.float32(1e6)                                            # and around -5e5 on one axis
    q[1, :, 0] -= np.float32(1e6)
    against_oracle(q, known, "offset -5e5 on x")


def test_queries_outside_the_box_and_on_known_points():
    rng = np.random.default_rng(4)
    known = room(2000, 8)
    lo, hi = known.min(0), known.max(0)
    inside = (lo + rng.random((60, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    rows = []
    for a in range(3):
        for side, sign in ((lo, -1), (hi, 1)):
            face = inside[:10 * (2 * a + 1)][-10:].copy()
            face[:, a] = side[a] + np.float32(sign * 1e-3)
            far = face.copy()
            far[:, a] = side[a] + np.float32(sign * 10) * (hi - lo)[a]
            rows += [face, far]
    corner = (hi + 10 * (hi - lo)).astype(np.float32)[None]
    on = known[rng.integers(0, 2000, 300)]
    q = np.concatenate(rows + [corner, (lo - 10 * (hi - lo))[None].astype(np.float32), on])
    d, i = against_oracle(q[None], known[None], "outside the box")
    assert len(q) == 120 + 2 + 300 and not d[0, -300:].any() and np.array_equal(known[i[0, -300:]], on)


def test_non_finite_inputs():
    rng = np.random.default_rng(5)
    known = rng.random((2, 1500, 3), dtype=np.float32)
    q = rng.random((2, 600, 3), dtype=np.float32)
    known[0, 7, 1], known[0, 9, 0], known[1, 0, 2], known[1, 1499, 0] = np.nan, np.inf, -np.inf, np.nan
    q[0, 3], q[0, 5, 2], q[1, 0, 0], q[1, 599, 1] = np.nan, np.inf, -np.inf, np.nan
    q[0, 10], q[0, 11] = known[0, 7], known[0, 9]                                # queries that ARE the non-finite points
    q[0, 12:14] = np.nan_to_num(known[0, [7, 9]], nan=0.5, posinf=1.0)           # and finite ones beside them
    d, i = against_oracle(q, known, "non-finite")
    dead = ~np.isfinite(q).all(-1)
    assert dead.sum() == 6 and np.isposinf(d[dead]).all() and not i[dead].any()              # no winner: (+inf, 0)
    assert np.isfinite(d[~dead]).all()
    assert not np.isin(i[0][~dead[0]], [7, 9]).any() and not np.isin(i[1][~dead[1]], [0, 1499]).any()     # a non-finite point never wins
    # nothing finite among the known points: every query keeps (+inf, 0)
    d, i = against_oracle(q[:1, :300], np.full((1, 5, 3), np.nan, np.float32), "all-NaN known points")
    assert np.isposinf(d).all() and not i.any()
    known_inf = np.full((1, 70, 3), np.inf, np.float32)
    known_inf[0, 1::2] = -np.inf
    d, i = against_oracle(q[:1, :300], known_inf, "all-inf known points")
    assert np.isposinf(d).all() and not i.any()


def first_minimum_torch(q, known, chunk=128):
    """the same unfused float32 operations in torch on the device, a chunk of queries at a time; argmin returns the first minimum"""
    ds, ids = [], []
    for at in range(0, q.shape[0], chunk):
        diff = known[None, :, :] - q[at:at + chunk, None, :]
        sq = diff * diff
        d = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        k = torch.argmin(d, 1)
        ds.append(torch.gather(d, 1, k[:, None])[:, 0])
        ids.append(k.int())
    return torch.cat(ds), torch.cat(ids)


def test_large_m_takes_the_capped_table_and_many_build_workgroups():
    m, n = 300000, 2000
    known = torch.from_numpy(room(m, 21)).cuda()
    q = torch.from_numpy(queries(known[:5000].cpu().numpy(), n, 22)).cuda()
    from gspn_amd.nearest import nearest_point
    d, i = nearest_point(q[None], known[None])
    wd, wi = first_minimum_torch(q, known)
    assert torch.equal(d[0].view(torch.int32), wd.view(torch.int32)) and torch.equal(i[0], wi)
    assert m // 4 > 1 << 16 and int(i.max()) > m // 2


def test_two_calls_give_the_same_bits_whatever_the_workspace_held():
    from gspn_amd import _lib
    from gspn_amd.nearest import nearest_point
    known = torch.from_numpy(np.stack([synth.cloud_d(9000, 1), room(9000, 2)])).cuda()
    q = torch.from_numpy(np.stack([queries(known[s].cpu().numpy(), 3000, 3 + s) for s in range(2)])).cuda()
    need = int(_lib.lib().gspn_nearest_point_ws_bytes(2, 9000))
    assert need >= 2 * 9000 * 16
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    a, b = nearest_point(q, known), nearest_point(q, known, ws)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    again = nearest_point(q, known, ws)                                          # and on the workspace the call itself left behind
    assert torch.equal(a[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(a[1], again[1])
    same((a[0].cpu().numpy(), a[1].cpu().numpy()), expected(q.cpu().numpy(), known.cpu().numpy()), "2 x 3000 <- 9000")


def test_the_call_captures_with_a_caller_owned_workspace():
    from gspn_amd import _lib
    from gspn_amd.nearest import nearest_point
    b, n, m = 2, 700, 5000
    inputs = [(np.stack([queries(room(m, 30 + r + s), n, r) for s in range(b)]), np.stack([room(m, 30 + r + s) for s in range(b)])) for r in range(3)]
    q, known = torch.from_numpy(inputs[0][0]).cuda(), torch.from_numpy(inputs[0][1]).cuda()
    ws = torch.empty((int(_lib.lib().gspn_nearest_point_ws_bytes(b, m)),), dtype=torch.uint8, device="cuda")
    nearest_point(q, known, ws)                                                  # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = nearest_point(q, known, ws)
    for nq, nk in inputs[1:]:
        q.copy_(torch.from_numpy(nq))
        known.copy_(torch.from_numpy(nk))
        graph.replay()
        torch.cuda.synchronize()
        eager = nearest_point(q.clone(), known.clone())
        assert torch.equal(out[0].view(torch.int32), eager[0].view(torch.int32)) and torch.equal(out[1], eager[1])
        same((out[0].cpu().numpy(), out[1].cpu().numpy()), expected(nq, nk), "replayed")


def test_declined_sizes_and_a_short_workspace():
    from gspn_amd import _lib
    from gspn_amd.nearest import NEAREST_MAX_M, nearest_point
    lib = _lib.lib()
    tiny = torch.zeros(64, dtype=torch.float32, device="cuda")
    out_d, out_i = torch.full((4,), 7.0, device="cuda"), torch.full((4,), 7, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                  # noqa: E731
    null = ctypes.c_void_p(0)
    assert NEAREST_MAX_M == 1 << 24
    assert lib.gspn_nearest_point(1, 1, NEAREST_MAX_M + 1, p(tiny), p(tiny), p(tiny), p(out_d), p(out_i), null) == -2
    assert lib.gspn_nearest_point_ws_bytes(1, NEAREST_MAX_M + 1) == 0 and lib.gspn_nearest_point_ws_bytes(1, NEAREST_MAX_M) > 0
    assert lib.gspn_nearest_point(1, 1, 0, p(tiny), p(tiny), p(tiny), p(out_d), p(out_i), null) == -1
    assert lib.gspn_nearest_point(-1, 1, 1, p(tiny), p(tiny), p(tiny), p(out_d), p(out_i), null) == -1
    assert lib.gspn_nearest_point(1, 1, 1, p(tiny), p(tiny), null, p(out_d), p(out_i), null) == -1
    assert lib.gspn_nearest_point(0, 1, 1, null, null, null, null, null, null) == 0 and lib.gspn_nearest_point(1, 0, 0, null, null, null, null, null, null) == 0
    torch.cuda.synchronize()
    assert bool((out_d == 7).all()) and bool((out_i == 7).all())                 # nothing was launched
    q, known = torch.rand(1, 10, 3, device="cuda"), torch.rand(1, 100, 3, device="cuda")
    need = int(lib.gspn_nearest_point_ws_bytes(1, 100))
    with pytest.raises(ValueError, match="at least %d bytes" % need):
        nearest_point(q, known, torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        nearest_point(q, known, torch.empty(need, dtype=torch.float32, device="cuda"))
    d, i = nearest_point(q[:, :0], known)
    assert tuple(d.shape) == tuple(i.shape) == (1, 0)


@pytest.mark.parametrize("v,n,s", [(70000, 18000, 256), (300, 9000, 3)])
def test_vertex_tables_by_nearest_point_equal_the_three_nn_route(v, n, s):
    from gspn_amd import lift
    pc = synth.cloud_s(n, 40)
    verts = torch.from_numpy(synth.scan_vertices(pc, np.zeros(n, np.int32), np.zeros(n, np.int32), n + v, 6)[0][n:].copy()).cuda()
    pc = torch.from_numpy(pc).cuda()
    seeds, fb = pc[torch.randperm(n, generator=torch.Generator().manual_seed(1))[:s].cuda()].contiguous(), torch.rand(s, 2).cuda()
    assert n > lift.NEAREST_FROM_M
    routes = {k: lift.vertex_tables(verts, pc, seeds, fb, search=k) for k in (None, "three_nn", "nearest_point")}
    for k in (None, "nearest_point"):
        assert torch.equal(routes[k][0], routes["three_nn"][0]) and torch.equal(routes[k][1].view(torch.int32), routes["three_nn"][1].view(torch.int32))
    assert routes[None][0].dtype == torch.int32 and tuple(routes[None][0].shape) == tuple(routes[None][1].shape) == (v,)
    with pytest.raises(ValueError, match="search must be one of"):
        lift.vertex_tables(verts, pc, seeds, fb, search="kd_tree")
