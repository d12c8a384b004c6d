"""query_ball_point past the 8192-point prefix on ragged sizes, planted boundary hits and degenerate cell-grid geometry.

Clouds of more than 8192 points run on three cooperating kernels (grouping.hip): ball_query_kernel scans the first 8192 points,
ball_query_cont_kernel resumes the open queries in steps of 512 points (4 per lane and 256-point chunk; three 16-byte loads when the scene
starts on a 16-byte boundary, guarded scalar loads otherwise and within the last 3 points), ball_grid_build_kernel / ball_grid_query_kernel
answer sparse queries through a cell grid and mark them `resolved`.  The rest of the suite runs them at n in {16384, 32768, 65536} only:
no ragged last step, no scene off a 16-byte boundary, no hit planted at a boundary, one constructed cloud for the grid.

Every case here goes through three entries that must agree with the oracle (pts_cnt, and every row that has a hit; rows without a hit
are all zero here and unspecified in the reference) and so with each other:
  (a) gspn_amd.tf_grouping.query_ball_point -- the wrapper, which takes gspn_queryballpoint_ws for n >= 8192 and nsample <= 256;
  (b) gspn_queryballpoint through ctypes -- no workspace: the prefix and the continuation do all the work;
  (c) gspn_queryballpoint_ws through ctypes with a workspace this file allocates, and reads back to see what the grid decided.

Workspace layout (grouping.hip:241-245, BallGridHdr / bqg_scene_bytes): b scene blocks of scene_bytes = gspn_ball_ws_bytes(1, n, 0) bytes
each, a block starting with the 64-byte header {float lo[3] @0; float inv[3] @12; int G[3] @24; int use @36; pad}; the (b, m) `resolved`
bytes follow the b scene blocks, at b * scene_bytes.  _run_ws asserts gspn_ball_ws_bytes(b, n, m) == b * scene_bytes + ceil16(b * m), so
a layout change fails there and cannot blind the checks on `use` and `resolved`.

GSPN_BALL_CELLS and GSPN_BALL_PREFIX are read once per process and must be at their defaults (unset) when this file runs."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import data as D

pytestmark = pytest.mark.gpu

PREFIX = 8192            # ball_query_kernel's share of the cloud (ball_query_impl: n_scan)
STEP = 512               # points per step of ball_query_cont_kernel, two chunks of 256, 4 consecutive points per lane and chunk
BQG_CAP = 256            # hits the grid kernel sorts
BQG_MAXCAND = 2048       # candidates of a 3 x 3 x 3 block the grid kernel is willing to test
F = ctypes.c_float
SENTINEL = -7            # what idx / pts_cnt hold before entries (b) and (c): a slot no kernel wrote shows


def _oracle(radius, ns, xyz, q):
    """(idx, cnt, open) -- open[s, j]: fewer than ns hits among the first PREFIX points, read from the oracle's rows and cross-checked
    with its `visited` (index of the ns-th hit + 1, else n)"""
    ridx, rcnt, vis = O.query_ball_point(radius, ns, xyz, q, mt=True, return_visited=True)
    valid = np.arange(ns)[None, None, :] < rcnt[..., None]
    below = ((ridx < PREFIX) & valid).sum(-1)
    opened = below < ns
    if xyz.shape[1] > PREFIX:
        np.testing.assert_array_equal(opened, vis > PREFIX)
    return ridx, rcnt, opened


def _compare(what, idx, cnt, ridx, rcnt):
    np.testing.assert_array_equal(cnt, rcnt, err_msg=what + ": pts_cnt")
    hit = rcnt > 0
    np.testing.assert_array_equal(idx[hit], ridx[hit], err_msg=what + ": rows with a hit")
    assert (idx[~hit] == 0).all(), what + ": a row without a hit is not all zero"


def _run_wrapper(radius, ns, t, tq):
    from gspn_amd.tf_grouping import query_ball_point
    idx, cnt = query_ball_point(radius, ns, t, tq)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), cnt.cpu().numpy()


def _outputs(b, m, ns):
    return (torch.full((b, m, ns), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((b, m), SENTINEL, dtype=torch.int32, device="cuda"))


def _run_plain(radius, ns, t, tq):
    from gspn_amd import _lib as L
    b, n, _ = t.shape
    m = tq.shape[1]
    idx, cnt = _outputs(b, m, ns)
    assert L.lib().gspn_queryballpoint(b, n, m, F(radius), ns, L.ptr(t), L.ptr(tq), L.ptr(idx), L.ptr(cnt), L.stream()) == 0
    torch.cuda.synchronize()
    return idx.cpu().numpy(), cnt.cpu().numpy()


def _run_ws(radius, ns, t, tq):
    """-> idx, cnt, hdr -- hdr None when the grid cannot run (nsample > BQG_CAP), else a dict of per-scene lo, inv, G, use and the (b, m)
    resolved bytes"""
    from gspn_amd import _lib as L
    b, n, _ = t.shape
    m = tq.shape[1]
    scene_bytes = int(L.lib().gspn_ball_ws_bytes(1, n, 0))
    total = int(L.lib().gspn_ball_ws_bytes(b, n, m))
    assert scene_bytes > 64 + 16 * n and scene_bytes % 16 == 0
    assert total == b * scene_bytes + (b * m + 15) // 16 * 16                 # the layout this function reads back
    ws = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")           # (the wrapper hands over uninitialised memory)
    assert ws.data_ptr() % 16 == 0
    idx, cnt = _outputs(b, m, ns)
    assert L.lib().gspn_queryballpoint_ws(b, n, m, F(radius), ns, L.ptr(t), L.ptr(tq), L.ptr(ws), L.ptr(idx), L.ptr(cnt), L.stream()) == 0
    torch.cuda.synchronize()
    hdr = None
    if ns <= BQG_CAP:
        raw = ws.cpu().numpy()
        heads = np.stack([raw[s * scene_bytes:s * scene_bytes + 40] for s in range(b)])
        hdr = {"lo": heads[:, 0:12].copy().view(np.float32), "inv": heads[:, 12:24].copy().view(np.float32),
               "G": heads[:, 24:36].copy().view(np.int32), "use": heads[:, 36:40].copy().view(np.int32)[:, 0],
               "resolved": raw[b * scene_bytes:b * scene_bytes + b * m].reshape(b, m).copy()}
        assert np.isin(hdr["use"], (0, 1)).all() and np.isin(hdr["resolved"], (0, 1)).all()
        assert (hdr["resolved"][hdr["use"] == 0] == 0).all()
    return idx.cpu().numpy(), cnt.cpu().numpy(), hdr


def _three_entries(radius, ns, xyz, q, ref):
    """run (a), (b), (c) on one case, compare each with the oracle's (ridx, rcnt); -> what the grid of entry (c) decided"""
    ridx, rcnt = ref[0], ref[1]
    t, tq = torch.from_numpy(xyz).cuda(), torch.from_numpy(q).cuda()
    got = {"wrapper": _run_wrapper(radius, ns, t, tq), "plain": _run_plain(radius, ns, t, tq)}
    ci, cc, hdr = _run_ws(radius, ns, t, tq)
    got["ws"] = (ci, cc)
    for name, (idx, cnt) in got.items():
        _compare(name, idx, cnt, ridx, rcnt)
    for name in ("plain", "ws"):                                               # identical to the last slot (the zero rows included)
        np.testing.assert_array_equal(got[name][0], got["wrapper"][0], err_msg=name + " vs wrapper")
    return hdr


# ============================================================================================================================================
# 1. ragged sizes on real clouds
# ============================================================================================================================================
RAGGED_N = [8193, 8194, 8195, 8196, 8447, 8448, 8449, 8703, 8704, 8705, 9001, 18000, 18001, 18002, 18003]


KNOT_C = np.array([2.125, 1.96875, 1.5], np.float32)      # "SC": the centre of the knot, mid-cell in x and y (cells of 0.25 x 0.1875 at r = 0.1)


def ragged_case(kind, n):
    """"U" and "S": synth's clouds, the queries 37 of their points.  "SC": the S cloud with its points 4000 .. 6499 pulled into a knot of
    sigma 0.008 (one cell wide), and three of the queries at the knot's centre and 0.15 to either side of it along x.  On "S" itself the grid
    refuses no open query -- a 3 x 3 x 3 block there holds at most 919 points (n = 18000) against BQG_MAXCAND = 2048, and a ball with more
    than BQG_CAP hits has 32 of them among the first 8192 points -- so entry (c) leaves the scan kernels nothing but closed queries.  Beside
    the knot a block holds 2500 candidates and a ball few hits: refused by the grid, and open to the last point."""
    b, m = 3, 37                                                 # m: no multiple of the continuation's 16 queries per workgroup, nor of 4
    xyz = D.batch(kind[0], b, n, 5)
    rng = np.random.default_rng(1000 + n)
    if kind == "SC":
        xyz[:, 4000:6500] = (KNOT_C + 0.008 * rng.standard_normal((b, 2500, 3))).astype(np.float32)
    q = np.ascontiguousarray(np.stack([xyz[s][rng.integers(0, n, size=m)] for s in range(b)]))
    if kind == "SC":
        q[:, 5] = KNOT_C
        q[:, 6] = KNOT_C + np.array([0.15, 0.0, 0.0], np.float32)
        q[:, 22] = KNOT_C - np.array([0.15, 0.0, 0.0], np.float32)
    return xyz, q


@pytest.mark.parametrize("n", RAGGED_N)
@pytest.mark.parametrize("kind,radius", [("U", 0.05), ("S", 0.1), ("SC", 0.1)])
def test_ragged_tail_after_the_prefix(kind, radius, n):
    """b = 3 scenes of n points, n - 8192 no multiple of 512 (a last step of 1 .. 511 points; 18000 = 8192 + 19 * 512 + 80 is the reference's
    own operating point) and for n % 4 != 0 scenes 1 and 2 off a 16-byte boundary: the continuation's scalar fetch path.  On entry (c) the
    grid resolves some queries of "S"; on "SC" it also refuses open ones, which the scan kernels finish beside the resolved ones they skip."""
    ns = 32
    xyz, q = ragged_case(kind, n)
    if n % 4:
        assert (n * 12) % 16 != 0                                # scene 1 starts n * 12 bytes behind a 16-byte boundary
    ref = _oracle(radius, ns, xyz, q)
    ridx, rcnt, opened = ref
    if n >= 9001:                                                # the regime, from the oracle, before anything is compared
        valid = np.arange(ns)[None, None, :] < rcnt[..., None]
        behind = ((ridx >= PREFIX) & valid).any(-1)
        before = ((ridx < PREFIX) & valid).any(-1)
        assert opened.mean() >= 0.3
        assert behind.any()
        assert (behind & before).any()
    hdr = _three_entries(radius, ns, xyz, q, ref)
    if kind != "U" and n >= 9001:
        res = hdr["resolved"].astype(bool)
        assert (hdr["use"] == 1).all() and res.any(), "the grid resolved no query"
        if kind == "SC":                                         # (unreachable on "S": ragged_case)
            assert (opened & ~res).sum(-1).min() >= 2, "every open query was resolved by the grid: the continuation had nothing to do on entry (c)"


# ============================================================================================================================================
# 2. planted hits at the boundaries
# ============================================================================================================================================
PLANT_R = 0.2
LANE = 37                # the lane of set 10's pair: points 8192 + 4 * 37 + {1, 2}, inside that lane's group of four


def planted_sets(n, ns, rng):
    """the 13 sorted index sets of the issue, one query each"""
    reserved = {0, n - 5, n - 4, n - 3, n - 2, n - 1, PREFIX - 1, PREFIX, PREFIX + 255, PREFIX + 256, PREFIX + 511, PREFIX + 512,
                PREFIX + 4 * LANE + 1, PREFIX + 4 * LANE + 2}
    low = rng.permutation(np.array([k for k in range(1, PREFIX - 1) if k not in reserved]))
    closed = sorted(low[:ns].tolist())                                                         # 9: closed by the prefix
    fills = sorted(low[ns:2 * ns - 1].tolist()) + [PREFIX + 4 * LANE + 1, PREFIX + 4 * LANE + 2]   # 10: fills inside one lane's four
    per_step = [[k for k in range(PREFIX + STEP * s, min(n, PREFIX + STEP * (s + 1))) if k not in reserved] for s in range(3)]
    want = [len(part) for part in np.array_split(np.arange(ns + 5), 3)]
    if all(len(p) >= w for p, w in zip(per_step, want)):
        spread = sorted(k for p, w in zip(per_step, want) for k in rng.choice(p, size=w, replace=False).tolist())
    else:                                                                                      # (n = 8705: the tail is one step and a point)
        spread = sorted(rng.choice(sum(per_step, []), size=ns + 5, replace=False).tolist())
    return [[n - 1], [n - 4, n - 3, n - 2, n - 1], [n - 5, n - 1], [PREFIX], [PREFIX - 1], [PREFIX - 1, PREFIX],
            [PREFIX + 255, PREFIX + 256], [PREFIX + 511, PREFIX + 512], [0, n - 1], closed, fills, spread, []]


def planted_layouts(sets):
    """a data point can lie next to one query only: the sets are split greedily into groups of pairwise disjoint ones, and call c gives
    scene s the group (c + s) % len(groups) -- every set is planted once in scene 0 and once in scene 1 (the unaligned one for n % 4 != 0);
    the queries whose set is not planted in a scene have no hit there"""
    groups = []
    for i, st in enumerate(sets):
        for g in groups:
            if all(not (set(st) & set(sets[j])) for j in g):
                g.append(i)
                break
        else:
            groups.append([i])
    return [[groups[(c + s) % len(groups)] for s in range(2)] for c in range(len(groups))]


def planted_case(n, ns, sets, layout, rng):
    """-> xyz (2, n, 3), q (2, 13, 3), the closed-form rows and counts"""
    b, m = 2, len(sets)
    xyz = rng.random((b, n, 3), dtype=np.float32)                # the unit cube: nothing of it within 90 of a query
    q = np.zeros((b, m, 3), np.float32)
    q[:, :, 0] = 100.0 + 10.0 * np.arange(m, dtype=np.float32)
    eidx = np.zeros((b, m, ns), np.int32)
    ecnt = np.zeros((b, m), np.int32)
    for s in range(b):
        for i in layout[s]:
            st = sets[i]
            if not st:
                continue
            xyz[s, st] = q[s, i] + (rng.random((len(st), 3), dtype=np.float32) - 0.5) * np.float32(0.04)      # within 0.035 < r / 4
            row = (st + [st[0]] * ns)[:ns] if len(st) < ns else st[:ns]
            eidx[s, i] = row
            ecnt[s, i] = min(len(st), ns)
    return xyz, q, eidx, ecnt


@pytest.mark.parametrize("ns", [1, 32, 100])
@pytest.mark.parametrize("n", [18000, 18003, 8705])
def test_planted_hits_at_the_boundaries(n, ns):
    """hits planted at index n - 1, either side of 8192, of the 256-point chunk and the 512-point step, a first hit behind the prefix (the
    continuation's c == 0 branch sets `first`), a row that fills inside one lane's group of four (the pos < nsample cut), a query the prefix
    closed, one without a hit: a closed form -- the first nsample planted indices, padded with the first -- and the oracle, both.  Entry
    (b) answers these with the continuation, entries (a) and (c) with the grid (far queries in an elongated box: every one resolved)."""
    rng = np.random.default_rng(n * 1000 + ns)
    sets = planted_sets(n, ns, rng)
    assert len(sets) == 13 and all(st == sorted(set(st)) and (not st or (0 <= st[0] and st[-1] < n)) for st in sets)
    assert len(sets[9]) == ns and sets[9][-1] < PREFIX and len(sets[10]) == ns + 1 and len(sets[11]) == ns + 5 and sets[11][0] >= PREFIX
    if n >= PREFIX + 3 * STEP:
        assert len({(k - PREFIX) // STEP for k in sets[11]}) == 3
    layouts = planted_layouts(sets)
    for s in range(2):
        assert sorted(i for lay in layouts for i in lay[s]) == list(range(13))       # every set once per scene
    for layout in layouts:
        xyz, q, eidx, ecnt = planted_case(n, ns, sets, layout, rng)
        ref = _oracle(PLANT_R, ns, xyz, q)
        np.testing.assert_array_equal(ref[1], ecnt)                                  # the oracle agrees with the closed form
        np.testing.assert_array_equal(ref[0][ecnt > 0], eidx[ecnt > 0])
        hdr = _three_entries(PLANT_R, ns, xyz, q, (eidx, ecnt))
        assert (hdr["use"] == 1).all()
        assert (hdr["resolved"] == 1).all()


# ============================================================================================================================================
# 3. degenerate geometry for the cell grid
# ============================================================================================================================================
GRID_CASES = ["plane", "line", "far_origin", "lattice", "duplicates", "capped", "crowded", "sort_tail", "mixed", "dense", "ns257"]
LATTICE_S = np.float32(0.25)         # lattice spacing = radius: exact in float32, so a neighbour's distance is exactly the radius
CROWD_C = np.array([2.125, 2.17, 0.965], np.float32)       # "crowded": the centre of the 3000-point cluster
CROWD_C2 = np.array([6.0, 4.0, 2.0], np.float32)           # ... and of the 600-point one


def _queries(xyz, rng, m_data=200, m_box=80, m_far=21):
    b, n, _ = xyz.shape
    lo, hi = xyz.min(1, keepdims=True), xyz.max(1, keepdims=True)
    data = np.stack([xyz[s][rng.integers(0, n, size=m_data)] for s in range(b)])
    box = (lo + rng.random((b, m_box, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    d = rng.standard_normal((b, m_far, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    diag = np.linalg.norm(hi - lo, axis=-1, keepdims=True).astype(np.float32)
    far = ((lo + hi) / 2 + d * (np.float32(5.0) * diag + np.float32(1.0))).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([data, box, far], axis=1).astype(np.float32))


def grid_case(case, n):
    """-> xyz (2, n, 3), q (2, 301, 3), radius, nsample"""
    rng = np.random.default_rng(7 * n + GRID_CASES.index(case))
    b, ns = 2, 32
    room = np.array([8.0, 6.0, 3.0], np.float32)
    if case == "plane":
        xyz = rng.random((b, n, 3), dtype=np.float32)
        xyz[..., 2] = 0.25                                       # zero extent along z: G[2] = 1, inv[2] = 0
        radius = 0.03
    elif case == "line":
        xyz = rng.random((b, n, 3), dtype=np.float32)
        xyz[..., 1] = 0.5
        xyz[..., 2] = -0.75
        radius = 0.001
    elif case == "far_origin":
        xyz = (D.batch("S", b, n, 21) + np.array([1000.0, -2000.0, 500.0], np.float32)).astype(np.float32)
        radius = 0.2
    elif case == "lattice":
        # integer sites 0..11 (each held by several points) times the spacing, r = one spacing: the six neighbours of a site are exactly
        # ON the radius and must not hit.  (Cells are at least 1.01 r wide by construction: 10 per axis here, edge 1.1 spacings.)
        xyz = (rng.integers(0, 12, size=(b, n, 3)).astype(np.float32) * LATTICE_S).astype(np.float32)
        radius = float(LATTICE_S)
    elif case == "duplicates":
        half = D.batch("U", b, (n + 1) // 2, 31)
        xyz = np.concatenate([half, half[:, :n // 2]], axis=1)   # every point twice (but one, for odd n)
        radius = 0.08
    elif case == "capped":
        xyz = rng.random((b, n, 3), dtype=np.float32) * room
        xyz[:, n // 2:] = (xyz[:, :n - n // 2] + 0.02 * rng.standard_normal((b, n - n // 2, 3))).astype(np.float32)   # (pairs: balls that hold more than their centre)
        radius = 0.05
    elif case == "crowded":
        # the last 3000 indices: a cluster inside ONE cell (cells of 0.25 x 0.207 x 0.214 at r = 0.2, the centre in the middle of one);
        # the 600 indices before them: a second cluster, more than BQG_CAP hits for a query in it but few candidates
        xyz = rng.random((b, n, 3), dtype=np.float32) * room
        xyz[:, n - 3000:] = (CROWD_C + 0.02 * rng.standard_normal((b, 3000, 3))).astype(np.float32)
        xyz[:, n - 3600:n - 3000] = (CROWD_C2 + 0.02 * rng.standard_normal((b, 600, 3))).astype(np.float32)
        radius = 0.2
    elif case == "sort_tail":
        xyz = D.batch("U", b, n, 61)
        ns = 256
        radius = float((130.0 / (4.18879 * n)) ** (1.0 / 3.0))   # about 130 points in an interior ball
    elif case == "mixed":
        radius = 0.05
        xyz = D.batch("U", 1, n, 71).repeat(2, axis=0)
        xyz[1] *= np.float32(2 * radius)                         # scene 1: the same points in a cube of edge 2 r
    elif case == "dense":
        xyz = D.batch("U", b, n, 81)
        radius = 3.0                                             # larger than the cloud
    else:
        xyz = D.batch("U", b, n, 91)
        ns = 257                                                 # the wrapper takes the no-workspace entry; the grid sorts at most 256
        radius = 0.12
    xyz = np.ascontiguousarray(xyz.astype(np.float32))
    q = _queries(xyz, rng)
    if case == "lattice":
        q[:, 0:200:3, 0] += LATTICE_S / 2                        # between two sites: both at half a spacing
        lo, hi = xyz.min(1), xyz.max(1)
        edge = (hi - lo) / np.float32(10.0)
        q[:, 200:240] = (lo[:, None] + np.round((q[:, 200:240] - lo[:, None]) / edge[:, None]) * edge[:, None]).astype(np.float32)   # on cell faces
    if case == "crowded":
        q[:, 0] = CROWD_C                                        # the centre of the cluster: 3000 candidates, 3000 hits
        q[:, 1] = CROWD_C + np.array([0.3, 0.0, 0.0], np.float32)   # the next cell: the cluster in its block, out of its ball
        q[:, 2] = CROWD_C2                                       # 600 hits among few candidates
    return xyz, q, radius, ns


@pytest.mark.parametrize("n", [PREFIX + 37, 16384])
@pytest.mark.parametrize("case", GRID_CASES)
def test_cell_grid_on_degenerate_geometry(case, n):
    """the ball grid on the geometries the three-NN grid is tested on (test_three_nn_cell_grid_is_exact): a zero-extent axis (inv = 0,
    G = 1), G clamped at 32, coordinates far from the origin, exact ties on the radius, duplicates, a sparse scene beside a dense one,
    65 .. 256 hits (the second rank-sort loop), more than BQG_MAXCAND candidates handed to the scan; queries are 200 data points, 80
    points of the bounding box and 21 far outside it"""
    xyz, q, radius, ns = grid_case(case, n)
    assert xyz.shape == (2, n, 3) and q.shape == (2, 301, 3) and np.isfinite(xyz).all() and np.isfinite(q).all()
    ext = xyz.max(1) - xyz.min(1)
    ref = _oracle(radius, ns, xyz, q)
    ridx, rcnt, _ = ref
    if case == "lattice":
        # a query on a site counts that site's own points, never the six neighbours at exactly one spacing
        sites = np.rint(xyz / LATTICE_S).astype(np.int64)
        for s in range(2):
            for j in (1, 2, 4, 5, 7, 8):
                own = int((sites[s] == np.rint(q[s, j] / LATTICE_S).astype(np.int64)).all(-1).sum())
                assert own > 0 and rcnt[s, j] == min(own, ns)
    if case == "capped":
        assert (ext / (np.float32(1.01) * np.float32(radius)) > 32).all()
    hdr = _three_entries(radius, ns, xyz, q, ref)
    if case == "ns257":
        assert hdr is None
        return
    res = hdr["resolved"].astype(bool)
    if case == "dense":
        assert (hdr["use"] == 0).all()
    elif case == "mixed":
        assert hdr["use"].tolist() == [1, 0]
    else:
        assert (hdr["use"] == 1).all() and res.any()
    if case == "plane":
        assert (hdr["G"][:, 2] == 1).all() and (hdr["inv"][:, 2] == 0).all() and (hdr["G"][:, :2] > 1).all()
    if case == "line":
        assert (hdr["G"][:, 1:] == 1).all() and (hdr["inv"][:, 1:] == 0).all() and (hdr["G"][:, 0] == 32).all()
    if case == "capped":
        assert (hdr["G"] == 32).all()
    if case == "lattice":
        assert (hdr["G"] == 10).all()                            # the cell faces the queries 200 .. 239 were put on
    if case == "crowded":
        # query 0, the centre: more than BQG_MAXCAND candidates (and hits): left to the scan, whose row (compared above) ends in the cluster
        assert (res[:, 0] == 0).all() and (rcnt[:, 0] == ns).all() and (ridx[:, 0, -1] >= n - 3000).all()
        # query 1: the whole cluster within one cell edge (>= 1.01 r) of the centre, so in the block of the next cell -- more than
        # BQG_MAXCAND candidates, but fewer than nsample hits: only the candidate limit can refuse it, and the scan runs to the end for it
        assert (np.abs(xyz[:, n - 3000:] - CROWD_C).max(-1) < 0.09).all()
        assert (res[:, 1] == 0).all() and (rcnt[:, 1] < ns).all()
        # query 2: a block reaches at most two cell edges (<= 0.26 each) from the query -- at most BQG_MAXCAND candidates, more than
        # BQG_CAP of them hits: only the hit limit can refuse it
        for s in range(2):
            d = np.abs(xyz[s] - q[s, 2]).max(-1)
            assert (d <= 0.52).sum() <= BQG_MAXCAND and (d < 0.1).sum() > BQG_CAP
        assert (res[:, 2] == 0).all() and (rcnt[:, 2] == ns).all()
    if case == "sort_tail":
        band = res & (rcnt > 64) & (rcnt <= BQG_CAP)
        assert band.sum() >= 10
