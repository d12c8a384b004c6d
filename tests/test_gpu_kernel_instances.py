"""The geometry and detection kernel instantiations a launcher selects from a shape threshold, each ALONE at the smallest shape that selects it,
against the reference the suite already uses for that operation (profiles/kernel_coverage_geometry.txt records which instantiation each
group of cases reaches; tools/kernel_coverage.py measures it from a kernel trace of this suite).

  crop_linear      csrc/heads.hip, cl_lanes(cout): every lane count 2 ... 64, partly dead lane groups (cout < 4 L), the second tile of a
                   workgroup in the backward (more than CL_MAX_PARTS tiles), T wider than the layer, clamped indices -- float64
                   tests/heads_ref.crop_linear, the bound of tests/test_gpu_heads.py (1e-5 of the largest reference value)
  three_nn_nested  csrc/threenn_nested.hip: 1, 2, 3, 4, 5 and 8 levels -- bits of per-level three_nn and of the C oracle
  three_nn         csrc/interpolate.hip, the cell-grid kernel at 8 / 16 / 32 known points per thread and the fall-back above NNG_MAX_M -- bits
                   of the C oracle
  box_point_count  csrc/roi.hip: eight boxes per workgroup from b * ceil(s / 8) >= 256 -- bits of tests/roi_ref.box_point_count
  nn_distance      csrc/nndistance.hip: two queries per lane from b * ceil(n / 512) >= 1024 -- bits of the C oracle, gradients as
                   tests/test_gpu_geometry.py::test_nn_distance_and_grad
  inverse_lists    csrc/grouping.hip: csr_count / csr_scan / csr_fill above CSR_LDS_MAX_N values, which the kernel trace of the suite showed
                   no test to reach -- a stable sort of the valid positions

Every test states the launcher's threshold as an assertion on its own shape: a later change of the constant fails here instead of
silently losing the path."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import data as D
from tests import heads_ref as HR
from tests import roi_ref as RR
from tests.test_gpu_heads import rel_err, run_crop_linear
from tests.test_gpu_roi import count_case

pytestmark = pytest.mark.gpu

BOUND = 1e-5                       # tests/test_gpu_heads.py: crop_linear and its gradients against float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- crop_linear ---------------------------------------------------------------------------------------------------------------------

CL_TILE, CL_MAX_PARTS = 128, 512   # csrc/heads.hip


def cl_lanes(cout):
    """csrc/heads.hip: the smallest power of two that covers cout / 4 float4 columns"""
    lanes = 1
    while lanes * 4 < cout:
        lanes *= 2
    return lanes


def check_crop_linear(shape, normalize, what):
    """forward and the four gradients of crop_linear against float64 (the bodies of test_crop_linear_forward_against_float64 and
    test_crop_linear_gradients_against_float64), the errors printed, then asserted against BOUND"""
    b, n, c, r, p, cout = shape
    case = HR.crop_linear_case(*shape, seed=2)
    dy = torch.randn(b, r, p, cout, generator=torch.Generator().manual_seed(7))
    y, got = run_crop_linear(case, normalize, dy)
    pc, fea, cen, rois, idx, w, bias = [t.double() if t.is_floating_point() else t for t in case]
    leaves = [t.requires_grad_(True) for t in (fea, cen, w, bias)]
    want = HR.crop_linear(pc, leaves[0], leaves[1], rois, idx, leaves[2], leaves[3], normalize)
    (want * dy.double()).sum().backward()
    assert y.shape == (b, r, p, cout) and y.dtype == torch.float32 and got[2].shape == (c + 6, cout)
    errs = {"forward": rel_err(y, want)}
    for name, g, leaf in zip(("pc_fea", "pc_center", "weights", "biases"), got, leaves):
        assert g.shape == leaf.grad.shape, name
        errs[name] = rel_err(g, leaf.grad)
    errs["side rows"] = rel_err(got[2][c:], leaves[2].grad[c:])                     # the six side rows on their own scale
    print("crop_linear %s %s normalize=%s: %s (of %.0e)" % (what, shape, normalize, "  ".join("%s %.3g" % kv for kv in errs.items()), BOUND))
    for name, err in errs.items():
        assert err <= BOUND, name
    _, again = run_crop_linear(case, normalize, dy)
    for g, h in zip(got, again):
        assert torch.equal(g, h)                                                   # two backward calls give identical bits


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("cout,lanes", [(8, 2), (12, 4), (16, 4), (20, 8), (32, 8), (36, 16), (72, 32), (132, 64), (200, 64), (256, 64)])
def test_crop_linear_every_lane_count_and_dead_lanes(cout, lanes, normalize):
    """crop_linear_fwd_kernel<L> / crop_linear_bwd_side_kernel<L> at every L the heads' tests leave out (2, 4, 8, 64), and at each L >= 4 a
    cout below 4 L: lanes with col >= cout are dead inside the __shfl_xor tree and leave zero rows of red[]"""
    assert cl_lanes(cout) == lanes and lanes * 4 >= cout and (lanes // 2) * 4 < cout
    assert cout in (8, 16, 32, 256) or cout < 4 * lanes                            # the others have dead lanes in every row group
    check_crop_linear((2, 50, 8, 3, 33, cout), normalize, "L=%d" % lanes)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("r,p,cout", [(130, 256, 4), (130, 256, 12), (130, 257, 12)])
def test_crop_linear_backward_second_tile_of_a_workgroup(r, p, cout, normalize):
    """more tiles than CL_MAX_PARTS workgroups: the backward's `for (t = blockIdx.x; t < tiles; t += gridDim.x)` takes a second trip in the
    first tiles - 512 workgroups (8 of them at 130 x 256; at 130 x 257 11 of them, and the last tile has 4 rows)"""
    from gspn_amd import _lib as L
    b = 2
    rows = b * r * p
    tiles = (rows + CL_TILE - 1) // CL_TILE
    assert rows > CL_MAX_PARTS * CL_TILE and CL_MAX_PARTS < tiles < 2 * CL_MAX_PARTS
    assert int(L.lib().gspn_crop_linear_part_floats(b, r, p, cout)) == CL_MAX_PARTS * 7 * cout      # the grid IS capped at CL_MAX_PARTS
    assert (rows % CL_TILE != 0) == (p == 257)
    check_crop_linear((b, 64, 4, r, p, cout), normalize, "%d rows, %d tiles" % (rows, tiles))


def side_case(cout, seed):
    """the operands of the two entry points of csrc/heads.hip, called without the Python wrapper"""
    b, n, r, p = 2, 50, 3, 33
    pc, _, cen, rois, idx, w, bias = HR.crop_linear_case(b, n, 0, r, p, cout, seed=seed)
    return b, n, r, p, pc, cen, rois, idx, w.contiguous(), bias


def call_fwd(b, n, r, p, cout, T, ldt, idx, pc, cen, rois, normalize, wside, bias):
    from gspn_amd import _lib as L
    y = torch.full((b, r, p, cout), float("nan"), device="cuda")
    L.check(L.lib().gspn_crop_linear_fwd(b, n, r, p, cout, L.ptr(T), ldt, L.ptr(idx), L.ptr(pc), L.ptr(cen), L.ptr(rois), int(normalize),
                                         L.ptr(wside), L.ptr(bias), L.ptr(y), L.stream()), "crop_linear")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("normalize", [True, False])
def test_crop_linear_forward_on_a_column_slice_of_a_wider_t(normalize):
    """ldt > cout: T is columns 8 ... 27 of a 48-column tensor (32 bytes into each row: 16-byte aligned), the other columns NaN"""
    cout, ldt, col0 = 20, 48, 8
    b, n, r, p, pc, cen, rois, idx, wside, bias = side_case(cout, seed=5)
    wide = torch.full((b * n, ldt), float("nan"))
    t = torch.randn(b * n, cout, generator=torch.Generator().manual_seed(9))
    wide[:, col0:col0 + cout] = t
    wide_d = wide.cuda()
    T = wide_d[:, col0:]
    assert ldt > cout and T.data_ptr() % 16 == 0 and T.data_ptr() != wide_d.data_ptr() and cl_lanes(cout) * 4 > cout
    y = call_fwd(b, n, r, p, cout, T, ldt, idx.cuda(), pc.cuda(), cen.cuda(), rois.cuda(), normalize, wside.cuda(), bias.cuda())
    # T as the feature tensor of a layer whose feature weights are the identity
    want = HR.crop_linear(pc.double(), t.double().reshape(b, n, cout), cen.double(), rois.double(), idx,
                          torch.cat((torch.eye(cout, dtype=torch.float64), wside.double())), bias.double(), normalize)
    err = rel_err(y, want)
    print("crop_linear ldt %d > cout %d normalize=%s: relative error %.3g (of %.0e)" % (ldt, cout, normalize, err, BOUND))
    assert err <= BOUND


@pytest.mark.parametrize("normalize", [True, False])
def test_crop_linear_clamps_indices_outside_the_cloud(normalize):
    """indices of -1 and n (and further out) are read as 0 and n - 1 by both kernels: forward, dWside, dbias and the per-row centre gradient
    against float64 on the clamped indices.  (The two entry points directly: the inverse lists of the wrapper's gather gradients are not
    defined for such an index.)"""
    from gspn_amd import _lib as L
    cout = 20
    b, n, r, p, pc, cen, rois, idx, wside, bias = side_case(cout, seed=6)
    g = torch.Generator().manual_seed(3)
    idx = idx.clone()
    idx[:, 1, ::4] = -1
    idx[:, 1, 1::4] = n
    idx[:, 2, ::5] = n + 7
    idx[:, 0, 2] = -(2 ** 31)
    idx[:, 0, 3] = 2 ** 31 - 1
    clamped = idx.clamp(0, n - 1)
    assert int((idx < 0).sum()) > 0 and int((idx >= n).sum()) > 0 and not torch.equal(idx, clamped)
    t = torch.randn(b * n, cout, generator=g)
    dy = torch.randn(b, r, p, cout, generator=g)
    lib = L.lib()
    dev_ = [x.cuda() for x in (idx, pc, cen, rois, wside, bias, t, dy)]
    idx_d, pc_d, cen_d, rois_d, w_d, bias_d, t_d, dy_d = dev_
    y = call_fwd(b, n, r, p, cout, t_d, cout, idx_d, pc_d, cen_d, rois_d, normalize, w_d, bias_d)
    dw = torch.full((6, cout), float("nan"), device="cuda")
    db = torch.full((cout,), float("nan"), device="cuda")
    drows = torch.full((b, r, p, 4), float("nan"), device="cuda")
    part = torch.empty(int(lib.gspn_crop_linear_part_floats(b, r, p, cout)), device="cuda")
    L.check(lib.gspn_crop_linear_bwd_side(b, n, r, p, cout, L.ptr(dy_d), L.ptr(idx_d), L.ptr(pc_d), L.ptr(cen_d), L.ptr(rois_d), int(normalize),
                                          L.ptr(w_d), L.ptr(part), L.ptr(dw), L.ptr(db), L.ptr(drows), L.stream()), "crop_linear(grad)")
    torch.cuda.synchronize()
    # float64 on the clamped indices; the gathered centre rows as a leaf of their own give the per-row gradient
    rows = HR.crop_rows(pc.double(), torch.zeros(b, n, 1, dtype=torch.float64), cen.double(), rois.double(), clamped, normalize)[..., 1:]
    centre_n = rows[..., :3].clone().requires_grad_(True)
    w64, b64 = wside.double().requires_grad_(True), bias.double().requires_grad_(True)
    tg = torch.gather(t.double().reshape(b, n, cout), 1, clamped.reshape(b, r * p, 1).long().expand(-1, -1, cout)).reshape(b, r, p, cout)
    want = tg + torch.cat((centre_n, rows[..., 3:]), -1) @ w64 + b64
    (want * dy.double()).sum().backward()
    size = rois.double()[:, :, 3:]
    if normalize:
        size = size + (rois.double().sum(2, keepdim=True) == 0).double()
    else:
        size = torch.ones_like(size)
    want_rows = centre_n.grad / size.unsqueeze(2)                                   # d / d pc_center[idx]: centre_n = (centre - c) / size
    errs = {"forward": rel_err(y, want), "dWside": rel_err(dw, w64.grad), "dbias": rel_err(db, b64.grad),
            "centre rows": rel_err(drows[..., :3], want_rows)}
    print("crop_linear clamped indices normalize=%s: %s (of %.0e)" % (normalize, "  ".join("%s %.3g" % kv for kv in errs.items()), BOUND))
    assert not drows[..., 3].any()
    for name, err in errs.items():
        assert err <= BOUND, name


# ---- three_nn_nested -------------------------------------------------------------------------------------------------------------------

def tie_cloud(kind, b, n, seed0):
    if kind == "T":            # exact ties: coordinates on a coarse grid, many duplicates (tests/test_gpu_spn_trunks.py)
        return (np.floor(D.batch("U", b, n, seed0) * 6.0) / 4.0).astype(np.float32)
    return D.batch(kind, b, n, seed0)


NESTED = [  # kernel's LM, level sizes (level 1 first: m), kind, b, n, ordered
    (1, (1,), "U", 2, 1, False), (1, (3,), "T", 2, 63, True), (1, (1000,), "S", 2, 700, False),
    (2, (2, 1), "U", 3, 63, False), (2, (100, 2), "T", 2, 700, True), (2, (1000, 100), "S", 2, 63, False),
    (4, (100, 40, 7), "D", 2, 63, True), (4, (1000, 300, 50), "T", 2, 700, False),
    (4, (3, 3, 2, 1), "U", 2, 1, False), (4, (1000, 256, 64, 16), "T", 2, 700, True),
    (8, (100, 64, 16, 4, 3), "T", 2, 63, False), (8, (1000, 500, 100, 20, 3), "S", 2, 700, True),
    (8, (2048, 1024, 512, 128, 32, 8, 2, 1), "T", 2, 700, True), (8, (1000, 999, 512, 511, 100, 3, 2, 2), "D", 2, 63, False),
    (8, (2, 2, 2, 2, 1, 1, 1, 1), "U", 2, 63, False),
]


@pytest.mark.parametrize("lm,sizes,kind,b,n,ordered", NESTED)
def test_three_nn_nested_every_level_count(lm, sizes, kind, b, n, ordered):
    """three_nn_nested_kernel<1|2|4|8> over chains of random subsets (level l + 1 a random subset of level l), known clouds that are not
    a multiple of the 512-point LDS tile or of the 8-candidate batch, levels of fewer than three points (+inf slots), queries ON known
    points in the "T" kind: bits of per-level three_nn and of the C oracle, as test_three_nn_nested_matches_per_level_and_oracle"""
    from gspn_amd.tf_interpolate import MAX_NESTED_LEVELS, nested_members, three_nn, three_nn_nested
    nl, m = len(sizes), sizes[0]
    assert nl <= MAX_NESTED_LEVELS == 8 and next(x for x in (1, 2, 4, 8) if nl <= x) == lm      # gspn_threenn_nested: L <= 1, <= 2, <= 4, else 8
    l1 = tie_cloud(kind, b, m, seed0=11)
    q = tie_cloud(kind, b, n, seed0=23)
    if kind == "T":
        k = min(n, m, 40)
        q[:, :k] = l1[:, :k]                                                       # queries ON known points: distance-0 ties
    g = torch.Generator().manual_seed(n + b + nl)
    chain = [torch.stack([torch.randperm(sizes[i], generator=g)[:sizes[i + 1]] for _ in range(b)]).int().cuda() for i in range(nl - 1)]
    members = [torch.arange(m, device="cuda").expand(b, -1)] + nested_members(chain)
    local = torch.full((nl, b, m), -1, dtype=torch.int32, device="cuda")
    for lvl, mem in enumerate(members):
        local[lvl].scatter_(1, mem, torch.arange(mem.shape[1], dtype=torch.int32, device="cuda").expand(b, -1).contiguous())
    tq, tl1 = dev(q), dev(l1)
    order = torch.stack([torch.randperm(n, generator=g) for _ in range(b)]).int().cuda() if ordered else None
    dist, idx = three_nn_nested(tq, tl1, local, order=order)
    assert tuple(dist.shape) == (nl, b, n, 3) and idx.dtype == torch.int32
    short = False
    for lvl, mem in enumerate(members):
        known = torch.gather(tl1, 1, mem.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        d_ref, i_ref = three_nn(tq, known)
        assert torch.equal(dist[lvl].view(torch.int32), d_ref.view(torch.int32)), lvl       # bits, +inf of the short levels included
        assert torch.equal(idx[lvl], i_ref), lvl
        od, oi = O.three_nn(q, known.cpu().numpy())
        np.testing.assert_array_equal(dist[lvl].cpu().numpy().view(np.int32), od.view(np.int32))
        np.testing.assert_array_equal(idx[lvl].cpu().numpy(), oi)
        if mem.shape[1] < 3:
            short = True
            assert np.isinf(od[..., mem.shape[1]:]).all() and not oi[..., mem.shape[1]:].any()
    assert short == (min(sizes) < 3)
    if kind == "T":
        od, _ = O.three_nn(q, l1)
        assert (od[..., 0] == 0).any() and (m < 100 or (od[..., 0] == od[..., 1]).any())    # ties occur


# ---- three_nn: the cell grid -------------------------------------------------------------------------------------------------------------

NNG_T, NNG_MAX_M = 256, 8192       # csrc/interpolate.hip


GRID_CASES = [(kind, m, ppt) for m, ppt in [(2048, 8), (2049, 16), (4096, 16), (4097, 32), (6000, 32), (8192, 32), (8193, 0)] for kind in ("U", "lattice")]
GRID_CASES.append(("duplicates", 8192, 32))


@pytest.mark.parametrize("kind,m,ppt", GRID_CASES)
def test_three_nn_cell_grid_every_points_per_thread(kind, m, ppt):
    """three_nn_grid_kernel<8|16|32> at both sides of m = 8 * NNG_T, 16 * NNG_T and NNG_MAX_M (8193: three_nn_kernel): indices and distances
    bit for bit against the C oracle and independent of the scan order, on a uniform cloud and on a random m-point subset of a 21^3
    integer lattice (ties everywhere); at 8192 also with every point twice"""
    from gspn_amd.tf_interpolate import three_nn
    dup = kind == "duplicates"
    assert ppt == (8 if m <= 8 * NNG_T else 16 if m <= 16 * NNG_T else 32 if m <= NNG_MAX_M else 0)     # launch_three_nn_grid / nn_grid_ok
    rng = np.random.default_rng(31 + m)
    b, n = 2, 700
    if kind == "lattice":
        g = np.stack(np.meshgrid(np.arange(21), np.arange(21), np.arange(21), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)     # 9261 points
        assert len(g) >= m
        sparse = np.stack([g[rng.permutation(len(g))[:m]] for _ in range(b)])
        dense = rng.integers(-2, 23, size=(b, n, 3)).astype(np.float32)
        dense[:, ::3] += 0.5                                                  # some queries on cell faces / between lattice points
    elif dup:
        sparse = D.batch("D", b, m, 40)
        sparse[:, m // 2:] = sparse[:, :m // 2]                               # every point twice: each nearest neighbour is a tie
        dense = D.batch("U", b, n, 41)
    else:
        sparse = D.batch("U", b, m, 50)
        dense = D.batch("U", b, n, 51)
    rd, ri = O.three_nn(dense, sparse)
    if kind == "lattice":
        assert (rd[..., 0] == rd[..., 1]).any() and (rd[..., 1] == rd[..., 2]).any()         # ties occur: the lower index must win them
    if dup:
        assert (rd[..., 0] == rd[..., 1]).all() and (ri[..., 0] < m // 2).all()             # every nearest neighbour is a tie
    d, i = three_nn(dev(dense), dev(sparse))
    np.testing.assert_array_equal(i.cpu().numpy(), ri)
    np.testing.assert_array_equal(d.cpu().numpy(), rd)
    perm = np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int32)
    d2, i2 = three_nn(dev(dense), dev(sparse), order=dev(perm))                # the result never depends on the scan order
    assert torch.equal(i2, i) and torch.equal(d2, d)


# ---- box_point_count ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("margin", [0.0, 1e-3])
@pytest.mark.parametrize("b,s,n,nb", [(2, 1020, 500, 8), (2, 1024, 500, 8), (3, 683, 300, 8), (1, 2041, 200, 8), (3, 680, 300, 4)])
def test_box_point_count_eight_boxes_per_workgroup(b, s, n, nb, margin):
    """box_point_count_kernel<8> from b * ceil(s / 8) >= 256, with s a multiple of 8 and not (the boxes past s of the last chunk are counted
    on a clamped index and not written), and <4> one workgroup below the threshold: bit equal to tests/roi_ref.box_point_count"""
    from gspn_amd.rpointnet import box_point_count
    assert (b * ((s + 7) // 8) >= 256) == (nb == 8)                                # gspn_box_point_count
    assert nb == 4 or b * ((s + 7) // 8) <= 258
    box, pc = count_case(b, s, n, 3 * s + n, margin)
    assert not box[:, 1].any() and not box[:, 2].any() and not box[:, s - 1].any()             # the all-zero padding boxes
    got = box_point_count(box.cuda(), pc.cuda(), margin)
    want = RR.box_point_count(box, pc, margin)
    assert got.dtype == torch.int32 and got.shape == (b, s)
    assert torch.equal(got.cpu(), want)
    assert (want[:, 0] == 0).all() and (want[:, 3] == 1).all()            # the point on the face is inside, its neighbour is not
    assert int((want[:, 4:] > 0).sum()) > s // 4 and int((want[:, 4:] == 0).sum()) > 0


# ---- nn_distance -------------------------------------------------------------------------------------------------------------------------

NM_BLOCK, NM_TILE = 256, 1024      # csrc/nndistance.hip


def nm_queries_per_lane(b, nq):
    return 2 if b * ((nq + 2 * NM_BLOCK - 1) // (2 * NM_BLOCK)) >= 1024 else 1               # gspn_nmdistance


@pytest.mark.parametrize("b,n,m,q1,q2,dup", [(1024, 37, 1100, 2, 2, False), (512, 700, 40, 2, 1, False), (1024, 513, 3, 2, 2, True),
                                             (342, 1025, 1025, 2, 2, False)])
def test_nn_distance_two_queries_per_lane(b, n, m, q1, q2, dup):
    """nm_distance_kernel<2> with a ragged slab (the second query of a lane past n), more than one slab per cloud and a second LDS tile of
    candidates (m > NM_TILE), none of which the 2048 x (512, 512) full-size case has: indices and distances of ALL clouds bit for bit
    against the C oracle in both directions, gradients as test_nn_distance_and_grad.  dup: a duplicated candidate and duplicated queries'
    targets, so the lowest index must win"""
    from gspn_amd.tf_nndistance import nn_distance
    assert nm_queries_per_lane(b, n) == q1 == 2 and nm_queries_per_lane(b, m) == q2
    assert b * ((n + 2 * NM_BLOCK - 1) // (2 * NM_BLOCK)) in (1024, 1026, 2048)                # at the threshold, or just past it
    assert n % (2 * NM_BLOCK) != 0                                                           # a ragged last slab in the first direction
    rng = np.random.default_rng(b + n + m)
    a = rng.random((b, n, 3), dtype=np.float32)
    c = rng.random((b, m, 3), dtype=np.float32)
    k = max(1, n // 10)
    a[:, n - k:] = a[:, :k]                                                                  # duplicates inside a cloud ("D" of tests/data.py)
    if dup:
        c[:, 2] = c[:, 0]                                                                    # candidates 0 and 2 tie for every query
    else:
        kc = max(1, m // 10)
        c[:, m - kc:] = c[:, :kc]
    O.set_mt(True)                                                                           # (the oracle over all cores: same bits)
    try:
        rd1, ri1, rd2, ri2 = O.nn_distance(a, c)
    finally:
        O.set_mt(False)
    if dup:
        assert (ri1 == 0).any() and not (ri1 == 2).any()                                     # a tie occurs, and the lower index wins it
    assert (ri2 < n - k).all() and (ri2 < k).any()                                           # the same in the other direction: a[n - k + i] == a[i]
    ta, tc = dev(a).requires_grad_(True), dev(c).requires_grad_(True)
    d1, i1, d2, i2 = nn_distance(ta, tc)
    np.testing.assert_array_equal(i1.cpu().numpy(), ri1)
    np.testing.assert_array_equal(i2.cpu().numpy(), ri2)
    np.testing.assert_array_equal(d1.detach().cpu().numpy(), rd1)
    np.testing.assert_array_equal(d2.detach().cpu().numpy(), rd2)
    g1 = rng.standard_normal(rd1.shape).astype(np.float32)
    g2 = rng.standard_normal(rd2.shape).astype(np.float32)
    (d1 * dev(g1)).sum().add((d2 * dev(g2)).sum()).backward()
    rg1, rg2 = O.nn_distance_grad(a, c, g1, ri1, g2, ri2)
    np.testing.assert_allclose(ta.grad.cpu().numpy(), rg1, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(tc.grad.cpu().numpy(), rg2, rtol=1e-5, atol=1e-5)


# ---- inverse lists -----------------------------------------------------------------------------------------------------------------------

CSR_LDS_MAX_N = 32768              # csrc/grouping.hip


@pytest.mark.parametrize("b,ln,n,lds", [(2, 5000, 32769, False), (3, 2049, 40001, False), (1, 5000, 32768, True)])
def test_inverse_lists_beyond_the_lds_histogram(b, ln, n, lds):
    """csr_count / csr_scan / csr_fill (global atomics) take over from the one-workgroup LDS build above CSR_LDS_MAX_N values -- a size no
    other test reaches: a value count that is not a multiple of the scan's 1024, crowded values (groups longer than a wave), dropped
    positions, against a stable sort of the valid positions as test_inverse_lists_spread_over_position_slices_with_dropped_positions"""
    from gspn_amd.geometry import inverse_lists
    assert (n <= CSR_LDS_MAX_N) == lds                                              # gspn_inverse_lists: n <= CSR_LDS_MAX_N takes the LDS kernel
    assert lds or n % 1024 != 0
    g = torch.Generator().manual_seed(ln * 7 + n)
    idx = torch.randint(0, n, (b, ln), generator=g, dtype=torch.int32)
    idx[:, : ln // 3] = idx[:, : ln // 3] % 3 + (n - 3)                             # a few crowded values at the very end of the scan
    bad = torch.rand(b, ln, generator=g) < 0.07
    idx[bad] = torch.where(torch.rand(int(bad.sum()), generator=g) < 0.5, torch.tensor(-1, dtype=torch.int32), torch.tensor(n + 5, dtype=torch.int32))
    order, offsets = inverse_lists(idx.cuda(), n)
    order, offsets = order.cpu().long(), offsets.cpu().long()
    for s_ in range(b):
        valid = (idx[s_] >= 0) & (idx[s_] < n)
        pos = torch.nonzero(valid).squeeze(1)
        keys, perm = torch.sort(idx[s_][valid].long(), stable=True)
        nv = int(valid.sum())
        assert 0 < nv < ln and int(offsets[s_, n]) == nv
        assert int((offsets[s_, 1:] - offsets[s_, :-1]).max()) > 64                  # a group longer than a wave: the radix sort
        assert torch.equal(order[s_, :nv], pos[perm])
        assert torch.equal(offsets[s_], torch.searchsorted(keys.contiguous(), torch.arange(n + 1)))
