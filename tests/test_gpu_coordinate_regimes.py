"""GPU parity of the geometry kernels off the unit scale (tests/regimes.py): exact power-of-two rescales, metres <-> millimetres, squared
distances that are subnormal or zero, room clouds and a raster placed far from the origin, slabs, lines and tilted planes -- every kernel
path bit for bit against the CPU oracle (or the kernel's restatement under tests/) on the same fp32 inputs.  Under an exact rescale the
result is also held against the ORACLE's at scale 1: same indices and counts, distances exactly d * s^2 (tests/test_cpu_coordinate_regimes.py
shows that identity in the oracle alone; a kernel that breaks it carries a hidden absolute constant).  No tolerance anywhere."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import regimes as R

pytestmark = pytest.mark.gpu

ALL = pytest.mark.parametrize("reg", R.REGIMES, ids=R.ids(R.REGIMES))
BALL = pytest.mark.parametrize("reg", R.BALL_REGIMES, ids=R.ids(R.BALL_REGIMES))
BOX = pytest.mark.parametrize("reg", R.BOX_REGIMES, ids=R.ids(R.BOX_REGIMES))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what):
    """bit for bit: assert_array_equal (which takes -0.0 for 0.0 and no more), on the host"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got, want, err_msg=what)


# ---- farthest point sampling: the five kernels -------------------------------------------------------------------------------------------

def check_fps(reg, kind, n, m, distinct, run, what):
    got = run(m, dev(R.cloud(reg, kind, 2, n, 3, distinct))).cpu().numpy()
    tag = "%s %s kind %s n %d m %d distinct %d" % (what, reg.name, kind, n, m, distinct)
    same(got, R.fps_ref(reg, kind, n, m, distinct), tag)
    if R.exact(reg):
        same(got, R.fps_ref(R.unit_of(reg), kind, n, m, distinct), tag + " (against the oracle at scale 1)")


@ALL
def test_fps_small_kernel(reg):
    from gspn_amd.tf_sampling import farthest_point_sample
    for n, m, distinct in R.FPS_SMALL:
        for kind in R.kinds(reg):
            check_fps(reg, kind, n, m, distinct, farthest_point_sample, "fps_small")


@pytest.mark.parametrize("mode,min_n", [("resident", 0), ("cells", 64), ("cells_torch", 64)])
@ALL
def test_fps_on_chip_kernels(reg, mode, min_n, monkeypatch):
    from gspn_amd import tf_sampling
    monkeypatch.setattr(tf_sampling, "FPS_MODE", mode)
    monkeypatch.setattr(tf_sampling, "FPS_CELLS_MIN_N", min_n)
    for n, m, distinct in R.FPS_ON_CHIP:
        for kind in R.kinds(reg):
            check_fps(reg, kind, n, m, distinct, tf_sampling.farthest_point_sample, mode)


@ALL
def test_fps_cell_kernel_in_its_own_range(reg):
    from gspn_amd import tf_sampling
    assert tf_sampling.FPS_MODE == "cells" and tf_sampling.FPS_CELLS_MIN_N <= 9000
    for n, m, distinct in R.FPS_CELLS_OWN:
        check_fps(reg, reg.kind, n, m, distinct, tf_sampling.farthest_point_sample, "cells")


@pytest.mark.parametrize("G", R.FPS_MULTI_G)
@ALL
def test_fps_multi_cu_kernel(reg, G, monkeypatch):
    from gspn_amd import tf_sampling
    monkeypatch.setattr(tf_sampling, "FPS_MULTI_FORCE", True)
    monkeypatch.setattr(tf_sampling, "FPS_MULTI_G", G)
    for n, m, distinct in R.FPS_ON_CHIP:
        check_fps(reg, reg.kind, n, m, distinct, tf_sampling.farthest_point_sample, "multi G=%d" % G)
    from gspn_amd import _lib as L
    L.check_async(block=True)                                       # the kernel's status word: no bounded wait expired


@ALL
def test_fps_segments_every_size_class(reg):
    """the two labelled scenes of tests/dataset_ref.py (instances in every size class of the segmented kernels), moved by the regime"""
    from gspn_amd import dataset
    from tests import dataset_ref as DR
    from tests.test_gpu_dataset import G, M, N
    both = [DR.labelled_scene(N, DR.SIZES[s], G, 40 + s, False) for s in range(2)]
    label = np.stack([l for _, l in both])
    pc = R.apply(reg, R.shape_map(reg.kind, np.stack([p for p, _ in both])))
    want_idx, want_pts, want_count = DR.instance_sets(pc, label, G, M, 7)
    idx, pts, count = dataset.fps_segments(dev(pc), dev(label), G, M, 7)
    same(count, want_count, "count")
    same(idx, want_idx, "idx")
    same(pts.cpu().numpy().view(np.int32), want_pts.view(np.int32), "pts")
    if R.exact(reg):
        unit = R.apply(R.unit_of(reg), R.shape_map(reg.kind, np.stack([p for p, _ in both])))
        same(idx, DR.instance_sets(unit, label, G, M, 7)[0], "idx (against the oracle at scale 1)")


# ---- ball query --------------------------------------------------------------------------------------------------------------------------

def check_ball(reg, case):
    from gspn_amd.tf_grouping import query_ball_point
    tag, spec, n, m, r0, ns, push = case
    for kind in R.ball_kinds(reg, spec):
        idx, cnt = query_ball_point(R.scaled(reg, r0), ns, dev(R.cloud(reg, kind, 2, n, 4)), dev(R.queries(reg, kind, 2, n, 4, m, push)))
        what = "ball %s %s kind %s n %d nsample %d" % (tag, reg.name, kind, n, ns)
        ridx, rcnt = R.ball_ref(reg, kind, n, m, r0, ns, push)
        same(cnt, rcnt, what)
        same(idx, ridx, what)
        if R.exact(reg):
            uidx, ucnt = R.ball_ref(R.unit_of(reg), kind, n, m, r0, ns, push)
            same(cnt, ucnt, what + " (against the oracle at scale 1)")
            same(idx, uidx, what + " (against the oracle at scale 1)")


@pytest.mark.parametrize("case", R.BALL_CASES, ids=["%s_n%d_ns%d" % (c[0], c[2], c[5]) for c in R.BALL_CASES])
@BALL
def test_ball_query(reg, case):
    check_ball(reg, case)


@pytest.mark.parametrize("case", R.BALL_CASES, ids=["%s_n%d_ns%d" % (c[0], c[2], c[5]) for c in R.BALL_CASES])
def test_ball_query_radius_below_the_reference_s_floor(case):
    """max(sqrtf(d2), 1e-20f) < radius with radius = 0.2 * 2^-70 < 1e-20: not even a query's own point is a hit"""
    from gspn_amd.tf_grouping import query_ball_point
    reg = R.BALL_BELOW_FLOOR
    tag, spec, n, m, r0, ns, push = case
    assert 0 < R.scaled(reg, r0) < R.BALL_FLOOR
    for kind in R.ball_kinds(reg, spec):
        idx, cnt = query_ball_point(R.scaled(reg, r0), ns, dev(R.cloud(reg, kind, 2, n, 4)), dev(R.queries(reg, kind, 2, n, 4, m, push)))
        ridx, rcnt = R.ball_ref(reg, kind, n, m, r0, ns, push)
        assert not rcnt.any() and not ridx.any()
        same(cnt, rcnt, "count")
        same(idx, ridx, "idx")


# ---- three_nn: wave, cell grid, thread per query, nested, ordered ------------------------------------------------------------------------

@pytest.mark.parametrize("m", R.NN_KNOWN)
@ALL
def test_three_nn(reg, m):
    from gspn_amd.tf_interpolate import three_nn
    q, known = R.nn_inputs(reg, m)
    rd, ri = R.nn_ref(reg, m)
    d, i = three_nn(dev(q), dev(known))
    what = "three_nn %s m %d" % (reg.name, m)
    same(i, ri, what)
    same(d, rd, what)
    if R.exact(reg):
        ud, ui = R.nn_ref(R.unit_of(reg), m)
        same(i, ui, what + " (against the oracle at scale 1)")
        same(d, R.times_s2(reg, ud), what + " (against the oracle at scale 1)")
    if m in R.NN_ORDERED:
        rng = np.random.default_rng(m)
        perm = np.stack([rng.permutation(q.shape[1]) for _ in range(q.shape[0])]).astype(np.int32)
        d2, i2 = three_nn(dev(q), dev(known), order=dev(perm))
        same(i2, ri, what + " ordered")
        same(d2, rd, what + " ordered")


@pytest.mark.parametrize("levels", R.NESTED_LEVELS)
@ALL
def test_three_nn_nested(reg, levels):
    """one scan of a 2048-point cloud answers `levels` nested subsets: each level equal to the oracle on that subset"""
    from gspn_amd.tf_interpolate import nested_local_maps, nested_members, three_nn_nested
    b, n, m = 2, R.NN_QUERIES, 2048
    q, l1 = R.cloud(reg, None, b, n, 23), R.cloud(reg, None, b, m, 11)
    g = torch.Generator().manual_seed(levels)
    sizes = (m, 512, 128, 32)
    chain = [torch.stack([torch.randperm(sizes[i], generator=g)[:sizes[i + 1]] for _ in range(b)]).int().cuda() for i in range(3)]
    chain.append(torch.stack([torch.randperm(32, generator=g)[:2] for _ in range(b)]).int().cuda())
    members = [torch.arange(m, device="cuda").expand(b, -1)] + nested_members(chain) + [torch.zeros((b, 1), dtype=torch.long, device="cuda")]
    local = nested_local_maps(m, chain, prefixes=(1,))
    assert local.shape[0] == 6 == len(members)
    local, members = local[:levels].contiguous(), members[:levels]
    order = torch.stack([torch.randperm(n, generator=g) for _ in range(b)]).int().cuda() if levels % 4 == 0 else None
    dist, idx = three_nn_nested(dev(q), dev(l1), local, order=order)
    assert tuple(dist.shape) == (levels, b, n, 3)
    for lvl, mem in enumerate(members):
        known = np.stack([l1[s][mem[s].cpu().numpy()] for s in range(b)])
        od, oi = O.three_nn(q, known)
        what = "nested %s level %d of %d" % (reg.name, lvl, levels)
        same(idx[lvl], oi, what)
        same(dist[lvl].cpu().numpy().view(np.int32), od.view(np.int32), what)                  # bits, +inf of the short levels included


# ---- knn_point, nn_distance, nearest_point -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,k", R.KNN_CASES)
@ALL
def test_knn_point_direct(reg, n, m, k):
    from gspn_amd.tf_grouping import knn_point
    x1, x2 = R.knn_inputs(reg, n, m)
    rv, ri = R.knn_ref(reg, n, m, k)
    v, i = knn_point(k, dev(x1), dev(x2))
    same(i, ri, "knn %s" % reg.name)
    same(v, rv, "knn %s" % reg.name)
    if R.exact(reg):
        uv, ui = R.knn_ref(R.unit_of(reg), n, m, k)
        same(i, ui, "knn %s (against the oracle at scale 1)" % reg.name)
        same(v, R.times_s2(reg, uv), "knn %s (against the oracle at scale 1)" % reg.name)


@pytest.mark.parametrize("b,n,m", R.NND_CASES)
@ALL
def test_nn_distance_forward(reg, b, n, m):
    from gspn_amd.tf_nndistance import nn_distance
    a, c = R.nnd_inputs(reg, b, n, m)
    got = nn_distance(dev(a), dev(c))
    want = R.nnd_ref(reg, b, n, m)
    unit = R.nnd_ref(R.unit_of(reg), b, n, m) if R.exact(reg) else None
    for k, name in enumerate(("dist1", "idx1", "dist2", "idx2")):
        same(got[k], want[k], "nn_distance %s %s" % (reg.name, name))
        if unit is not None:
            same(got[k], unit[k] if k % 2 else R.times_s2(reg, unit[k]), "nn_distance %s %s (against the oracle at scale 1)" % (reg.name, name))


@ALL
def test_nearest_point(reg):
    from gspn_amd.nearest import nearest_point
    q, known = R.nearest_inputs(reg)
    rd, ri = R.nearest_ref(reg)
    d, i = nearest_point(dev(q), dev(known))
    same(i, ri, "nearest_point %s" % reg.name)
    same(d, rd, "nearest_point %s" % reg.name)
    if R.exact(reg):
        ud, ui = R.nearest_ref(R.unit_of(reg))
        same(i, ui, "nearest_point %s (against the oracle at scale 1)" % reg.name)
        same(d, R.times_s2(reg, ud), "nearest_point %s (against the oracle at scale 1)" % reg.name)


# ---- the box side: units, placement and shape (the reference's 1e-3 and margins are absolute) ---------------------------------------------

def box_case(reg, b, s, n, seed):
    """the regime's cloud and s boxes per scene around seeded points of it, sizes 0.05 .. 1.5 of the BASE cloud's extent per axis (so a
    box of a slab is a slab); the last box all zeros, the one before it far outside -> boxes (b, s, 6), pc (b, n, 3), CPU tensors"""
    base, pc = R.base(reg.kind, b, n, seed), R.cloud(reg, None, b, n, seed)
    rng = np.random.default_rng(seed + s)
    ext = np.maximum(base.max(1) - base.min(1), np.float32(2.0 ** -10))[:, None, :]                  # a flat axis: boxes 2^-10 thick
    centre = np.stack([pc[i][rng.integers(0, n, size=s)] for i in range(b)])
    size = ((0.05 + 1.45 * rng.random((b, s, 3))) * ext).astype(np.float32) * np.float32(reg.s)
    box = np.concatenate((centre, size.astype(np.float32)), -1).astype(np.float32)
    box[:, s - 1] = 0.0
    box[:, s - 2, :3] = pc.max(1) + 100 * ext[:, 0] * np.float32(reg.s)
    return torch.from_numpy(box), torch.from_numpy(pc.copy())


@pytest.mark.parametrize("margin", [0.0, 1e-3])
@BOX
def test_box_point_count_and_samples(reg, margin):
    from gspn_amd.rpointnet import box_point_count, sample_points_in_boxes
    from tests import roi_ref as RR
    box, pc = box_case(reg, 2, 24, 6000, 21)
    want = RR.box_point_count(box, pc, margin)
    assert (want[:, :22] > 0).all() and not want[:, 22].any() and int((want > 1).sum()) > 20     # (the all-zero row counts what its margin holds)
    assert torch.equal(box_point_count(box.cuda(), pc.cuda(), margin).cpu(), want)
    got = sample_points_in_boxes(box.cuda(), pc.cuda(), 64, 42, margin)
    assert torch.equal(got.cpu(), RR.sample_points_in_boxes(box, pc, 64, 42, margin))


@BOX
def test_box_shrink(reg):
    from gspn_amd.spn_boxes import box_shrink
    from tests import spn_ref as SR
    box, pc = box_case(reg, 2, 24, 6000, 22)
    want = SR.box_shrink_direct(box, pc)
    assert want.abs().sum(-1).gt(0).any() or reg.kind == "line"              # (a line's boxes are flat on two axes: all rows drop out)
    got = box_shrink(box.cuda(), pc.cuda()).cpu()
    assert torch.equal(got, want) and torch.equal(got.view(torch.int32), want.view(torch.int32))


@BOX
def test_crop_mean_of_coordinates(reg):
    """crop_mean over the coordinates themselves, 64 sampled points per box: the kernel adds in double and rounds once, the 64 summands of
    24 bits and one magnitude range add exactly in double and 1 / 64 is a power of two -- so the float64 restatement, rounded to float,
    is the result bit for bit"""
    from gspn_amd.rpointnet import crop_mean
    from tests import inference_ref as IR
    from tests import roi_ref as RR
    box, pc = box_case(reg, 2, 24, 6000, 23)
    idx = RR.sample_points_in_boxes(box, pc, 64, 5)
    want = IR.crop_mean(pc, idx).float()
    got = crop_mean(pc.cuda(), idx.cuda()).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def crops_of(box, pc, p, seed):
    """p crop points per box drawn with replacement from the points inside it (the origin for a box without one)"""
    from tests import roi_ref as RR
    g = torch.Generator().manual_seed(seed)
    b, r = box.shape[:2]
    crop = torch.zeros(b, r, p, 3)
    for i in range(b):
        members = RR.inside(box[i], pc[i])
        for k in range(r):
            rows = torch.nonzero(members[k])[:, 0]
            if len(rows):
                crop[i, k] = pc[i][rows[torch.randint(0, len(rows), (p,), generator=g)]]
    return crop.contiguous()


@BOX
def test_in_box_nearest_tile_through_unmolding(reg):
    from gspn_amd import rpointnet as RP
    from tests import detect_ref as DR
    b, r, n, p, c = 2, 24, 6000, 64, 5
    box, pc = box_case(reg, b, r, n, 24)
    crop = crops_of(box, pc, p, 24)
    g = torch.Generator().manual_seed(24)
    masks = torch.randn(b, r, p, c, generator=g) * 3.0
    ids = torch.randint(0, c, (b, r), generator=g).int()
    got = RP.unmold_segmentation(masks.cuda(), box.cuda(), ids.cuda(), crop.cuda(), pc.cuda())
    want = DR.unmold_segmentation(masks, box, ids, crop, pc)
    assert want.abs().sum() > 0
    assert torch.equal(got.cpu(), want)


@BOX
def test_in_box_nearest_tile_through_the_lift(reg):
    """lift_masks on the regime's cloud as the scan's vertices: the masks and their point counts are the definition's (the two
    confidences are sums of probabilities in double: they do not read a coordinate)"""
    from gspn_amd.lift import lift_masks
    from tests import lift_ref as LR
    r, v, p, n, c = 24, 6000, 64, 50, 6
    box, pc = box_case(reg, 1, r, v, 25)
    crop = crops_of(box, pc, p, 25)
    rng = np.random.default_rng(25)
    sem = rng.random((n, c), dtype=np.float32) + np.float32(0.01)
    case = dict(verts=pc[0].numpy(), crops=crop[0].numpy(), boxes=box[0].numpy(),
                masks=(1.0 / (1.0 + np.exp(-2.5 * rng.standard_normal((r, p))))).astype(np.float32),
                class_ids=rng.integers(1, c, r).astype(np.int32), src=rng.integers(0, n, v).astype(np.int32),
                sem_prob=(sem / sem.sum(-1, keepdims=True)).astype(np.float32), vert_fb=(0.05 + 0.9 * rng.random(v)).astype(np.float32))
    order = ("verts", "crops", "boxes", "masks", "class_ids", "src", "sem_prob", "vert_fb")
    _, _, want_mask, want_points = LR.lift(*[case[k] for k in order], 0.4)
    assert want_points.sum() > 0
    _, _, mask, points = lift_masks(**{k: torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in order})
    same(mask, want_mask, "mask")
    same(points, want_points, "points")
