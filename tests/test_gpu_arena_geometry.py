"""Sampling, grouping, interpolation, Chamfer and the drop-in *_ws symbols on poisoned, guard-banded allocations (tests/arena.py).

Every row of CASES runs unpatched and under the fills 0x00, 0xFF, 0x7F.  A: no guard band of any allocation made inside the wrapper is
touched.  B: every returned tensor has the bits of the unpatched run.  Rows with `atomic=` add floats with atomicAdd (the line is
cited); their sums have no order, so they are held to the float64 comparison of tests/test_gpu_dropin_grads.py instead (1e-5 of the
magnitude a sum went through), in every run, and must be NaN-free.  Five rows are masked (MASKED below): the spatial order that
farthest_point_sample returns beside its samples is open inside a voxel (include/gspn_hip.h:83-88) -- every run is checked against all
the header fixes, the runs against each other as permutations --, and inverse_lists leaves order behind the kept positions unwritten
(include/gspn_hip.h:727-729) -- exactly that tail is masked.

Shapes are the smallest that select each path; the thresholds are the wrappers' (tf_sampling.py:85,103; tf_grouping.py:40;
tf_nndistance.py:39; csrc/grouping.hip CSR_LDS_MAX_N)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import data as D
from tests.arena import Case, sweep

pytestmark = pytest.mark.gpu

CASES = []
P = ctypes.c_void_p


def case(fn):
    CASES.append(fn)
    return fn


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return P(t.data_ptr())


def _st():
    return P(torch.cuda.current_stream().cuda_stream)


def leaf(t):
    return t.detach().requires_grad_(True)


def close(got, ref, scale, tol=1e-5):
    """tests/test_gpu_dropin_grads.py: |got - ref| <= tol * (the sum of |terms| that went into each element)"""
    got, ref = np.asarray(got.detach().cpu().numpy(), np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    bound = tol * np.maximum(np.asarray(scale, np.float64), 1e-30) + 1e-12
    err = np.abs(got - ref)
    assert (err <= bound).all(), "max err/bound %.3g" % float((err / bound).max())


# ---- sampling ------------------------------------------------------------------------------------------------------------------------
@case
def fps_single_workgroup():
    from gspn_amd.tf_sampling import farthest_point_sample
    xyz = dev(D.batch("D", 2, 1000, 3))
    return Case("farthest_point_sample n=1000 m=64 (on-chip kernel)", lambda: farthest_point_sample(64, xyz))


@case
def fps_cells():
    from gspn_amd import tf_sampling as S
    xyz = dev(D.batch("S", 2, S.FPS_CELLS_MIN_N, 5))
    assert S.FPS_MODE == "cells" and S.FPS_CELLS_MIN_N == 8192
    return Case("farthest_point_sample n=8192 m=64 (cells)", lambda: S.farthest_point_sample(64, xyz))


def _any_order_inside_a_voxel(i, t):
    """output 1, the spatial order: the counting sort of the pre-pass places the points of one voxel with LDS atomics, and the header
    leaves their order open, so two correct runs differ.  Everything the header does fix is asserted on EVERY run by _check_voxel_order /
    _check_cell_order below -- a complete description of the valid answers, so a stale or missing slot fails there; across runs what is
    left to compare is that each is a permutation of 0..n-1.  Output 0, the samples, is compared bit for bit."""
    return t.sort(1).values if i == 1 else t


def _voxel_codes(xyz):
    """fps_bin_kernel's 12-bit Morton voxel of every point (csrc/sampling.hip: voxel()), in float32 as the kernel computes it:
    q = (int)((x - lo) * (16 / (hi - lo))) clamped to 0..15 per axis, the bits of x, y, z interleaved"""
    x = np.ascontiguousarray(xyz, np.float32)
    lo, hi = x.min(1, keepdims=True), x.max(1, keepdims=True)
    ext = (hi - lo).astype(np.float32)
    inv = np.where(ext > 0, np.float32(16.0) / np.where(ext > 0, ext, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    q = np.clip((((x - lo).astype(np.float32)) * inv).astype(np.float32).astype(np.int64), 0, 15)
    spread = lambda v: (v & 1) | ((v & 2) << 2) | ((v & 4) << 4) | ((v & 8) << 6)      # noqa: E731
    return spread(q[..., 0]) | (spread(q[..., 1]) << 1) | (spread(q[..., 2]) << 2)


def _check_voxel_order(order, codes):
    """gspn_hip.h:87-88: the scene's points in 16^3-voxel Morton order, any order inside a voxel <=> a permutation whose voxel codes ascend"""
    o = order.cpu().numpy().astype(np.int64)
    b, n = o.shape
    assert (np.sort(o, 1) == np.arange(n)).all(), "the order is no permutation of 0..n-1: a slot was not written, or written twice"
    along = np.take_along_axis(codes, o, 1)
    assert (np.diff(along, axis=1) >= 0).all(), "the voxel codes do not ascend along the order"


def _check_cell_order(order, codes):
    """gspn_hip.h:71-73,83-85: 16 cells of csz = ceil(n/16) consecutive points of the voxel order, the reference tie rank (k mod 512, k)
    ascending inside a cell <=> a permutation, rank-sorted inside each cell, no voxel code of a cell above one of the next cell"""
    o = order.cpu().numpy().astype(np.int64)
    b, n = o.shape
    assert (np.sort(o, 1) == np.arange(n)).all(), "the order is no permutation of 0..n-1: a slot was not written, or written twice"
    csz = (n + 15) // 16
    along = np.take_along_axis(codes, o, 1)
    rank = ((o & 511) << 22) | (o >> 9)                     # fps_tie_rank, csrc/fps_common.h
    top = -1 * np.ones(b, np.int64)
    for c in range(0, n, csz):
        assert (np.diff(rank[:, c:c + csz], axis=1) > 0).all(), "cell %d is not in tie-rank order" % (c // csz)
        assert (along[:, c:c + csz].min(1) >= top).all(), "cell %d holds a voxel below the cell before it" % (c // csz)
        top = along[:, c:c + csz].max(1)


@case
def fps_cells_return_order():
    from gspn_amd import tf_sampling as S
    cloud = D.batch("S", 2, S.FPS_CELLS_MIN_N, 5)
    xyz, codes = dev(cloud), _voxel_codes(cloud)

    def run():
        out, order = S.farthest_point_sample(64, xyz, return_order=True)
        _check_voxel_order(order, codes)
        return out, order
    return Case("farthest_point_sample n=8192 m=64 (cells, return_order)", run, canon=_any_order_inside_a_voxel, header="include/gspn_hip.h:87-88")


@case
def fps_cells_return_cell_order():
    from gspn_amd import tf_sampling as S
    cloud = D.batch("U", 1, 8193, 6)
    xyz, codes = dev(cloud), _voxel_codes(cloud)

    def run():
        old, S.VOXEL_ORDER = S.VOXEL_ORDER, False          # the order is then the first b*n words of the workspace itself
        try:
            out, order = S.farthest_point_sample(37, xyz, return_order=True)
        finally:
            S.VOXEL_ORDER = old
        _check_cell_order(order, codes)
        return out, order
    return Case("farthest_point_sample n=8193 m=37 (cells, 16-cell order out of the workspace)", run, canon=_any_order_inside_a_voxel,
                header="include/gspn_hip.h:83-85")


@case
def fps_multi_cu():
    from gspn_amd import _lib as L
    from gspn_amd import tf_sampling as S
    xyz = dev(D.batch("U", 2, 32769, 9))

    def run():
        out = S.farthest_point_sample(64, xyz)
        L.check_async(block=True)                          # the status word inside the exact-size workspace
        return out
    return Case("farthest_point_sample b=2 n=32769 m=64 (multi-CU, exact gspn_fps_multi_ws_bytes)", run)


def _gather_inputs():
    rng = np.random.default_rng(12)
    b, n, m = 2, 301, 1000
    inp = rng.standard_normal((b, n, 3)).astype(np.float32)
    idx = rng.integers(0, n, size=(b, m)).astype(np.int32)
    idx[:, : m // 4] = idx[:, :1]                          # a quarter of the samples hit one point
    go = rng.standard_normal((b, m, 3)).astype(np.float32)
    return inp, idx, go


@case
def gather_point_atomic_grad():
    from gspn_amd import invlists
    from gspn_amd.tf_sampling import gather_point
    inp, idx, go = _gather_inputs()
    t_inp, t_idx, t_go = dev(inp), dev(idx), dev(go)
    ref_out = O.gather_point(inp, idx)
    ref = O.gather_point_grad(np.zeros_like(inp), idx, go)
    scale = O.gather_point_grad(np.zeros_like(inp), idx, np.abs(go))
    assert invlists.use_atomic(3)

    def run():
        x = leaf(t_inp)
        out = gather_point(x, t_idx)
        out.backward(t_go)
        return out.detach(), x.grad

    def verify(res):
        np.testing.assert_array_equal(res[0].cpu().numpy(), ref_out)
        close(res[1], ref, scale)
    return Case("gather_point + gradient (gspn_scatteraddpoint)", run, atomic="gspn_amd/csrc/sampling.hip:1058", verify=verify)


@case
def gather_point_csr_grad():
    from gspn_amd import invlists
    from gspn_amd.tf_sampling import gather_point
    inp, idx, go = _gather_inputs()
    t_inp, t_idx, t_go = dev(inp), dev(idx), dev(go)

    def run():
        old, invlists.DETERMINISTIC = invlists.DETERMINISTIC, True
        try:
            x = leaf(t_inp)
            out = gather_point(x, t_idx)
            out.backward(t_go)
            return out.detach(), x.grad
        finally:
            invlists.DETERMINISTIC = old
    return Case("gather_point + gradient through the inverse lists", run)


@case
def prob_sample():
    from gspn_amd.tf_sampling import prob_sample
    rng = np.random.default_rng(2)
    w, r = dev(rng.random((3, 37), dtype=np.float32)), dev(rng.random((3, 129), dtype=np.float32))
    return Case("prob_sample b=3 n=37 m=129", lambda: prob_sample(w, r))


def _scenes():
    from tests import dataset_ref as DR
    both = [DR.labelled_scene(32768, DR.SIZES[s], 8, 40 + s, False) for s in range(2)]
    return dev(np.stack([p for p, _ in both])), dev(np.stack([l for _, l in both]))


@case
def fps_segments_every_size_class():
    from gspn_amd import dataset
    pc, label = _scenes()
    return Case("fps_segments (2, 32768) g=8 m=64: every size class of tests/test_gpu_dataset.py", lambda: dataset.fps_segments(pc, label, 8, 64, 7))


@case
def instance_point_sets_resample_augment():
    from gspn_amd import dataset
    pc, label = _scenes()
    pc, label = pc[:, :4096].contiguous(), label[:, :4096].contiguous()
    color = torch.rand(2, 4096, 3, generator=torch.Generator().manual_seed(3)).cuda()
    rot = torch.eye(3, dtype=torch.float64).expand(2, 3, 3).clone()
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1] = 0.6, 0.8, -0.8, 0.6
    tr = torch.tensor([[0.5, -1.0, 2.0], [0.0, 0.25, -3.0]], dtype=torch.float64)

    def run():
        ins = dataset.instance_point_sets(pc, label, 8, 32, 5)
        down = dataset.resample_scene(pc, color, label, label % 3, 1024, 5)        # FPS + gather_point
        up = dataset.resample_scene(pc[:, :1000].contiguous(), color[:, :1000].contiguous(), label[:, :1000].contiguous(),
                                    label[:, :1000].contiguous(), 1024, 5)         # padding draws
        aug = dataset.augment_and_box(down[0], ins, torch.tensor([8, 5]), rot, tr)
        return ins, down, up, aug
    return Case("instance_point_sets, resample_scene (down and up), augment_and_box", run)


# ---- grouping ------------------------------------------------------------------------------------------------------------------------
def _ball_small(ns):
    from gspn_amd.tf_grouping import query_ball_point
    xyz = D.batch("U", 2, 1000, 14)
    q = xyz[:, :37].copy()
    q[:, 30:] += 5.0                                       # rows without any hit: zero-filled (include/gspn_hip.h:146)
    t_xyz, t_q = dev(xyz), dev(q)

    def run():
        idx, cnt = query_ball_point(0.1, ns, t_xyz, t_q)
        assert int((cnt == 0).sum()) == 14 and not bool(idx[:, 30:].any())
        return idx, cnt
    return Case("query_ball_point n=1000 m=37 ns=%d (no workspace)" % ns, run)


@case
def ball_query_ns5():
    return _ball_small(5)


@case
def ball_query_ns32():
    return _ball_small(32)


def _ball_ws(kind):
    from gspn_amd.tf_grouping import query_ball_point
    from tests.test_gpu_ball_query_ragged import grid_case
    xyz, q, radius, ns = grid_case(kind, 8192)             # 301 queries, the last 21 far outside the cloud
    t_xyz, t_q = dev(xyz), dev(q)

    def run():
        idx, cnt = query_ball_point(radius, ns, t_xyz, t_q)
        assert bool((cnt[:, -21:] == 0).all()) and not bool(idx[:, -21:].any())
        return idx, cnt
    return Case("query_ball_point n=8192 m=301 (%s cloud, exact gspn_ball_ws_bytes)" % kind, run)


@case
def ball_query_ws_sparse():
    return _ball_ws("capped")


@case
def ball_query_ws_dense():
    return _ball_ws("dense")


@case
def ball_query_ws_mixed():
    return _ball_ws("mixed")


@case
def knn_point():
    from gspn_amd.tf_grouping import knn_point
    xyz, q = dev(D.batch("D", 2, 700, 15)), dev(D.batch("U", 2, 65, 16))
    x5 = torch.rand(2, 70, 5, generator=torch.Generator().manual_seed(1)).cuda()
    return Case("knn_point: direct (k=7) and the dense matrix + selection sort (c=5, and k=33)",
                lambda: (knn_point(7, xyz, q), knn_point(4, x5, x5[:, :9].contiguous()), knn_point(33, xyz[:, :100].contiguous(), q)))


@case
def select_top_k():
    from gspn_amd.tf_grouping import select_top_k
    dist = torch.rand(2, 37, 130, generator=torch.Generator().manual_seed(8)).cuda()
    # include/gspn_hip.h:161-162 says nothing of the columns >= k, and csrc/grouping.hip:745 copies the whole row first: all n columns compared
    return Case("select_top_k k=5 < n=130: both (b,m,n) outputs, every column", lambda: select_top_k(5, dist))


def _group_inputs(c):
    from tests.test_gpu_dropin_grads import contended_group_idx
    rng = np.random.default_rng(100 + c)
    b, n, m, ns = 2, 500, 70, 32
    idx = contended_group_idx(rng, b, n, m, ns)
    pts = rng.standard_normal((b, n, c)).astype(np.float32)
    go = rng.standard_normal((b, m, ns, c)).astype(np.float32)
    return pts, idx, go


@case
def group_point_c3_atomic_grad():
    from gspn_amd import invlists
    from gspn_amd.tf_grouping import group_point
    pts, idx, go = _group_inputs(3)
    t_pts, t_idx, t_go = dev(pts), dev(idx), dev(go)
    ref_out = O.group_point(pts, idx)
    ref = O.group_point_grad(np.zeros_like(pts), idx, go)
    scale = O.group_point_grad(np.zeros_like(pts), idx, np.abs(go))
    assert invlists.use_atomic(3) and not invlists.use_atomic(64)

    def run():
        x = leaf(t_pts)
        out = group_point(x, t_idx)
        out.backward(t_go)
        return out.detach(), x.grad

    def verify(res):
        np.testing.assert_array_equal(res[0].cpu().numpy(), ref_out)
        close(res[1], ref, scale)
    return Case("group_point c=3 + gradient (gspn_grouppoint_grad)", run, atomic="gspn_amd/csrc/grouping.hip:503,505", verify=verify)


@case
def group_point_c64_csr_grad():
    from gspn_amd.tf_grouping import group_point
    pts, idx, go = _group_inputs(64)
    t_pts, t_idx, t_go = dev(pts), dev(idx), dev(go)

    def run():
        x = leaf(t_pts)
        out = group_point(x, t_idx)
        out.backward(t_go)
        return out.detach(), x.grad
    return Case("group_point c=64 + gradient through the inverse lists", run)


@case
def group_maxpool():
    from gspn_amd.tf_grouping import group_maxpool
    rng = np.random.default_rng(5)
    b, n, c, m, ns = 2, 700, 24, 90, 12
    pts = (np.round(rng.standard_normal((b, n, c)) * 2) / 2).astype(np.float32)       # tied maxima
    idx = rng.integers(0, n, size=(b, m, ns)).astype(np.int32)
    go = rng.standard_normal((b, m, c)).astype(np.float32)
    ref_out, ref_mi = O.group_maxpool(pts, idx)
    ref = O.group_maxpool_grad(pts, ref_mi, go)
    scale = O.group_maxpool_grad(pts, ref_mi, np.abs(go))
    t_pts, t_idx, t_go = dev(pts), dev(idx), dev(go)

    def run():
        x = leaf(t_pts)
        out, mi = group_maxpool(x, t_idx)
        out.backward(t_go)
        return out.detach(), mi, x.grad

    def verify(res):
        np.testing.assert_array_equal(res[0].cpu().numpy(), ref_out)
        np.testing.assert_array_equal(res[1].cpu().numpy(), ref_mi)
        close(res[2], ref, scale)
    return Case("group_maxpool + gradient", run, atomic="gspn_amd/csrc/grouping.hip:722", verify=verify)


# ---- interpolation -------------------------------------------------------------------------------------------------------------------
@case
def three_nn_dense_ordered_short():
    from gspn_amd.tf_interpolate import three_nn
    g = torch.Generator().manual_seed(21)
    q, known = dev(D.batch("S", 2, 701, 17)), dev(D.batch("S", 2, 130, 18))
    order = torch.stack([torch.randperm(701, generator=g) for _ in range(2)]).int().cuda()
    return Case("three_nn: dense, ordered, m=2 and m=1 known points",
                lambda: (three_nn(q, known), three_nn(q, known, order=order), three_nn(q, known[:, :2].contiguous()),
                         three_nn(q, known[:, :1].contiguous(), order=order)))


@case
def three_nn_cell_grid():
    from gspn_amd.tf_interpolate import three_nn
    q, known = dev(D.batch("U", 2, 700, 51)), dev(D.batch("U", 2, 2049, 50))      # tests/test_gpu_kernel_instances.py GRID_CASES: 16 points per thread
    return Case("three_nn against m=2049 known points (cell grid)", lambda: three_nn(q, known))


def _nested(sizes, n, ordered):
    from gspn_amd.tf_interpolate import nested_local_maps, three_nn_nested
    b, m = 2, sizes[0]
    g = torch.Generator().manual_seed(n + len(sizes))
    chain = [torch.stack([torch.randperm(sizes[i], generator=g)[:sizes[i + 1]] for _ in range(b)]).int().cuda() for i in range(len(sizes) - 1)]
    q, known = dev(D.batch("D", b, n, 23)), dev(D.batch("D", b, m, 11))
    order = torch.stack([torch.randperm(n, generator=g) for _ in range(b)]).int().cuda() if ordered else None
    if chain:
        return Case("three_nn_nested %d levels %s" % (len(sizes), sizes),
                    lambda: (lambda local: (local, three_nn_nested(q, known, local, order=order)))(nested_local_maps(m, chain)))
    local = torch.arange(m, dtype=torch.int32, device="cuda").expand(1, b, m).contiguous()
    return Case("three_nn_nested 1 level %s" % (sizes,), lambda: three_nn_nested(q, known, local, order=order))


@case
def three_nn_nested_1():
    return _nested((100,), 63, False)


@case
def three_nn_nested_2():
    return _nested((100, 2), 700, True)


@case
def three_nn_nested_4():
    return _nested((1000, 256, 64, 16), 700, True)


@case
def three_nn_weights_and_fp_geometry():
    from gspn_amd.geometry import fp_geometry
    q, known = dev(D.batch("D", 2, 701, 17)), dev(D.batch("D", 2, 130, 18))        # "D": exact zero distances go through the 1e-10 floor
    return Case("fp_geometry: three_nn, three_nn_weights, inverse lists", lambda: fp_geometry(q, known).tensors())


def _interp_inputs(c):
    rng = np.random.default_rng(c)
    b, n, m = 2, 513, 50
    idx = rng.integers(0, m, size=(b, n, 3)).astype(np.int32)
    idx[:, ::7, :] = idx[:, :1, :1]                        # hot sparse points; also i1 == i2 == i3 rows
    w = rng.random((b, n, 3)).astype(np.float32)
    w /= w.sum(2, keepdims=True)
    pts = rng.standard_normal((b, m, c)).astype(np.float32)
    go = rng.standard_normal((b, n, c)).astype(np.float32)
    return pts, idx, w, go


@case
def three_interpolate_csr_grad():
    from gspn_amd.tf_interpolate import three_interpolate
    pts, idx, w, go = _interp_inputs(37)
    t_pts, t_idx, t_w, t_go = dev(pts), dev(idx), dev(w), dev(go)

    def run():
        x = leaf(t_pts)
        out = three_interpolate(x, t_idx, t_w)
        out.backward(t_go)
        return out.detach(), x.grad
    return Case("three_interpolate c=37 + gradient through the inverse lists", run)


@case
def three_interpolate_atomic_grad():
    from gspn_amd import invlists
    from gspn_amd.tf_interpolate import three_interpolate
    pts, idx, w, go = _interp_inputs(37)
    t_pts, t_idx, t_w, t_go = dev(pts), dev(idx), dev(w), dev(go)
    ref = O.three_interpolate_grad(np.zeros_like(pts), idx, w, go)
    scale = O.three_interpolate_grad(np.zeros_like(pts), idx, w, np.abs(go))

    def run():
        old, invlists.ATOMIC_GRADS = invlists.ATOMIC_GRADS, True
        try:
            x = leaf(t_pts)
            three_interpolate(x, t_idx, t_w).backward(t_go)
            return x.grad
        finally:
            invlists.ATOMIC_GRADS = old
    return Case("three_interpolate gradient (gspn_threeinterpolate_grad)", run, atomic="gspn_amd/csrc/interpolate.hip:480-482",
                verify=lambda res: close(res, ref, scale))


def _fp_concat(form, c2=33, c1=3):
    from gspn_amd import _lib as L
    from gspn_amd.geometry import inverse_lists
    from gspn_amd.pointnet_util import fp_concat
    rng = np.random.default_rng(c2 + c1)
    b, n, m = 2, 513, 50
    idx = rng.integers(0, m, size=(b, n, 3)).astype(np.int32)
    idx[:, :300, :] = 0                                    # one list of 900 entries: longer than any split_t used below
    w = rng.random((b, n, 3)).astype(np.float32)
    p2, p1 = rng.standard_normal((b, m, c2)).astype(np.float32), rng.standard_normal((b, n, c1)).astype(np.float32)
    ld = (c2 + c1 + 3) // 4 * 4
    go = rng.standard_normal((b * n, ld)).astype(np.float32)
    t_idx, t_w, t_p2, t_p1, t_go = dev(idx), dev(w), dev(p2), dev(p1), dev(go)
    gi = np.ascontiguousarray(go[:, :c2].reshape(b, n, c2))
    ref = O.three_interpolate_grad(np.zeros_like(p2), idx, w, gi)
    scale = O.three_interpolate_grad(np.zeros_like(p2), idx, w, np.abs(gi))

    def run():
        a, c = leaf(t_p2), leaf(t_p1)
        lists = inverse_lists(t_idx.reshape(b, 3 * n), m) if form != "atomic" else (None, None)
        if form == "csr_split":
            g2 = torch.empty((b, m, c2), dtype=torch.float32, device="cuda")
            L.check(L.lib().gspn_fp_concat_grad_csr_split(b, n, m, c2, 0, ld, L.ptr(t_go), L.ptr(lists[0]), L.ptr(lists[1]), L.ptr(t_w), L.ptr(g2), None,
                                                          128, L.stream()), "fp_concat_grad_csr_split")
            return g2
        out = fp_concat(a, t_idx, t_w, c, *lists)
        out.backward(t_go)
        return out.detach(), a.grad, c.grad
    if form == "atomic":
        def verify(res):
            close(res[1], ref, scale)
            assert torch.equal(res[2], t_go[:, c2:c2 + c1].reshape(b, n, c1)) and not bool(res[0][:, c2 + c1:].any())
        return Case("fp_concat c2=33 c1=3 + gradient (gspn_fp_concat_grad)", run, atomic="gspn_amd/csrc/interpolate.hip:581-583", verify=verify)
    return Case("fp_concat c2=33 c1=3 + gradient: %s" % form, run,
                note="gspn_fp_concat_grad_csr_split has no public wrapper of its own (pointnet_util.py:310 calls it inside the pre-aggregated FP layer): called as there")


@case
def fp_concat_atomic():
    return _fp_concat("atomic")


@case
def fp_concat_csr():
    return _fp_concat("csr")


@case
def fp_concat_csr_split():
    return _fp_concat("csr_split")


def _inverse_lists(b, ln, n):
    from gspn_amd.geometry import inverse_lists
    g = torch.Generator().manual_seed(ln * 7 + n)
    idx = torch.randint(0, n, (b, ln), generator=g, dtype=torch.int32)
    idx[:, : ln // 3] = idx[:, : ln // 3] % 3 + (n - 3)    # a few crowded values at the very end of the scan
    bad = torch.rand(b, ln, generator=g) < 0.07            # dropped positions, as tests/test_gpu_kernel_instances.py plants them
    idx[bad] = torch.where(torch.rand(int(bad.sum()), generator=g) < 0.5, torch.tensor(-1, dtype=torch.int32), torch.tensor(n + 5, dtype=torch.int32))
    kept = ((idx >= 0) & (idx < n)).sum(1)
    assert bool((kept < ln).all()) and bool((kept > 0).all())
    t_idx = idx.cuda()

    def run():
        order, offsets = inverse_lists(t_idx, n)
        assert torch.equal(offsets[:, n].cpu().long(), kept)
        return order, offsets

    def written(i, t, outs):
        """order[s, offsets[s, n]:] is not written (include/gspn_hip.h:727-729); offsets, and order in front of that, are compared in full"""
        if i != 0:
            return None
        return torch.arange(ln, device=t.device).expand(b, ln) < outs[1][:, n].long().unsqueeze(1)
    return Case("inverse_lists b=%d L=%d n=%d, 7 %% of the positions dropped" % (b, ln, n), run, mask=written, header="include/gspn_hip.h:727-729")


@case
def inverse_lists_lds():
    return _inverse_lists(1, 5000, 32768)


@case
def inverse_lists_global_32769():
    return _inverse_lists(2, 5000, 32769)


@case
def inverse_lists_global_40001():
    return _inverse_lists(3, 2049, 40001)


# ---- Chamfer -------------------------------------------------------------------------------------------------------------------------
def _chamfer(b, n, m, seed):
    from gspn_amd.tf_nndistance import nn_distance
    rng = np.random.default_rng(seed)
    a, c = rng.random((b, n, 3), dtype=np.float32), rng.random((b, m, 3), dtype=np.float32)
    g1, g2 = rng.standard_normal((b, n)).astype(np.float32), rng.standard_normal((b, m)).astype(np.float32)
    t = [dev(x) for x in (a, c, g1, g2)]

    def run():
        x, y = leaf(t[0]), leaf(t[1])
        d1, i1, d2, i2 = nn_distance(x, y)
        (d1 * t[2]).sum().add((d2 * t[3]).sum()).backward()
        return d1.detach(), i1, d2.detach(), i2, x.grad, y.grad
    return a, c, g1, g2, run


def _chamfer_atomic(name, b, n, m, seed):
    from gspn_amd import tf_nndistance as T
    a, c, g1, g2, run = _chamfer(b, n, m, seed)
    assert n + m <= T.LDS_GRAD_MAX_POINTS
    rd1, ri1, rd2, ri2 = O.nn_distance(a, c)
    rg1, rg2 = O.nn_distance_grad(a, c, g1, ri1, g2, ri2)

    def verify(res):
        for got, want in zip(res[:4], (rd1, ri1, rd2, ri2)):
            np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_allclose(res[4].cpu().numpy(), rg1, rtol=1e-5, atol=1e-5)      # tests/test_gpu_kernel_instances.py:362
        np.testing.assert_allclose(res[5].cpu().numpy(), rg2, rtol=1e-5, atol=1e-5)
    return Case(name, run, atomic="gspn_amd/csrc/nndistance.hip:151,157 (LDS)", verify=verify)


@case
def nn_distance_csr():
    a, c, g1, g2, run = _chamfer(2, 4000, 100, 3)          # n + m = 4100 > 4096: the gather through both inverse lists, n != m
    return Case("nn_distance n=4000 m=100 + gradient (CSR)", run)


@case
def nn_distance_global_atomic_grad():
    from gspn_amd import invlists
    a, c, g1, g2, run = _chamfer(2, 4000, 100, 3)          # the same clouds through the plain symbol: memset + global atomics beyond the LDS size
    rd1, ri1, rd2, ri2 = O.nn_distance(a, c)
    rg1, rg2 = O.nn_distance_grad(a, c, g1, ri1, g2, ri2)

    def atomic_run():
        old, invlists.ATOMIC_GRADS = invlists.ATOMIC_GRADS, True
        try:
            return run()
        finally:
            invlists.ATOMIC_GRADS = old

    def verify(res):
        for got, want in zip(res[:4], (rd1, ri1, rd2, ri2)):
            np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_allclose(res[4].cpu().numpy(), rg1, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(res[5].cpu().numpy(), rg2, rtol=1e-5, atol=1e-5)
    return Case("nn_distance n=4000 m=100 + gradient (gspn_nmdistance_grad, global atomics)", atomic_run, atomic="gspn_amd/csrc/nndistance.hip:112-113", verify=verify)


@case
def nn_distance_single_points():
    return _chamfer_atomic("nn_distance n=1 m=1 and its gradient (gspn_nmdistance_grad)", 3, 1, 1, 4)


@case
def nn_distance_one_workgroup_grad():
    return _chamfer_atomic("nn_distance n=100 m=7 + gradient (gspn_nmdistance_grad)", 3, 100, 7, 7)


@case
def nn_distance_two_queries_per_lane():
    a, c, g1, g2, run = _chamfer(1024, 37, 1100, 5)        # tests/test_gpu_kernel_instances.py:323: nm_distance_kernel<2> both ways
    rd1, ri1, rd2, ri2 = O.nn_distance(a, c)
    rg1, rg2 = O.nn_distance_grad(a, c, g1, ri1, g2, ri2)

    def verify(res):
        for got, want in zip(res[:4], (rd1, ri1, rd2, ri2)):
            np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_allclose(res[4].cpu().numpy(), rg1, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(res[5].cpu().numpy(), rg2, rtol=1e-5, atol=1e-5)
    return Case("nn_distance b=1024 n=37 m=1100 (two queries per lane)", run, atomic="gspn_amd/csrc/nndistance.hip:151,157 (LDS)", verify=verify)


# ---- the drop-in symbols with a workspace: exactly *_ws_bytes, taken from the patched torch.empty ---------------------------------------
def _exact_ws(nbytes):
    assert nbytes > 0
    return torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")


@case
def grouppoint_grad_ws():
    from gspn_amd import _lib as L
    lib = L.lib()
    pts, idx, go = _group_inputs(6)
    b, n, c = pts.shape
    m, ns = idx.shape[1:]
    t_idx, t_go = dev(idx), dev(go)
    ref = O.group_point_grad(np.zeros_like(pts), idx, go)

    def run():
        g, ws = torch.empty((b, n, c), device="cuda"), _exact_ws(lib.gspn_grouppoint_grad_ws_bytes(b, n, c, m, ns))
        assert lib.gspn_grouppoint_grad_ws(b, n, c, m, ns, _p(t_go), _p(t_idx), _p(g), _p(ws), _st()) == 0
        torch.cuda.current_stream().synchronize()
        np.testing.assert_array_equal(g.cpu().numpy(), ref)
        return g
    return Case("gspn_grouppoint_grad_ws c=6", run, note="called through ctypes: the Python ops take the inverse-list gathers instead")


@case
def scatteraddpoint_ws():
    from gspn_amd import _lib as L
    lib = L.lib()
    inp, idx, go = _gather_inputs()
    b, n, _ = inp.shape
    m = idx.shape[1]
    t_idx, t_go = dev(idx), dev(go)
    ref = O.gather_point_grad(np.zeros_like(inp), idx, go)

    def run():
        g, ws = torch.empty((b, n, 3), device="cuda"), _exact_ws(lib.gspn_scatteraddpoint_ws_bytes(b, n, m))
        assert lib.gspn_scatteraddpoint_ws(b, n, m, _p(t_go), _p(t_idx), _p(g), _p(ws), _st()) == 0
        torch.cuda.current_stream().synchronize()
        np.testing.assert_array_equal(g.cpu().numpy(), ref)
        return g
    return Case("gspn_scatteraddpoint_ws", run, note="called through ctypes")


@case
def threeinterpolate_grad_ws():
    from gspn_amd import _lib as L
    lib = L.lib()
    pts, idx, w, go = _interp_inputs(37)
    b, m, c = pts.shape
    n = idx.shape[1]
    t_idx, t_w, t_go = dev(idx), dev(w), dev(go)
    ref = O.three_interpolate_grad(np.zeros_like(pts), idx, w, go)

    def run():
        g, ws = torch.empty((b, m, c), device="cuda"), _exact_ws(lib.gspn_threeinterpolate_grad_ws_bytes(b, n, c, m))
        assert lib.gspn_threeinterpolate_grad_ws(b, n, c, m, _p(t_go), _p(t_idx), _p(t_w), _p(g), _p(ws), _st()) == 0
        torch.cuda.current_stream().synchronize()
        np.testing.assert_array_equal(g.cpu().numpy(), ref)
        return g
    return Case("gspn_threeinterpolate_grad_ws c=37", run, note="called through ctypes")


@case
def nmdistance_grad_ws():
    from gspn_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(7)
    b, n, m = 3, 100, 7
    a, c = rng.standard_normal((b, n, 3)).astype(np.float32), rng.standard_normal((b, m, 3)).astype(np.float32)
    d1, i1, d2, i2 = O.nn_distance(a, c)
    g1, g2 = rng.standard_normal((b, n)).astype(np.float32), rng.standard_normal((b, m)).astype(np.float32)
    t = [dev(x) for x in (a, c, g1, i1, g2, i2)]

    def run():
        ga, gc = torch.empty((b, n, 3), device="cuda"), torch.empty((b, m, 3), device="cuda")
        ws = _exact_ws(lib.gspn_nmdistance_grad_ws_bytes(b, n, m))
        assert lib.gspn_nmdistance_grad_ws(b, n, _p(t[0]), m, _p(t[1]), _p(t[2]), _p(t[3]), _p(t[4]), _p(t[5]), _p(ga), _p(gc), _p(ws), _st()) == 0
        return ga, gc
    return Case("gspn_nmdistance_grad_ws n=100 m=7", run, note="called through ctypes")


@case
def queryballpoint_ws():
    from gspn_amd import _lib as L
    from tests.test_gpu_ball_query_ragged import grid_case
    lib = L.lib()
    xyz, q, radius, ns = grid_case("capped", 8192 + 37)
    b, n, m = 2, xyz.shape[1], q.shape[1]
    t_xyz, t_q = dev(xyz), dev(q)

    def run():
        idx, cnt = torch.empty((b, m, ns), dtype=torch.int32, device="cuda"), torch.empty((b, m), dtype=torch.int32, device="cuda")
        ws = _exact_ws(lib.gspn_ball_ws_bytes(b, n, m))
        assert lib.gspn_queryballpoint_ws(b, n, m, ctypes.c_float(radius), ns, _p(t_xyz), _p(t_q), _p(ws), _p(idx), _p(cnt), _st()) == 0
        return idx, cnt
    return Case("gspn_queryballpoint_ws n=8229 (ragged tail after the prefix)", run, note="called through ctypes")


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
MASKED = {"fps_cells_return_order", "fps_cells_return_cell_order", "inverse_lists_lds", "inverse_lists_global_32769", "inverse_lists_global_40001"}


@pytest.mark.parametrize("build", CASES, ids=lambda f: f.__name__)
def test_arena(build):
    c = build()
    assert c.masked == (build.__name__ in MASKED), "MASKED above lists the rows that carry a mask or a canonical form, and only those"
    sweep(c)


def test_twin_of_the_harness_self_test_on_the_device():
    """tests/test_cpu_arena.py's first three items with torch ops on the device; the stray store lands inside the arena, nothing faults"""
    from tests.arena import Arena, GuardError, bits
    for off, want in ((0, "after, +0..+3"), (-1, "before, -4..-1"), (63, "after, +252..+255")):
        with Arena(0xFF) as a:
            out = torch.empty(5, 7, device="cuda")
            out.as_strided((1,), (1,), out.storage_offset() + (35 + off if off >= 0 else off)).view(torch.uint8).fill_(0x5A)
            with pytest.raises(GuardError) as e:
                a.check()
        assert want in str(e.value) and "test_gpu_arena_geometry.py" in str(e.value) and "(5, 7) float32" in str(e.value)
    x = torch.arange(12, dtype=torch.float32, device="cuda")

    def accumulates():
        out = torch.empty_like(x)
        out += x
        return out
    got = {}
    for fill in (0x00, 0xFF):
        with Arena(fill) as a:
            got[fill] = accumulates()
            a.check()
    assert torch.equal(got[0x00], x) and not torch.equal(bits(got[0x00]), bits(got[0xFF]))
    with pytest.raises(AssertionError, match="read memory it did not write"):
        sweep(Case("accumulates", accumulates))
    sweep(Case("overwrites", lambda: torch.mul(x, 2.0, out=torch.empty_like(x))))
    for fill in (0x00, 0xFF, 0x7F):
        with Arena(fill) as a:
            z, f = torch.zeros(3, 5, device="cuda"), torch.full((7,), 3, dtype=torch.int32, device="cuda")
            host = torch.empty(1, dtype=torch.int32, pin_memory=True)
            assert a.check() == 2 and host.is_pinned()
        assert not bool(z.any()) and bool((f == 3).all())
        for r in a.records:
            raw = r.arena.view(torch.uint8)
            assert bool((raw[:256] == fill).all()) and bool((raw[-256:] == fill).all())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(RuntimeError, match="capture"):
            Arena(0x00).__enter__()
        x + 1                                   # (a capture must record something)
    assert torch.empty.__module__ != "tests.arena"      # the refused open patched nothing


def test_zz_masked_cases():
    print("\ntests/test_gpu_arena_geometry.py: %d cases, %d masked" % (len(CASES), len(MASKED)))
    assert MASKED <= {f.__name__ for f in CASES}
