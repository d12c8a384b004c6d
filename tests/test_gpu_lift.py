"""GPU tests of gspn_amd/lift.py on the kernels of csrc/lift.hip against tests/lift_ref.py: gspn_lift_masks through ctypes and through its
wrapper (one vertex; below, at and past the vertex tile of both instantiations; ragged tiles; 32769 vertices, one past what nearest_in_sets
takes; the declined sizes), the planted cases of the definition, row offsets beyond 2^31, vertex_tables against the brute-force search,
the anchor -- scan_predictions on the scene's own points against scene_predictions, and the files of both --, and the stage behind
rpointnet_inference at V = 2 N.

Bounds: masks, counts and zeroed rows are equal; a confidence is within 4 V 2^-53 relative of the correctly rounded sums
(predict_ref.within_bound: exact non-negative terms, only the order of the additions differs); two calls give the same bits."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import lift_ref as LR
from tests import predict_ref as PR
from tests.test_gpu_predict import bits, cuda, read_tree

pytestmark = pytest.mark.gpu


def make_case(r, v, p, n, c, seed, full_row=True):
    """inputs of gspn_lift_masks, numpy: vertices uniform in the unit cube, boxes of varied sizes around vertices (row 0 around the whole
    cloud when full_row, row 1 around nothing, both of a valid class), crop points drawn from the vertices inside, classes in [0, c] --
    0 and c are dropped rows --, src anywhere in [0, n)"""
    rng = np.random.default_rng(seed)
    verts = rng.random((v, 3), dtype=np.float32)
    boxes = np.zeros((r, 6), np.float32)
    crops = np.zeros((r, p, 3), np.float32)
    cls = rng.integers(1, c, r).astype(np.int32)
    cls[rng.random(r) < 0.15] = 0
    cls[rng.random(r) < 0.05] = c
    for k in range(r):
        boxes[k, :3] = verts[rng.integers(v)]
        boxes[k, 3:] = (0.1 + 0.8 * rng.random()) * (0.5 + rng.random(3))
        if k == 0 and full_row:
            boxes[k], cls[k] = (0.5, 0.5, 0.5, 2, 2, 2), max(1, min(int(cls[k]), c - 1))
        if k == 1:
            boxes[k], cls[k] = (3, 3, 3, 0.5, 0.5, 0.5), max(1, min(int(cls[k]), c - 1))
        members = np.nonzero(LR.inside(verts, boxes[k]))[0]
        pool = members if len(members) else np.arange(v)
        crops[k] = verts[pool[rng.integers(len(pool), size=p)]]
    masks = (1.0 / (1.0 + np.exp(-2.5 * rng.standard_normal((r, p))))).astype(np.float32)
    sem = rng.random((n, c), dtype=np.float32) + np.float32(0.01)
    sem_prob = (sem / sem.sum(-1, keepdims=True)).astype(np.float32)
    return dict(verts=verts, crops=crops, boxes=boxes, masks=masks, class_ids=cls, src=rng.integers(0, n, v).astype(np.int32), sem_prob=sem_prob,
                vert_fb=(0.05 + 0.9 * rng.random(v)).astype(np.float32))


ORDER = ("verts", "crops", "boxes", "masks", "class_ids", "src", "sem_prob", "vert_fb")


def on_device(case):
    return {k: torch.from_numpy(case[k]).cuda() for k in ORDER}


def raw_call(dev, mask_th, part_fill):
    """gspn_lift_masks through ctypes, every output and the workspace pre-filled -> rc, (sem_conf, fb_conf, mask, mask_points), part"""
    from gspn_amd import _lib as L
    v, (r, p), (n, c) = dev["verts"].shape[0], dev["masks"].shape, dev["sem_prob"].shape
    need = int(L.lib().gspn_lift_part_doubles(r, v)) if r <= 65535 and v <= (1 << 24) else 0
    part = torch.full((max(need, 1),), part_fill, dtype=torch.float64, device="cuda")
    outs = [torch.full((r,), -7.0, dtype=torch.float64, device="cuda"), torch.full((r,), -7.0, dtype=torch.float64, device="cuda"),
            torch.full((r, v), 7, dtype=torch.uint8, device="cuda"), torch.full((r,), -7, dtype=torch.int32, device="cuda")]
    rc = L.lib().gspn_lift_masks(r, v, p, n, c, *[L.ptr(dev[k]) for k in ORDER], ctypes.c_double(mask_th), L.ptr(part), *[L.ptr(t) for t in outs],
                                 L.stream())
    torch.cuda.synchronize()
    return rc, outs, part


def check_against_the_definition(case, got, v, mask_th=0.4):
    want_sem, want_fb, want_mask, want_points = LR.lift(*[case[k] for k in ORDER], mask_th)
    sem_conf, fb_conf, mask, points = [t.cpu().numpy() for t in got]
    live = want_sem != 0
    print("largest relative error sem %.3g fb %.3g, bound %.3g" % (
        np.max(np.abs(sem_conf - want_sem)[live] / want_sem[live], initial=0), np.max(np.abs(fb_conf - want_fb)[live] / want_fb[live], initial=0),
        4.0 * v * 2.0 ** -53))
    assert np.array_equal(mask, want_mask) and np.array_equal(points, want_points)
    assert PR.within_bound(sem_conf, want_sem, v) and PR.within_bound(fb_conf, want_fb, v)
    c = case["sem_prob"].shape[1]
    dead = (case["class_ids"] <= 0) | (case["class_ids"] >= c)
    assert bits(sem_conf[dead]) == bits(np.zeros(int(dead.sum()))) == bits(fb_conf[dead]) and not mask[dead].any() and not points[dead].any()
    return want_sem, want_points


# (r, v, p, n, c): one vertex; V = T - 1, T, T + 1 at T = 256 (one vertex per lane) and at T = 1024 (four: r * ceil(v / 1024) >= 512);
# several tiles with a ragged last one; one vertex past the old limit of nearest_in_sets; the largest P
LIFT_SHAPES = [(1, 1, 1, 1, 2), (2, 255, 3, 7, 4), (2, 256, 3, 7, 4), (2, 257, 3, 7, 4), (512, 1023, 5, 33, 6), (512, 1024, 5, 33, 6),
               (512, 1025, 5, 33, 6), (3, 4099, 5, 257, 19), (5, 32769, 64, 1000, 19), (2, 700, 4096, 50, 19)]


@pytest.mark.parametrize("shape", LIFT_SHAPES)
def test_lift_masks_against_the_definition(shape):
    from gspn_amd import _lib as L
    from gspn_amd.lift import lift_masks, lift_tile
    r, v, p, n, c = shape
    case = make_case(*shape, seed=11 + v, full_row=v > 1)
    if shape == (1, 1, 1, 1, 2):
        case["boxes"][0], case["class_ids"][0] = (0.5, 0.5, 0.5, 2, 2, 2), 1
        case["crops"][0, 0] = case["verts"][0]
    assert lift_tile(r, v) == (1024 if r == 512 else 256)
    dev = on_device(case)
    rc, first, part = raw_call(dev, 0.4, float("nan"))
    assert rc == 0 and not bool(torch.isnan(part).any())                            # every slot of the workspace was written
    want_sem, want_points = check_against_the_definition(case, first, v)
    if v > 1:
        assert want_points[0] > 0 and want_sem[0] > 0 and want_points[1] == 0 and want_sem[1] == 0      # the full row, the empty row
        inside = np.array([LR.inside(case["verts"], b).sum() for b in case["boxes"]])
        assert inside[0] == v and (r < 3 or bool(((inside > 0) & (inside < v)).any()))
    rc, second, _ = raw_call(dev, 0.4, 3e38)                                        # other leftovers in the workspace: the same bits
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(first, second))
    wrapped = lift_masks(**dev)
    assert [t.dtype for t in wrapped] == [torch.float64, torch.float64, torch.uint8, torch.int32]
    assert [tuple(t.shape) for t in wrapped] == [(r,), (r,), (r, v), (r,)] and all(torch.equal(a, b) for a, b in zip(first, wrapped))
    if shape == (5, 32769, 64, 1000, 19):                                           # the size the unfused path declines
        idx = torch.full((1, r, v), -7, dtype=torch.int32, device="cuda")
        rc = L.lib().gspn_nearest_in_sets(1, r, v, p, L.ptr(dev["verts"]), L.ptr(dev["crops"]), L.ptr(dev["boxes"]), L.ptr(idx), L.stream())
        torch.cuda.synchronize()
        assert rc == -2 and bool((idx == -7).all())
        rc = L.lib().gspn_nearest_in_sets(1, r, v - 1, p, L.ptr(dev["verts"]), L.ptr(dev["crops"]), L.ptr(dev["boxes"]), L.ptr(idx), L.stream())
        torch.cuda.synchronize()
        assert rc == 0


@pytest.mark.parametrize("shape", [(2, 257, 3, 7, 4), (512, 1025, 5, 33, 6)])           # one vertex per lane; four: 512 * ceil(1025 / 1024) >= 512
def test_lift_masks_is_nearest_in_sets_behind_the_threshold(shape):
    """The two entry points over the shared tile (csrc/inbox_nearest.h), against each other and without a tolerance: for the rows of a
    valid class, mask[k][i] is idx[k][i] >= 0 and float64(masks[k][idx[k][i]]) > mask_th with idx = gspn_nearest_in_sets(b = 1, ...) on the
    same arrays, and mask_points[k] is that row's sum.  Row 0 holds every vertex and row 1 none, so that each instantiation sees a tile
    of more than 128 inside vertices (one lane per vertex), one of exactly 1 (the vertex past the first tile, 64 lanes for it) and
    one of 0."""
    from gspn_amd import _lib as L
    from gspn_amd.lift import lift_tile
    r, v, p, n, c = shape
    tile = lift_tile(r, v)
    assert tile == (1024 if r == 512 else 256)
    case = make_case(*shape, seed=29 + v, full_row=True)
    valid = (case["class_ids"] > 0) & (case["class_ids"] < c)
    assert valid[0] and valid[1]
    inside = np.stack([LR.inside(case["verts"], b) for b in case["boxes"]])[valid]            # (valid rows, v)
    per_tile = np.concatenate([inside[:, at:at + tile].sum(1) for at in range(0, v, tile)])
    assert (per_tile > 128).any() and (per_tile == 1).any() and (per_tile == 0).any()
    dev = on_device(case)
    idx = torch.full((1, r, v), -7, dtype=torch.int32, device="cuda")
    rc = L.lib().gspn_nearest_in_sets(1, r, v, p, L.ptr(dev["verts"]), L.ptr(dev["crops"]), L.ptr(dev["boxes"]), L.ptr(idx), L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    idx = idx[0].cpu().numpy()
    assert idx.min() >= -1 and idx.max() < p
    rc, (_, _, mask, points), _ = raw_call(dev, 0.4, float("nan"))
    assert rc == 0
    want = (idx >= 0) & (np.take_along_axis(case["masks"], np.maximum(idx, 0), 1).astype(np.float64) > 0.4)
    assert np.array_equal(mask.cpu().numpy()[valid], want[valid].astype(np.uint8))
    assert np.array_equal(points.cpu().numpy()[valid], want[valid].sum(1).astype(np.int32))


def test_lift_masks_declines_what_it_does_not_take():
    from gspn_amd.lift import lift_masks
    case = make_case(2, 300, 4097, 9, 4, seed=3)
    rc, outs, part = raw_call(on_device(case), 0.4, 5.0)
    assert rc == -2                                                                 # GSPN_ERR_UNSUPPORTED, P = 4097
    assert bool((outs[0] == -7).all() and (outs[1] == -7).all() and (outs[2] == 7).all() and (outs[3] == -7).all() and (part == 5.0).all())
    with pytest.raises(NotImplementedError, match="P <= 4096"):
        lift_masks(**on_device(case))
    big = make_case(1, 4, 2, 3, 3, seed=4)
    dev = on_device(big)
    v = (1 << 24) + 1
    dev["verts"] = torch.zeros((v, 3), device="cuda")
    dev["src"] = torch.zeros((v,), dtype=torch.int32, device="cuda")
    dev["vert_fb"] = torch.zeros((v,), device="cuda")
    rc, outs, _ = raw_call(dev, 0.4, 5.0)
    assert rc == -2 and bool((outs[0] == -7).all() and (outs[2] == 7).all() and (outs[3] == -7).all())      # V = 2^24 + 1: nothing launched
    with pytest.raises(NotImplementedError, match="V <= 16777216"):
        lift_masks(**dev)
    small = on_device(make_case(2, 10, 2, 3, 3, seed=5))
    rc, outs, _ = raw_call(small, float("nan"), 5.0)
    assert rc == -1 and bool((outs[2] == 7).all())                                  # GSPN_ERR_ARG: a NaN threshold


# ---- the planted cases ---------------------------------------------------------------------------------------------------------------------

def planted_case():
    """three tiles of 256 vertices, all far away but the planted ones; eight detections, four crop points each, five scene points, C = 4"""
    v, r, p, n, c = 768, 8, 4, 5, 4
    rng = np.random.default_rng(8)
    verts = (20 + rng.random((v, 3))).astype(np.float32)
    verts[:5] = [[0.375, 0.25, 0.0], [0.625, 0.75, 1.0], [0.3749999, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, 0.5, 0.5]]
    verts[300] = (6, 6, 6)
    verts[600:603] = [[-3.25, -3, -3], [-3, -3, -3], [-2.75, -3, -3]]
    verts[v - 1] = (3, 3, 3)
    box_a = (0.5, 0.5, 0.5, 0.25, 0.5, 1.0)
    boxes = np.array([box_a, (-9, -9, -9, 1, 1, 1), (3, 3, 3, 0.5, 0.5, 0.5), (6, 6, 6, 1, 1, 1), (6, 6, 6, 1, 1, 1), box_a, box_a,
                      (-3, -3, -3, 1, 1, 1)], np.float32)
    crops = (40 + rng.random((r, p, 3))).astype(np.float32)
    crops[0] = [[0.4, 0.3, 0.1], [0.6, 0.7, 0.9], [0.5, 0.5, 0.5], [0.45, 0.5, 0.6]]
    crops[3] = [[6.25, 6, 6], [5.75, 6, 6], [6, 6.5, 6], [6, 6, 7]]                 # two at the same distance of vertex 300
    crops[4] = [[6.125, 6, 6], [6.125, 6, 6], [9, 9, 9], [9, 9, 9]]                 # duplicated points
    crops[5] = crops[6] = crops[0]
    crops[7] = [[-3.25, -3, -3], [-3, -3, -3], [-2.75, -3, -3], [-8, -8, -8]]
    at = np.float32(0.4)
    masks = np.full((r, p), 0.75, np.float32)
    masks[0] = [0.9, 0.8, 0.7, 0.6]
    masks[3] = [0.25, 0.9, 0.9, 0.9]                                                 # the smaller j wins: 0.25, a clear byte
    masks[4] = [0.95, 0.125, 0.125, 0.125]
    masks[7] = [at, np.nextafter(at, np.float32(0)), np.nextafter(at, np.float32(1)), 0.5]
    cls = np.array([1, 2, 1, 3, 2, 0, c, 1], np.int32)
    src = rng.integers(0, n, v).astype(np.int32)
    src[0], src[1], src[300], src[601] = -1, n, -5, n + 7                            # clamped to 0 and n - 1
    sem = rng.random((n, c), dtype=np.float32)
    return dict(verts=verts, crops=crops, boxes=boxes, masks=masks, class_ids=cls, src=src, sem_prob=(sem / sem.sum(-1, keepdims=True)).astype(np.float32),
                vert_fb=(0.05 + 0.9 * rng.random(v)).astype(np.float32))


def test_lift_masks_planted_cases():
    case = planted_case()
    v, n = 768, 5
    assert float(case["masks"][7, 0]) > 0.4 > float(case["masks"][7, 1]) and not (case["masks"][7, 0] > np.float32(0.4))
    dev = on_device(case)
    rc, first, part = raw_call(dev, 0.4, float("nan"))
    assert rc == 0 and not bool(torch.isnan(part).any()) and part.numel() == 4 * 8 * 3
    check_against_the_definition(case, first, v)
    sem_conf, fb_conf, mask, points = [t.cpu().numpy() for t in first]
    set_at = lambda k: np.nonzero(mask[k])[0].tolist()                              # noqa: E731
    assert set_at(0) == [0, 1, 4]                                                   # on a face: inside; just outside and NaN: not
    assert points.tolist() == [3, 0, 1, 0, 1, 0, 0, 2]
    assert sem_conf[1] == 0 and fb_conf[1] == 0                                     # no vertex in the box: 0 / 1e-8
    assert set_at(2) == [v - 1]                                                     # the last lane of the last tile, two empty tiles before it
    assert set_at(3) == [] and sem_conf[3] > 0                                      # j = 0 of the two equal distances: 0.25, counted and not set
    g3 = float(np.float32(0.25))
    assert sem_conf[3] == (g3 * float(case["sem_prob"][0, 3])) / (1e-8 + g3)        # src -5 clamped to 0; one term: no rounding to argue about
    assert set_at(4) == [300] and fb_conf[4] == (float(np.float32(0.95)) * float(case["vert_fb"][300])) / (1e-8 + float(np.float32(0.95)))
    assert set_at(7) == [600, 602]                                                  # float32(0.4) is above the double 0.4, its lower neighbour is not
    # clamped src: the rows of scene points 0 and n - 1
    terms = [(0, 0), (1, n - 1), (4, int(case["src"][4]))]
    near = LR.nearest(case["verts"][[0, 1, 4]], case["crops"][0])
    g = case["masks"][0][near].astype(np.float64)
    s0, s1 = math.fsum(g.tolist()), math.fsum((g * case["sem_prob"][[t[1] for t in terms], 1].astype(np.float64)).tolist())
    assert PR.within_bound(sem_conf[0:1], np.array([s1 / (1e-8 + s0)]), v)
    rc, second, _ = raw_call(dev, 0.4, 3e38)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(first, second))
    # the threshold crosses as a double: at float32(0.4) itself nothing of row 7's first value is above it
    rc, third, _ = raw_call(dev, float(np.float32(0.4)), 0.0)
    assert rc == 0 and np.nonzero(third[2][7].cpu().numpy())[0].tolist() == [602]


# ---- row offsets beyond 2^31 ------------------------------------------------------------------------------------------------------------

def test_lift_masks_rows_beyond_2_to_the_31():
    """R * V > 2^31: every vertex far outside every box but a few planted per row, vertex V - 1 of row 1023 among them.  Checked on the
    device; the 2 GiB of masks stay there."""
    from gspn_amd.lift import lift_masks, lift_tile
    r, v, p, n, c = 1024, (1 << 21) + 3, 4, 64, 3
    assert r * v > 1 << 31 and lift_tile(r, v) == 1024
    gen = torch.Generator(device="cuda").manual_seed(5)
    verts = 5000 + torch.rand((v, 3), device="cuda", generator=gen)
    k = torch.arange(r, device="cuda")
    planted = [k * 2048 + k % 1000, v - 1 - (r - 1 - k), k * 1533 + 1001]          # three per row; row 1023 holds vertex V - 1
    assert int(planted[1][r - 1]) == v - 1 and len(set(torch.cat(planted).tolist())) == 3 * r
    for j, at in enumerate(planted):
        verts[at] = torch.stack((k.float(), torch.full_like(k, j).float() * 0.125, torch.zeros_like(k).float()), 1)
    boxes = torch.cat((k.float()[:, None], torch.zeros(r, 2, device="cuda"), torch.full((r, 3), 0.5, device="cuda")), 1)
    crops = boxes[:, None, :3] + torch.tensor([[0, 0, 0], [0, 0.125, 0], [0, 0.25, 0], [0.125, 0, 0.125]], device="cuda")[None]
    masks = torch.tensor([0.5, 0.75, 0.875, 0.125], device="cuda").expand(r, p).contiguous()            # vertex j of a row meets crop point j
    cls = (1 + k % 2).int()
    cls[5], cls[777] = 0, c                                                         # two dropped rows
    src = torch.randint(0, n, (v,), device="cuda", generator=gen).int()
    sem = torch.rand((n, c), device="cuda", generator=gen) + 0.1
    sem_prob = sem / sem.sum(-1, keepdim=True)
    vert_fb = 0.05 + 0.9 * torch.rand((v,), device="cuda", generator=gen)
    sem_conf, fb_conf, mask, points = lift_masks(verts, crops.contiguous(), boxes, masks, cls, src, sem_prob, vert_fb)
    live = (cls > 0) & (cls < c)
    assert torch.equal(points, torch.where(live, 3, 0).int()) and torch.equal(mask.sum(1, dtype=torch.int32), points)
    for at in planted:
        assert torch.equal(mask[k, at], live.to(torch.uint8))
    for row in (0, r - 1):
        want = torch.zeros(v, dtype=torch.uint8, device="cuda")
        want[torch.stack([at[row] for at in planted])] = 1
        assert torch.equal(mask[row], want)
    assert not bool(mask[5].any()) and not bool(mask[777].any()) and float(sem_conf[5]) == float(fb_conf[777]) == 0.0
    # the sums of the three planted terms, by hand on the host
    at = torch.stack(planted, 1).cpu().numpy()                                      # (r, 3)
    g = np.array([0.5, 0.75, 0.875])
    sem_h, fb_h, src_h, cls_h = sem_prob.cpu().numpy(), vert_fb.cpu().numpy(), src.cpu().numpy(), cls.cpu().numpy()
    want_sem, want_fb = np.zeros(r), np.zeros(r)
    for row in np.nonzero(live.cpu().numpy())[0]:
        s0 = math.fsum(g.tolist())
        want_sem[row] = math.fsum((g * sem_h[src_h[at[row]], cls_h[row]].astype(np.float64)).tolist()) / (1e-8 + s0)
        want_fb[row] = math.fsum((g * fb_h[at[row]].astype(np.float64)).tolist()) / (1e-8 + s0)
    assert PR.within_bound(sem_conf.cpu().numpy(), want_sem, v) and PR.within_bound(fb_conf.cpu().numpy(), want_fb, v)
    again = lift_masks(verts, crops.contiguous(), boxes, masks, cls, src, sem_prob, vert_fb)
    assert torch.equal(again[0], sem_conf) and torch.equal(again[1], fb_conf) and torch.equal(again[3], points)


# ---- vertex_tables ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cloud():
    """70 000 vertices and 18 000 scene points, of which the smaller cases take their first ones; 256 seeds; searched once on the host"""
    rng = np.random.default_rng(17)
    verts = rng.random((70000, 3), dtype=np.float32)
    pc = rng.random((18000, 3), dtype=np.float32)
    seeds = pc[rng.choice(18000, 256, replace=False)].copy()
    fb1 = (0.05 + 0.9 * rng.random(256)).astype(np.float32)
    fb_prob = np.stack((1 - fb1, fb1), -1).astype(np.float32)
    return verts, pc, seeds, fb_prob, {}


@pytest.mark.parametrize("n", [3, 1025, 18000])
@pytest.mark.parametrize("v", [1, 70000])
def test_vertex_tables_against_the_brute_force_search(cloud, v, n):
    from gspn_amd.lift import vertex_tables
    verts, pc, seeds, fb_prob, memo = cloud
    src, vert_fb = vertex_tables(torch.from_numpy(verts[:v]).cuda(), torch.from_numpy(pc[:n]).cuda(), torch.from_numpy(seeds).cuda(),
                                 torch.from_numpy(fb_prob).cuda())
    assert src.dtype == torch.int32 and vert_fb.dtype == torch.float32 and tuple(src.shape) == tuple(vert_fb.shape) == (v,)
    if n not in memo:                                                               # V = 1 is the first row of the larger search
        memo[n] = LR.vertex_tables(verts, pc[:n], seeds, fb_prob, search=LR.nearest_threads)
    want_src, want_fb = memo[n]
    assert np.array_equal(src.cpu().numpy(), want_src[:v]) and bits(vert_fb.cpu().numpy()) == bits(want_fb[:v])


def test_vertex_tables_ties_and_the_scene_s_own_points():
    from gspn_amd.inference import _point_probabilities
    from gspn_amd.lift import vertex_tables
    rng = np.random.default_rng(23)
    n = 3000
    pc = rng.random((n, 3), dtype=np.float32)
    assert len(np.unique(pc, axis=0)) == n
    seeds = pc[rng.choice(n, 64, replace=False)].copy()
    fb1 = rng.random(64).astype(np.float32)
    fb_prob = np.stack((1 - fb1, fb1), -1).astype(np.float32)
    dev = [torch.from_numpy(a).cuda() for a in (pc, seeds, fb_prob)]
    src, vert_fb = vertex_tables(dev[0], *dev)                                      # the scene's own, distinct points
    assert torch.equal(src, torch.arange(n, dtype=torch.int32, device="cuda"))
    table = _point_probabilities(dev[0][None], {"pc_seed": dev[1][None], "fb_prob": dev[2][None], "sem_class_logits": torch.zeros(1, n, 4, device="cuda")})
    assert torch.equal(vert_fb.view(torch.int32), table[0, :, 0].contiguous().view(torch.int32))
    # duplicated scene points: the first one wins, wherever the copies sit
    dup = pc.copy()
    dup[2000:2500] = dup[100:600]
    dup[2999] = dup[0]
    src, _ = vertex_tables(torch.from_numpy(dup).cuda(), torch.from_numpy(dup).cuda(), dev[1], dev[2])
    want = np.arange(n)
    want[2000:2500], want[2999] = np.arange(100, 600), 0
    assert np.array_equal(src.cpu().numpy(), want)
    for m in (3, 1025):                                                             # and in the two smaller kernels of three_nn
        few = dup[:m].copy()
        few[m - 1] = few[1]
        src, _ = vertex_tables(torch.from_numpy(few).cuda(), torch.from_numpy(few).cuda(), dev[1], dev[2])
        assert src.cpu().tolist() == list(range(m - 1)) + [1]


# ---- the anchor ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 100, 18000, 256, 19), (2, 7, 3001, 64, 19)])
def test_scan_predictions_on_the_scene_s_own_points_is_scene_predictions(shape, tmp_path):
    from gspn_amd.lift import scan_predictions
    from gspn_amd.predict import scene_predictions, write_predictions
    b, r, n, p, c = shape
    pc, ep = PR.stage_inputs(*shape, seed=41)                                       # tests/test_gpu_predict.py's score ladder
    assert all(len(np.unique(pc[i].numpy(), axis=0)) == n for i in range(b))        # pairwise distinct: src is the identity
    dev_pc, dev_ep = pc.cuda(), cuda(ep)
    whole = scene_predictions(dev_ep, dev_pc)
    for s in range(b):
        keys = set(dev_ep)
        got = scan_predictions(dev_ep, s, dev_pc[s], pc=dev_pc)
        assert set(dev_ep) == keys and set(got) == set(whole) | {"src"}
        assert torch.equal(got["src"], torch.arange(n, dtype=torch.int32, device="cuda"))
        for k in ("masks", "mask_points", "order", "count", "label_ids", "confidence"):
            assert got[k].dtype == whole[k].dtype and torch.equal(got[k][0], whole[k][s]), k
        assert tuple(got["masks"].shape) == (1, r, n) and tuple(got["count"].shape) == (1,)
        for k in ("sem_conf", "fb_conf", "score"):
            assert got[k].dtype == torch.float64 and PR.within_bound(got[k][0].cpu().numpy(), whole[k][s].cpu().numpy(), n), k
        assert int(got["count"][0]) > 0 and int((got["mask_points"][0] > 0).sum()) > 0
        ours, theirs = str(tmp_path / ("scan%d" % s)), str(tmp_path / ("scene%d" % s))
        os.makedirs(ours)
        os.makedirs(theirs)
        assert write_predictions(ours, "scene%04d_00" % s, got, 0) == write_predictions(theirs, "scene%04d_00" % s, whole, s) > 0
        a, w = read_tree(ours), read_tree(theirs)
        assert sorted(a) == sorted(w) and all(a[k] == w[k] for k in w)
        again = scan_predictions(dict(dev_ep, pc=dev_pc), s, dev_pc[s])             # pc as a key; a second call repeats the bits
        assert all(torch.equal(again[k], got[k]) for k in got)


# ---- behind rpointnet_inference -------------------------------------------------------------------------------------------------------------

def test_scan_predictions_behind_rpointnet_inference_at_twice_the_points():
    from gspn_amd import synth
    from gspn_amd.lift import lift_masks, scan_predictions, vertex_tables
    from gspn_amd.predict import SCANNET_LABEL_MAP, scene_predictions
    from tests import test_gpu_inference as TI
    run = TI.Run()
    label_map = SCANNET_LABEL_MAP[:TI.NCAT]
    pc, ep = run.sc["pc"], run.ep
    whole = scene_predictions(ep, pc, label_map=label_map)
    n = TI.N
    for s in range(TI.B):
        host_pc = pc[s].cpu().numpy()
        verts = synth.scan_vertices(host_pc, np.zeros(n, np.int32), np.zeros(n, np.int32), 2 * n, 50 + s)[0]
        dev_verts = torch.from_numpy(verts).cuda()
        got = scan_predictions(ep, s, dev_verts, pc=pc, label_map=label_map)
        assert tuple(got["masks"].shape) == (1, TI.D, 2 * n) and not any(t.requires_grad for t in got.values())
        # the device's own tables, then the definition on the host
        src, vert_fb = vertex_tables(dev_verts, pc[s], ep["pc_seed"][s], ep["fb_prob"][s])
        assert torch.equal(src, got["src"]) and torch.equal(src[:n], torch.arange(n, dtype=torch.int32, device="cuda"))
        want_src, want_fb = LR.vertex_tables(verts, host_pc, ep["pc_seed"][s].cpu().numpy(), ep["fb_prob"][s].cpu().numpy())
        assert np.array_equal(src.cpu().numpy(), want_src) and bits(vert_fb.cpu().numpy()) == bits(want_fb)
        sem_prob = torch.softmax(ep["sem_class_logits"], -1)[s].contiguous()
        det = ep["detections"][s]
        cls = det[:, 6].int()
        case = dict(verts=verts, crops=ep["pc_coord_cropped_final_unnormalized"][s].cpu().numpy(), boxes=det[:, :6].contiguous().cpu().numpy(),
                    masks=ep["rpointnet_mask_selected"][s].cpu().numpy(), class_ids=cls.cpu().numpy(), src=want_src, sem_prob=sem_prob.cpu().numpy(),
                    vert_fb=want_fb)
        plain = lift_masks(**on_device(case))
        check_against_the_definition(case, plain, 2 * n)
        order, count, label_ids, confidence, score = PR.rank(det[None, :, 7].cpu().numpy(), case["class_ids"][None], plain[0].cpu().numpy()[None],
                                                             plain[1].cpu().numpy()[None], seg_label_map=np.asarray(label_map))
        at = order[0]
        assert np.array_equal(got["order"].cpu().numpy(), order) and np.array_equal(got["count"].cpu().numpy(), count) and count[0] >= 4
        assert np.array_equal(got["label_ids"].cpu().numpy(), label_ids) and np.array_equal(got["confidence"].cpu().numpy(), confidence)
        assert bits(got["score"].cpu().numpy()) == bits(score)
        for k, t in (("sem_conf", plain[0]), ("fb_conf", plain[1]), ("masks", plain[2]), ("mask_points", plain[3])):
            assert torch.equal(got[k][0], t[torch.from_numpy(at).long().cuda()]), k
        # on the scene's own points the masks are the scene stage's, detection by detection (the orders may differ: the sums run over more)
        back = {int(row): j for j, row in enumerate(whole["order"][s].cpu().tolist())}
        pick = torch.tensor([back[int(row)] for row in at], device="cuda")
        assert torch.equal(got["masks"][0][:, :n], whole["masks"][s][pick])
        assert bool(got["masks"][0][:, n:].any())                                   # the added vertices take part
