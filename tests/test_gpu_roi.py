"""GPU tests of the ROI stage (gspn_amd/roi.py on csrc/roi.hip): nms_3d equal to the outputs of the reference's own function
(tests/golden/roi/nms3d_ref.npz) and to its restatement, the inside-point counts and samples equal to fp32 restatements driven by the same
generator, the detection targets equal to the restatement and agreeing with float64 away from the 0.5 threshold, points_cropping equal to a
torch.gather restatement with gradients within 1e-5 of float64 autograd, and the training and inference chains captured in a graph."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import roi_ref as RR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi", "nms3d_ref.npz")
ROOM = torch.tensor(RR.ROOM)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@functools.lru_cache(maxsize=None)
def scene():
    return RR.target_scene()


def config(nsmp=256, rois=64):
    from gspn_amd.rpointnet import Config
    cfg = Config()
    cfg.NUM_POINT_INS_MASK, cfg.TRAIN_ROIS_PER_IMAGE = nsmp, rois
    return cfg


def dev_seed(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


# ---- nms_3d ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(RR.NMS_CASES))
def test_nms_3d_equals_the_reference_function(name):
    from gspn_amd.rpointnet import nms_3d
    z = np.load(GOLDEN)
    pre, m, thr, sthr = z[name + "/args"].tolist()
    boxes, scores = torch.from_numpy(z[name + "/boxes"]), torch.from_numpy(z[name + "/scores"])
    got = nms_3d(boxes.cuda(), scores.cuda(), int(pre), int(m), thr, sthr)
    assert got.dtype == torch.int32 and got.is_cuda and got.shape == (boxes.shape[0], int(m))
    assert torch.equal(got.cpu(), torch.from_numpy(z[name + "/selected"]))


@pytest.mark.parametrize("b,n,pre,m,thr,zero_rows", [(8, 256, 192, 128, 0.5, 5), (8, 2048, 1536, 384, 0.1, 0), (2, 4096, 3000, 512, 0.5, 0),
                                                     (1, 4096, -1, 384, 0.25, 64), (3, 1, -1, 4, 0.5, 0), (2, 65, 64, 70, 0.3, 0)])
def test_nms_3d_equals_the_restatement(b, n, pre, m, thr, zero_rows):
    from gspn_amd.rpointnet import nms_3d
    boxes, scores = RR.nms_boxes(b, n, 1000 + n + b, zero_rows)
    for row in scores:
        assert row.unique().numel() == n
    got = nms_3d(boxes.cuda(), scores.cuda(), pre, m, thr).cpu()
    assert torch.equal(got, RR.nms_3d(boxes, scores, pre, m, thr))


def test_nms_3d_ties_thresholds_and_limits():
    from gspn_amd.rpointnet import nms_3d
    # equal scores: the lower index first
    boxes = torch.tensor([[[0.0, 0, 0, 1, 1, 1], [5.0, 0, 0, 1, 1, 1], [10.0, 0, 0, 1, 1, 1], [0.1, 0, 0, 1, 1, 1]]])
    scores = torch.tensor([[0.5, 0.9, 0.5, 0.5]])
    assert nms_3d(boxes.cuda(), scores.cuda(), -1, 4).cpu().tolist() == [[1, 0, 2, -1]]
    # many equal scores among 512 boxes, a finite score threshold and negative scores
    bx, sc = RR.nms_boxes(2, 512, 5)
    sc = (torch.floor(sc * 16) / 16 - 0.5).contiguous()
    for sthr in (float("-inf"), -0.2, 0.3):
        want = RR.nms_3d(bx, sc, 400, 200, 0.4, sthr)
        assert torch.equal(nms_3d(bx.cuda(), sc.cuda(), 400, 200, 0.4, sthr).cpu(), want)
    with pytest.raises(NotImplementedError):
        nms_3d(torch.zeros(1, 4097, 6, device="cuda"), torch.zeros(1, 4097, device="cuda"), -1, 8)
    with pytest.raises(ValueError):
        nms_3d(torch.zeros(1, 4, 5, device="cuda"), torch.zeros(1, 4, device="cuda"), -1, 8)
    with pytest.raises(ValueError):
        nms_3d(torch.zeros(1, 4, 6, device="cuda"), torch.zeros(1, 4, device="cuda"), -1, 0)


# ---- counts and samples ------------------------------------------------------------------------------------------------------------

def count_case(b, s, n, seed, margin):
    """random boxes in a random cloud, plus: an empty box, all-zero rows, a box with ONE point exactly on its upper face (margin
    included, so c + s/2 + margin is the point's own coordinate in fp32) and one with a point just outside that face"""
    g = torch.Generator().manual_seed(seed)
    pc = torch.rand(b, n, 3, generator=g) * ROOM
    box = torch.cat((torch.rand(b, s, 3, generator=g) * ROOM, torch.rand(b, s, 3, generator=g) * 1.5 + 0.05), -1)
    m = torch.tensor(margin, dtype=torch.float32)
    face = (torch.tensor([70.0, 69.75, 70.25]) + 0.5) + m                 # the upper corner of box 3, as the kernel computes it
    pc[:, 0] = face
    pc[:, 1] = face - torch.tensor([0.0, 0.25, 0.25])
    pc[:, 1, 0] = torch.nextafter(face[0], torch.tensor(float("inf")))                         # x just outside box 3
    box[:, 0] = torch.tensor([100.0, 100.0, 100.0, 1.0, 1.0, 1.0])        # empty
    box[:, 1] = 0.0
    box[:, 2] = 0.0
    box[:, 3] = torch.tensor([70.0, 69.75, 70.25, 1.0, 1.0, 1.0])
    box[:, s - 1] = 0.0
    return box.contiguous(), pc.contiguous()


@pytest.mark.parametrize("margin", [0.0, 1e-3])
@pytest.mark.parametrize("b,s,n", [(2, 128, 18000), (2, 512, 18000), (1, 5, 7), (3, 13, 1000)])
def test_box_point_count_bit_equal(b, s, n, margin):
    from gspn_amd.rpointnet import box_point_count
    box, pc = count_case(b, s, n, 3 * s + n, margin)
    got = box_point_count(box.cuda(), pc.cuda(), margin)
    want = RR.box_point_count(box, pc, margin)
    assert got.dtype == torch.int32 and got.shape == (b, s)
    assert torch.equal(got.cpu(), want)
    assert (want[:, 0] == 0).all() and (want[:, 3] == 1).all()            # the point on the face is inside, its neighbour is not
    if n >= 1000:
        assert int((want[:, 4:] > 0).sum()) > s // 2 and int((want[:, 4:] == 0).sum()) > 0


@pytest.mark.parametrize("margin", [0.0, 1e-3])
@pytest.mark.parametrize("b,r,n,nsmp", [(2, 64, 18000, 256), (1, 24, 32768, 1024), (2, 9, 100, 7), (1, 5, 3, 300)])
def test_sample_points_in_boxes(b, r, n, nsmp, margin):
    from gspn_amd.rpointnet import box_point_count, sample_points_in_boxes
    box, pc = count_case(b, r, n, 11 * r + n, margin)
    bx, p = box.cuda(), pc.cuda()
    got = sample_points_in_boxes(bx, p, nsmp, dev_seed(42), margin)
    assert got.dtype == torch.int32 and got.shape == (b, r, nsmp)
    assert torch.equal(got.cpu(), RR.sample_points_in_boxes(box, pc, nsmp, 42, margin))
    assert torch.equal(sample_points_in_boxes(bx, p, nsmp, 42, margin), got)                  # a Python int seed is the same seed
    assert torch.equal(sample_points_in_boxes(bx, p, nsmp, dev_seed(42), margin), got)        # two calls with one seed agree
    other = sample_points_in_boxes(bx, p, nsmp, dev_seed(43), margin)
    cnt = box_point_count(bx, p, margin).cpu()
    zero = (cnt == 0) | (box.abs().sum(-1) == 0)
    assert not got.cpu()[zero].any() and not other.cpu()[zero].any()                          # rows of zeros where nothing can be drawn
    many = (cnt > 1) & ~zero
    if many.any():
        assert not torch.equal(other.cpu()[many], got.cpu()[many])                            # two seeds differ
    for i in range(b):                                                                        # every index is inside its box
        for k in torch.nonzero(~zero[i])[:, 0]:
            members = RR.inside(box[i, k:k + 1], pc[i], margin)[0]
            assert members[got[i, k].cpu().long()].all() and members[other[i, k].cpu().long()].all()


def test_sample_points_in_boxes_draws_are_spread():
    """4096 draws over a box of 37 points: every point is drawn, none more than three times its share"""
    from gspn_amd.rpointnet import sample_points_in_boxes
    g = torch.Generator().manual_seed(1)
    pc = torch.rand(1, 5000, 3, generator=g) * ROOM + 10.0
    pc[0, torch.randperm(5000, generator=g)[:37]] = torch.rand(37, 3, generator=g)            # 37 points in the unit cube
    box = torch.tensor([[[0.5, 0.5, 0.5, 1.0, 1.0, 1.0]]])
    got = sample_points_in_boxes(box.cuda(), pc.cuda(), 4096, 7).cpu().long().reshape(-1)
    hist = torch.bincount(got, minlength=5000)
    assert int((hist > 0).sum()) == 37 and int(hist.max()) < 3 * 4096 // 37
    with pytest.raises(NotImplementedError):
        sample_points_in_boxes(box.cuda(), torch.zeros(1, 32769, 3, device="cuda"), 4, 0)
    with pytest.raises(ValueError):
        sample_points_in_boxes(box.cuda(), pc.cuda(), 4, torch.zeros(2, dtype=torch.int64, device="cuda"))


# ---- targets -----------------------------------------------------------------------------------------------------------------------

def check_target_structure(prop, cnt, gt_boxes, roi_src, roi_gt, rois_per_image=64, ratio=0.33):
    """positives first, then negatives, then padding; the counts obey the two formulas; no source repeated; every positive has IoU >= 0.5
    with its roi_gt, which is its arg-max; no ROI is empty or a zero row"""
    for i in range(prop.shape[0]):
        src, rgt = roi_src[i], roi_gt[i]
        nrow, npos = int((src >= 0).sum()), int((rgt >= 0).sum())
        assert (src[:nrow] >= 0).all() and (src[nrow:] == -1).all() and (rgt[:npos] >= 0).all() and (rgt[npos:] == -1).all() and npos <= nrow
        used = src[:nrow].long()
        assert used.unique().numel() == nrow
        assert (cnt[i][used] > 0).all() and (prop[i][used].abs().sum(1) > 0).all()
        part = (prop[i].abs().sum(1) > 0) & (cnt[i] > 0)
        valid = gt_boxes[i].abs().sum(1) > 0
        m = RR.ious(prop[i], gt_boxes[i])
        m[:, ~valid] = float("-inf")
        best = m.max(1).values if valid.any() else torch.full((prop.shape[1],), float("-inf"))
        want_pos, want_neg = RR.selection_counts(int(((best >= 0.5) & part).sum()), int(((best < 0.5) & part).sum()), rois_per_image, ratio)
        assert (npos, nrow - npos) == (want_pos, want_neg)
        for k in range(npos):
            row, j = m[used[k]], int(rgt[k])
            assert row[j] >= 0.5 and row[j] == row.max() and int(torch.nonzero(row == row.max())[0]) == j
        assert (best[used[npos:]] < 0.5).all()


@pytest.mark.parametrize("mix", sorted(RR.TARGET_MIXES))
def test_detection_target_select(mix):
    from gspn_amd.roi import box_point_count, detection_target_select
    sc = scene()
    s, njit = RR.TARGET_MIXES[mix]
    gt = sc["bbox_ins"]
    for seed in (3, 4):
        prop = RR.target_proposals(gt, s, njit, 100 + seed)
        cnt = box_point_count(prop.cuda(), sc["pc"].cuda())
        assert torch.equal(cnt.cpu(), RR.box_point_count(prop, sc["pc"]))
        roi_src, roi_gt = detection_target_select(prop.cuda(), cnt, sc["gt_class_ids"].cuda(), gt.cuda(), 64, 0.33, dev_seed(seed))
        want_src, want_gt, iou32 = RR.detection_target_select(prop, cnt.cpu(), gt, 64, 0.33, seed)
        assert roi_src.dtype == torch.int32 and roi_gt.dtype == torch.int32 and roi_src.shape == (2, 64) and roi_gt.shape == (2, 64)
        assert torch.equal(roi_src.cpu(), want_src) and torch.equal(roi_gt.cpu(), want_gt)
        check_target_structure(prop, cnt.cpu(), gt, roi_src.cpu(), roi_gt.cpu())
        # the fp32 decisions against float64, where the largest IoU is farther than 1e-5 from 0.5: at most 1 % of a scene is left out
        _, _, iou64 = RR.detection_target_select(prop, cnt.cpu(), gt, 64, 0.33, seed, torch.float64)
        part = ~torch.isnan(iou64)
        near = ((iou64 - 0.5).abs() <= 1e-5) & part
        assert int(near.sum(1).max()) <= s // 100
        if not near.any():
            src64, gt64, _ = RR.detection_target_select(prop, cnt.cpu(), gt, 64, 0.33, seed, torch.float64)
            assert torch.equal(roi_src.cpu(), src64) and torch.equal(roi_gt.cpu(), gt64)
        got_pos = torch.zeros_like(part)
        for i in range(2):
            got_pos[i][roi_src[i].cpu()[roi_gt[i].cpu() >= 0].long()] = True
        assert not (got_pos & ~near & ~(iou64 >= 0.5)).any()                                   # no fp32 positive is a float64 negative
        other = detection_target_select(prop.cuda(), cnt, sc["gt_class_ids"].cuda(), gt.cuda(), 64, 0.33, dev_seed(seed + 10))[0]
        assert not torch.equal(other, roi_src)


def test_detection_target_select_without_ground_truth_and_limits():
    """no ground-truth box takes part: reduce_max over an empty axis, every proposal that takes part is negative -- and none is taken,
    since the number of negatives follows the number of positives"""
    from gspn_amd.roi import box_point_count, detection_target_select
    sc = scene()
    prop = RR.target_proposals(sc["bbox_ins"], 128, 88, 1).cuda()
    cnt = box_point_count(prop, sc["pc"].cuda())
    gt = sc["bbox_ins"].clone()
    gt[0] = 0.0
    roi_src, roi_gt = detection_target_select(prop, cnt, sc["gt_class_ids"].cuda(), gt.cuda(), 64, 0.33, 5)
    assert (roi_src[0] == -1).all() and (roi_gt[0] == -1).all() and int((roi_gt[1] >= 0).sum()) == 21
    want_src, want_gt, _ = RR.detection_target_select(prop.cpu(), cnt.cpu(), gt, 64, 0.33, 5)
    assert torch.equal(roi_src.cpu(), want_src) and torch.equal(roi_gt.cpu(), want_gt)
    # other sizes and ratios, rows past rois_per_image dropped
    for r, ratio in ((16, 0.5), (200, 0.25), (8, 0.9)):
        a, b = detection_target_select(prop, cnt, sc["gt_class_ids"].cuda(), sc["bbox_ins"].cuda(), r, ratio, 6)
        wa, wb, _ = RR.detection_target_select(prop.cpu(), cnt.cpu(), sc["bbox_ins"], r, ratio, 6)
        assert torch.equal(a.cpu(), wa) and torch.equal(b.cpu(), wb)
    with pytest.raises(NotImplementedError):
        detection_target_select(torch.zeros(1, 1025, 6, device="cuda"), torch.zeros(1, 1025, dtype=torch.int32, device="cuda"),
                                torch.zeros(1, 4, device="cuda"), torch.zeros(1, 4, 6, device="cuda"), 64, 0.33, 0)


@pytest.mark.parametrize("mix", sorted(RR.TARGET_MIXES))
def test_detection_target_gen_batch(mix):
    from gspn_amd import rpointnet as RP
    from gspn_amd.roi import box_point_count, detection_target_select
    sc = scene()
    cfg = config()
    s, njit = RR.TARGET_MIXES[mix]
    gt, cls, lab, pc = sc["bbox_ins"], sc["gt_class_ids"], sc["group_label"], sc["pc"]
    prop = RR.target_proposals(gt, s, njit, 103)
    seed = dev_seed(21)
    rois, tcls, tbox, idx, mask = RP.detection_target_gen_batch(prop.cuda(), cls.cuda(), gt.cuda(), lab.cuda(), pc.cuda(), cfg, seed)
    assert rois.shape == (2, 64, 6) and tcls.shape == (2, 64) and tbox.shape == (2, 64, 6) and idx.shape == (2, 64, 256) and mask.shape == (2, 64, 256)
    assert tcls.dtype == cls.dtype and idx.dtype == torch.int32 and mask.dtype == torch.bool and tbox.dtype == torch.float32
    cnt = box_point_count(prop.cuda(), pc.cuda())
    roi_src, roi_gt = detection_target_select(prop.cuda(), cnt, cls.cuda(), gt.cuda(), 64, 0.33, seed)
    roi_src, roi_gt = roi_src.cpu(), roi_gt.cpu()
    pos = roi_gt >= 0
    pos_rois = RR.take_rows(prop, roi_src) * pos.unsqueeze(-1)
    want_idx = RR.sample_points_in_boxes(pos_rois, pc, 256, 21)
    assert torch.equal(idx.cpu(), want_idx)
    want_rois, want_cls, want_box, want_mask = RR.detection_targets(prop, cls, gt, lab, pc, roi_src, roi_gt, want_idx, cfg.BBOX_STD_DEV)
    assert torch.equal(rois.cpu(), want_rois) and torch.equal(tcls.cpu(), want_cls) and torch.equal(mask.cpu(), want_mask)
    err = (tbox.cpu().double() - want_box).abs().max()
    print("target_bbox: max |fp32 - float64| = %.3g (max |value| %.3g)" % (float(err), float(want_box.abs().max())))
    assert float(err) <= 1e-5
    # rows of negatives and padding are zero; the masks of the positives are neither empty nor full everywhere
    assert not tbox.cpu()[~pos].any() and not idx.cpu()[~pos].any() and not mask.cpu()[~pos].any() and not tcls.cpu()[~pos].any()
    assert not rois.cpu()[roi_src < 0].any() and mask.cpu()[pos].any() and not mask.cpu()[pos].all()
    # the per-scene wrappers equal the batch form row by row
    onehot = (lab.unsqueeze(-1) == torch.arange(100)).float()
    for i in range(2):
        # the generator's stream is the scene's position in its batch and the wrapper is a batch of one: it is compared with the batch
        # form on that scene alone, and for scene 0 with the batch of two as well
        out = RP.detection_target_gen(prop[i].cuda(), cls[i].cuda(), gt[i].cuda(), onehot[i].cuda(), pc[i].cuda(), cfg, seed)
        one = RP.detection_target_gen_batch(prop[i:i + 1].cuda(), cls[i:i + 1].cuda(), gt[i:i + 1].cuda(), lab[i:i + 1].cuda(), pc[i:i + 1].cuda(), cfg, seed)
        assert out[0].shape == (64, 6) and out[3].shape == (64, 256) and out[4].dtype == torch.bool and bool(out[4].any())
        for got, want in zip(out, one):
            assert torch.equal(got, want[0])
        if i == 0:
            for got, want in zip(out, (rois, tcls, tbox, idx, mask)):
                assert torch.equal(got, want[0])


@pytest.mark.parametrize("empty_removal", [True, False])
def test_mask_selection_gen_batch(empty_removal):
    from gspn_amd import rpointnet as RP
    sc = scene()
    cfg = config(nsmp=128)
    pc = sc["pc"]
    prop = RR.target_proposals(sc["bbox_ins"], 384, 200, 9)
    for num_rois in (384, 96, 500):
        rois, idx = RP.mask_selection_gen_batch(prop.cuda(), pc.cuda(), num_rois, cfg, empty_removal, dev_seed(5))
        assert rois.shape == (2, num_rois, 6) and idx.shape == (2, num_rois, 128) and idx.dtype == torch.int32
        rows = RR.mask_selection_rows(prop, pc, num_rois, empty_removal)
        kept = (rows >= 0).sum(1)
        assert (kept < 384).all() and (kept > 40).all()
        want_rois = RR.take_rows(prop, rows)
        assert torch.equal(rois.cpu(), want_rois)
        assert torch.equal(idx.cpu(), RR.sample_points_in_boxes(want_rois, pc, 128, 5, 1e-3))
    cnt = RR.box_point_count(prop, pc, 1e-3)
    assert int(((cnt == 0) & (prop.abs().sum(-1) > 0)).sum()) > 50                             # there are empty proposals to remove
    r0, i0 = RP.mask_selection_gen(prop[0].cuda(), pc[0].cuda(), 384, cfg, empty_removal, dev_seed(5))
    rois, idx = RP.mask_selection_gen_batch(prop.cuda(), pc.cuda(), 384, cfg, empty_removal, dev_seed(5))
    assert torch.equal(r0, rois[0]) and torch.equal(i0, idx[0])


# ---- cropping ----------------------------------------------------------------------------------------------------------------------

def crop_case(b=2, n=18000, c=1024, r=64, p=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    pc = torch.rand(b, n, 3, generator=g) * ROOM
    fea = torch.randn(b, n, c, generator=g)
    cen = pc + 0.1 * torch.randn(b, n, 3, generator=g)
    rois = torch.cat((torch.rand(b, r, 3, generator=g) * ROOM, torch.rand(b, r, 3, generator=g) + 0.3), -1)
    rois[:, r - 5:] = 0.0                                                  # padding rows: size turned into ones
    idx = torch.randint(0, n, (b, r, p), generator=g).int()
    idx[:, 0] = 17                                                         # one point drawn 256 times by one ROI
    idx[:, r - 5:] = 0
    return pc, fea, cen, rois, idx


@pytest.mark.parametrize("normalize", [True, False])
def test_points_cropping_forward_and_gradients(normalize):
    from gspn_amd.rpointnet import points_cropping
    pc, fea, cen, rois, idx = crop_case()
    b, r, p = idx.shape
    want = RR.points_cropping(pc, fea, cen, rois, idx, normalize)
    fea_d, cen_d = fea.cuda().requires_grad_(True), cen.cuda().requires_grad_(True)
    got = points_cropping(pc.cuda(), fea_d, cen_d, rois.cuda(), idx.cuda(), r, p, normalize)
    assert len(got) == 4 and got[0].shape == (b, r, p, 1024) and got[1].shape == (b, r, p, 3)
    for a, w in zip(got, want):
        assert torch.equal(a.cpu(), w)
    g = torch.Generator().manual_seed(3)
    w_fea, w_cen = torch.randn(b, r, p, 1024, generator=g), torch.randn(b, r, p, 3, generator=g)

    def grads():
        fea_d.grad = cen_d.grad = None
        out = points_cropping(pc.cuda(), fea_d, cen_d, rois.cuda(), idx.cuda(), r, p, normalize)
        ((out[0] * w_fea.cuda()).sum() + (out[1] * w_cen.cuda()).sum()).backward()
        return fea_d.grad.clone(), cen_d.grad.clone()

    g_fea, g_cen = grads()
    fea64, cen64 = fea.double().requires_grad_(True), cen.double().requires_grad_(True)
    out64 = RR.points_cropping(pc.double(), fea64, cen64, rois.double(), idx, normalize)
    ((out64[0] * w_fea.double()).sum() + (out64[1] * w_cen.double()).sum()).backward()
    e_fea, e_cen = rel_err(g_fea, fea64.grad), rel_err(g_cen, cen64.grad)
    print("points_cropping gradients against float64: pc_fea %.3g, pc_center %.3g" % (e_fea, e_cen))
    assert e_fea <= 1e-5 and e_cen <= 1e-5
    g_fea2, g_cen2 = grads()
    assert torch.equal(g_fea, g_fea2) and torch.equal(g_cen, g_cen2)       # two backward calls give identical bits
    with pytest.raises(ValueError):
        points_cropping(pc.cuda(), fea_d, cen_d, rois.cuda(), idx.cuda(), r + 1, p, normalize)


# ---- the chains, captured ----------------------------------------------------------------------------------------------------------

def spn_like_proposals(sc, n, seed):
    """what SPN hands on: n boxes per scene around the ground truth (some far off, some degenerate after box_shrink) with distinct scores"""
    prop = RR.target_proposals(sc["bbox_ins"], n, (3 * n) // 4, seed)
    prop[..., 3:] += 1e-3 * (prop.abs().sum(-1, keepdim=True) > 0)         # box_shrink's 1e-3: no size is zero, though a wall's box is flat
    g = torch.Generator().manual_seed(seed)
    scores = torch.stack([(torch.randperm(n, generator=g).float() + 0.5) / n for _ in range(prop.shape[0])])
    scores = torch.where(prop.abs().sum(-1) > 0, scores, scores * 1e-5)   # a degenerate box has a low score: a zero row that is picked repeats
    for row in scores:
        assert row.unique().numel() == n
    return prop, scores.contiguous()


def test_training_chain_captured():
    from gspn_amd import rpointnet as RP
    from gspn_amd.graph import CapturedStep
    sc = scene()
    cfg = config()
    prop, scores = spn_like_proposals(sc, 256, 31)
    d = {k: sc[k].cuda() for k in ("pc", "bbox_ins", "gt_class_ids", "group_label")}
    prop_d, scores_d = prop.cuda(), scores.cuda()
    g = torch.Generator().manual_seed(2)
    fea = torch.randn(2, 18000, 128, generator=g).cuda().requires_grad_(True)
    cen = (sc["pc"] + 0.1 * torch.randn(2, 18000, 3, generator=g)).cuda().requires_grad_(True)
    seed = dev_seed(100)
    st = {}

    def step():
        fea.grad = cen.grad = None
        sel = RP.nms_3d(prop_d, scores_d, cfg.SPN_PRE_NMS_LIMIT, cfg.SPN_NMS_MAX_SIZE_TRAINING, cfg.SPN_IOU_THRESHOLD, cfg.SPN_SCORE_THRESHOLD)
        spn_rois = RP.gather_selection(prop_d, sel, cfg.SPN_NMS_MAX_SIZE_TRAINING)
        rois, tcls, tbox, idx, mask = RP.detection_target_gen_batch(spn_rois, d["gt_class_ids"], d["bbox_ins"], d["group_label"], d["pc"], cfg, seed)
        crop = RP.points_cropping(d["pc"], fea, cen, rois, idx, cfg.TRAIN_ROIS_PER_IMAGE, cfg.NUM_POINT_INS_MASK, cfg.NORMALIZE_CROP_REGION)
        loss = crop[0].square().sum() * 1e-3 + (crop[1] * crop[2]).sum()
        loss.backward()
        st["out"] = [sel, rois, tcls, tbox, idx, mask, crop[2].detach(), fea.grad, cen.grad]
        return loss.detach()

    loss0 = step().clone()
    out0 = [o.clone() for o in st["out"]]
    cap = CapturedStep(step)                                               # the capture itself proves that nothing synchronises with the host
    loss1 = cap.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(loss0) and torch.allclose(loss1, loss0, rtol=1e-6)
    for a, w in zip(st["out"], out0):
        assert torch.equal(a, w)                                           # the replay equals the eager run for the same seed
    sel0 = out0[0].cpu()
    assert torch.equal(sel0, RR.nms_3d(prop, scores, 192, 128, 0.5))
    assert float(out0[7].abs().max()) > 0 and float(out0[8].abs().max()) > 0
    spn_rois = RR.take_rows(prop, sel0.long())
    cnt = RR.box_point_count(spn_rois, sc["pc"])

    def check(out, seed_value):
        """rois as the restatement selects them for this seed, the structure of that selection, every sample inside its ROI"""
        roi_src, roi_gt, _ = RR.detection_target_select(spn_rois, cnt, sc["bbox_ins"], 64, 0.33, seed_value)
        check_target_structure(spn_rois, cnt, sc["bbox_ins"], roi_src, roi_gt)
        rois, idx = out[1].cpu(), out[4].cpu()
        assert torch.equal(rois, RR.take_rows(spn_rois, roi_src)) and int((roi_gt >= 0).sum()) >= 20
        for i in range(2):
            for k in range(64):
                if roi_gt[i, k] >= 0:
                    assert RR.inside(rois[i, k:k + 1], sc["pc"][i])[0][idx[i, k].long()].all() and idx[i, k].any()
                else:
                    assert not idx[i, k].any()

    check(out0, 100)
    seed.add_(1)                                                           # fresh draws on the next replay
    cap.replay()
    torch.cuda.synchronize()
    assert torch.equal(st["out"][0], out0[0])                              # NMS does not depend on the seed
    assert not torch.equal(st["out"][4], out0[4])
    check(st["out"], 101)
    eager = RP.detection_target_gen_batch(RP.gather_selection(prop_d, out0[0], 128), d["gt_class_ids"], d["bbox_ins"], d["group_label"], d["pc"],
                                          cfg, dev_seed(101))
    for a, w in zip(st["out"][1:6], eager):
        assert torch.equal(a, w)


def test_inference_chain_captured():
    from gspn_amd import rpointnet as RP
    from gspn_amd.graph import CapturedStep
    sc = scene()
    cfg = RP.Config(istrain=False)
    prop, scores = spn_like_proposals(sc, 2048, 32)
    pc_d, prop_d, scores_d = sc["pc"].cuda(), prop.cuda(), scores.cuda()
    g = torch.Generator().manual_seed(4)
    fea = torch.randn(2, 18000, 64, generator=g).cuda()
    cen = (sc["pc"] + 0.1 * torch.randn(2, 18000, 3, generator=g)).cuda()
    seed = dev_seed(7)
    m, nsmp = cfg.SPN_NMS_MAX_SIZE_INFERENCE, cfg.NUM_POINT_INS_MASK
    assert (cfg.NUM_SAMPLE, cfg.SPN_PRE_NMS_LIMIT, m, nsmp) == (2048, 1536, 384, 1024)
    st = {}

    def step():
        with torch.no_grad():
            sel = RP.nms_3d(prop_d, scores_d, cfg.SPN_PRE_NMS_LIMIT, m, cfg.SPN_IOU_THRESHOLD, cfg.SPN_SCORE_THRESHOLD)
            spn_rois = RP.gather_selection(prop_d, sel, m)
            rois, idx = RP.mask_selection_gen_batch(spn_rois, pc_d, m, cfg, True, seed)
            crop = RP.points_cropping(pc_d, fea, cen, rois, idx, m, nsmp, cfg.NORMALIZE_CROP_REGION)
        st["out"] = [sel, rois, idx, crop[0], crop[1], crop[2]]
        return crop[2].sum()

    step()
    out0 = [o.clone() for o in st["out"]]
    cap = CapturedStep(step)
    cap.replay()
    torch.cuda.synchronize()
    for a, w in zip(st["out"], out0):
        assert torch.equal(a, w)
    sel = RR.nms_3d(prop, scores, 1536, 384, 0.5)
    assert torch.equal(out0[0].cpu(), sel)
    spn_rois = RR.take_rows(prop, sel.long())
    rows = RR.mask_selection_rows(spn_rois, sc["pc"], 384)
    want_rois = RR.take_rows(spn_rois, rows)
    assert torch.equal(out0[1].cpu(), want_rois) and 40 < int((rows >= 0).sum(1).min()) and int((rows >= 0).sum(1).max()) < 384
    assert torch.equal(out0[2].cpu(), RR.sample_points_in_boxes(want_rois, sc["pc"], 1024, 7, 1e-3))
    seed.add_(1)
    cap.replay()
    torch.cuda.synchronize()
    assert torch.equal(st["out"][1], out0[1]) and not torch.equal(st["out"][2], out0[2])
    assert torch.equal(st["out"][2].cpu(), RR.sample_points_in_boxes(want_rois, sc["pc"], 1024, 8, 1e-3))
    want = RR.points_cropping(sc["pc"], fea.cpu(), cen.cpu(), want_rois, st["out"][2].cpu())
    for a, w in zip(st["out"][3:], want[:3]):
        assert torch.equal(a.cpu(), w)
