"""The box and ROI stages, the export, evaluation and preparation stages and the training loop's kernels on poisoned, guard-banded
allocations (tests/arena.py; the table's rules are those of tests/test_gpu_arena_geometry.py).

Inputs come from the builders of the value tests of each stage (tests/test_gpu_roi.py, test_gpu_detect.py, test_gpu_spn_boxes.py,
test_gpu_predict.py, test_gpu_evaluate.py, test_gpu_data_prep.py, test_gpu_train.py) at their smallest shapes.  Every atomic in these
kernels adds integers, so every row is held to equal bits; no row is masked.  State updated in place (Adam moments, the device's step
counter, the running sums, the IoU accumulators) is created inside the case, through the patched allocators, and returned."""
import numpy as np
import pytest
import torch

from tests.arena import Case, sweep

pytestmark = pytest.mark.gpu

CASES = []


def case(fn):
    CASES.append(fn)
    return fn


def leaf(t):
    return t.detach().requires_grad_(True)


def cuda(*ts):
    return [t.cuda() for t in ts]


def dev_seed(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


def rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


# ---- roi.py / detect.py --------------------------------------------------------------------------------------------------------------
@case
def nms_3d():
    from gspn_amd.roi import nms_3d
    from tests import roi_ref as RR
    a = cuda(*RR.nms_boxes(2, 65, 1067, 0))
    b = cuda(*RR.nms_boxes(8, 256, 1264, 5))
    return Case("nms_3d (2, 65) pre 64 keep 70 and (8, 256) pre 192 keep 128 with zero rows",
                lambda: (nms_3d(a[0], a[1], 64, 70, 0.3), nms_3d(b[0], b[1], 192, 128, 0.5), nms_3d(a[0], a[1], -1, 4, 0.5)))


@case
def class_nms_3d():
    from gspn_amd.detect import class_nms_3d
    from tests import detect_ref as DR
    a = cuda(*DR.class_boxes(2, 65, 69, 2067, 2, (0,)))
    b = cuda(*DR.class_boxes(2, 384, 18, 2386, 4, ()))
    return Case("class_nms_3d (2, 65) 70 classes, one empty scene; (2, 384) 19 classes",
                lambda: (class_nms_3d(a[0], a[1], a[2], 3, 70, 0.3), class_nms_3d(b[0], b[1], b[2], 100, 100, 0.1)))


@case
def box_point_count():
    from gspn_amd.roi import box_point_count
    from tests.test_gpu_roi import count_case
    small = cuda(*count_case(1, 5, 7, 22, 0.0))
    eight = cuda(*count_case(2, 1020, 500, 3560, 1e-3))                    # b * ceil(s / 8) >= 256: eight boxes per workgroup, s no multiple of 8
    return Case("box_point_count (1, 5, 7) and (2, 1020, 500): four and eight boxes per workgroup",
                lambda: (box_point_count(small[0], small[1], 0.0), box_point_count(eight[0], eight[1], 1e-3)))


@case
def sample_points_in_boxes():
    from gspn_amd.roi import sample_points_in_boxes
    from tests.test_gpu_roi import count_case
    box, pc = cuda(*count_case(1, 5, 3, 58, 0.0))
    box2, pc2 = cuda(*count_case(2, 9, 100, 199, 1e-3))
    seed = dev_seed(42)
    return Case("sample_points_in_boxes (1, 5, 3, 300) and (2, 9, 100, 7)",
                lambda: (sample_points_in_boxes(box, pc, 300, seed, 0.0), sample_points_in_boxes(box2, pc2, 7, 42, 1e-3)))


@case
def detection_target_select():
    from gspn_amd.roi import box_point_count, detection_target_select
    from tests import roi_ref as RR
    from tests.test_gpu_roi import scene
    sc = scene()
    prop = RR.target_proposals(sc["bbox_ins"], 128, 88, 103).cuda()
    pc, cls, gt = cuda(sc["pc"], sc["gt_class_ids"], sc["bbox_ins"])
    no_gt = gt.clone()
    no_gt[0] = 0.0                                                          # a scene without ground truth
    seed = dev_seed(3)

    def run():
        cnt = box_point_count(prop, pc)
        return cnt, detection_target_select(prop, cnt, cls, gt, 64, 0.33, seed), detection_target_select(prop, cnt, cls, no_gt, 64, 0.33, 5)
    return Case("detection_target_select 128 proposals, 64 ROIs; one scene without ground truth", run)


@case
def detection_target_and_mask_selection_batches():
    from gspn_amd import roi
    from tests import roi_ref as RR
    from tests.test_gpu_roi import config, scene
    sc = scene()
    prop = RR.target_proposals(sc["bbox_ins"], 128, 88, 104).cuda()
    pc, cls, gt, group = cuda(sc["pc"], sc["gt_class_ids"], sc["bbox_ins"], sc["group_label"])
    cfg = config(nsmp=64, rois=16)
    return Case("detection_target_gen_batch and mask_selection_gen_batch (the ROI stage's two chains)",
                lambda: (roi.detection_target_gen_batch(prop, cls, gt, group, pc, cfg, seed=7), roi.mask_selection_gen_batch(prop, pc, 16, cfg, seed=7)))


@case
def points_cropping():
    from gspn_amd.roi import points_cropping
    from tests.test_gpu_roi import crop_case
    pc, fea, cen, rois, idx = cuda(*crop_case(b=2, n=300, c=20, r=7, p=33, seed=1))
    w_fea, w_cen = rand(2, 7, 33, 20, seed=3), rand(2, 7, 33, 3, seed=4)

    def run():
        f, c = leaf(fea), leaf(cen)
        out = points_cropping(pc, f, c, rois, idx, 7, 33, True)
        ((out[0] * w_fea).sum() + (out[1] * w_cen).sum()).backward()
        return [o.detach() for o in out], f.grad, c.grad
    return Case("points_cropping (2, 300, 20) r=7 p=33 forward and gradients", run)


@case
def nearest_in_sets():
    from gspn_amd.detect import nearest_in_sets
    from tests.test_gpu_detect import nearest_case
    a = cuda(*nearest_case(2, 3, 63, 7, "replacement", 31 * 63 + 7))
    b = cuda(*nearest_case(2, 5, 257, 256, "lattice", 31 * 257 + 256))
    return Case("nearest_in_sets (2, 3, 63, 7) and (2, 5, 257, 256), gated and not",
                lambda: (nearest_in_sets(a[0], a[1], a[2]), nearest_in_sets(a[0], a[1], None), nearest_in_sets(b[0], b[1], b[2]), nearest_in_sets(b[0], b[1], None)))


@case
def unmold_and_select():
    from gspn_amd import detect
    from tests.test_gpu_detect import unmold_case
    a = cuda(*unmold_case(1, 3, 50, 5, 2, 55))
    b = cuda(*unmold_case(2, 9, 700, 33, 19, 733))

    def run():
        return [(detect.select_segmentation(m, ids), detect.unmold_segmentation(m, rois, ids, crop, pc)) for m, rois, ids, crop, pc in (a, b)]
    return Case("select_segmentation and unmold_segmentation (1, 3, 50, 5, 2) and (2, 9, 700, 33, 19)", run)


@case
def refine_detections():
    from gspn_amd.detect import refine_detections_batch
    from tests.test_gpu_detect import config, detection_inputs
    args = cuda(*detection_inputs(1, 7, 3, 11))
    cfg = config(4, 0.7, True)
    cfg0 = config(4, 0, False)
    return Case("refine_detections_batch (1, 7, 3): with the shrink and a confidence floor, and without either",
                lambda: (refine_detections_batch(*args, cfg), refine_detections_batch(*args, cfg0)))


# ---- spn_boxes.py --------------------------------------------------------------------------------------------------------------------
@case
def box_shrink():
    from gspn_amd.spn_boxes import box_shrink
    from tests.test_gpu_spn_boxes import shrink_case
    one = cuda(*shrink_case(1, 1, 1, 8))
    odd = cuda(*shrink_case(1, 7, 63, 112))
    more = cuda(*shrink_case(3, 65, 1000, 1455))
    return Case("box_shrink (1, 1, 1), (1, 7, 63), (3, 65, 1000)", lambda: (box_shrink(*one), box_shrink(*odd), box_shrink(*more)))


@case
def points_bbox():
    from gspn_amd.spn_boxes import points_bbox
    pts, off = rand(5, 1000, 3, seed=1), rand(5, 3, seed=2)
    lead, lead_off = rand(2, 7, 33, 3, seed=3), rand(2, 7, 3, seed=4)
    return Case("points_bbox (5, 1000), (1, 1), (2, 7, 33) with and without an offset",
                lambda: (points_bbox(pts, off), points_bbox(pts[:1, :1].contiguous(), None), points_bbox(lead, lead_off), points_bbox(pts, None)))


@case
def spn_target_gen():
    from gspn_amd.spn_boxes import spn_target_gen_batch
    from tests import spn_ref as SR
    args = list(SR.seeded_target_inputs(3, b=2))
    args[2][0] = 0.0                                                        # one scene of the batch has no valid box
    args = cuda(*args)
    full = cuda(*SR.seeded_target_inputs(4))
    return Case("spn_target_gen_batch: a batch with a scene without ground truth, and a full scene",
                lambda: (spn_target_gen_batch(*args), spn_target_gen_batch(*full)))


# ---- predict.py ----------------------------------------------------------------------------------------------------------------------
def _stage(b, r, n, p, c, seed, **kw):
    from tests import predict_ref as PR
    from tests.test_gpu_predict import class_ids_of, host_tables
    pc, ep = PR.stage_inputs(b, r, n, p, c, seed=seed, ladder=False, **kw)
    sem_prob, point_fb = host_tables(pc, ep)
    boxes = ep["detections"][:, :, :6].contiguous().cuda()
    crop = ep["pc_coord_cropped_final_unnormalized"].cuda()
    args = (ep["rpointnet_mask_selected"].cuda(), class_ids_of(ep).cuda(), torch.from_numpy(sem_prob).cuda(), torch.from_numpy(point_fb).cuda())
    return pc.cuda(), boxes, crop, args, ep["detections"][:, :, 7].contiguous().cuda()


@case
def scene_confidence():
    from gspn_amd.detect import nearest_in_sets
    from gspn_amd.predict import scene_confidence
    pc, boxes, crop, args, _ = _stage(2, 3, 257, 5, 19, 21, empty_row=True, full_row=True)
    one = _stage(1, 1, 1, 1, 2, 21, empty_row=True, full_row=True)
    return Case("scene_confidence (2, 3, 257, 5, 19) and (1, 1, 1, 1, 2) behind nearest_in_sets",
                lambda: (scene_confidence(nearest_in_sets(pc, crop, boxes), *args), scene_confidence(nearest_in_sets(one[0], one[2], one[1]), *one[3])))


def _scene_rank(r):
    from gspn_amd.detect import nearest_in_sets
    from gspn_amd.predict import scene_confidence, scene_rank
    pc, boxes, crop, args, det_score = _stage(2, r, 300, 8, 19, 30 + r, empty_row=r > 2)

    def run():
        sem_conf, fb_conf, _, _ = scene_confidence(nearest_in_sets(pc, crop, boxes), *args)
        return scene_rank(det_score, args[1], sem_conf, fb_conf)
    return Case("scene_rank r=%d on the device's own confidences" % r, run)


@case
def scene_rank_r1():
    return _scene_rank(1)


@case
def scene_rank_r65():
    return _scene_rank(65)


@case
def sem_iou_counts():
    from gspn_amd.predict import mean_iou, semantic_iou_counts
    rng = np.random.default_rng(19)
    batches = []
    for rows in (255, 256, 257):
        logits = np.round(1.5 * rng.standard_normal((rows, 19)), 1).astype(np.float32)
        logits[::5, 0] = logits[::5, 18] = 9.0                              # two equal maxima: the first wins
        labels = rng.integers(0, 19, rows).astype(np.int32)
        labels[::3] = 0
        batches.append((torch.from_numpy(logits).cuda(), torch.from_numpy(labels).cuda()))

    def run():
        out = []
        for logits, labels in batches:
            inter, union = semantic_iou_counts(logits, labels)
            inter, union = semantic_iou_counts(logits.flip(0).contiguous(), labels.flip(0).contiguous(), inter, union)      # added into the same accumulators
            out.append((inter, union, mean_iou(inter, union)))
        return out
    return Case("semantic_iou_counts rows 255, 256, 257 (two calls into one pair of accumulators) and mean_iou", run)


# ---- evaluate.py ---------------------------------------------------------------------------------------------------------------------
@case
def instance_overlaps():
    from gspn_amd.evaluate import instance_overlaps
    from tests.test_gpu_evaluate import dev, overlap_inputs
    sets = []
    for shape in ((3, 1, 257, 2, 1), (2, 5, 1003, 4, 7)):
        masks, cls, seg, group = overlap_inputs(*shape, seed=sum(shape))
        sets.append((dev(masks, torch.uint8), dev(cls, torch.int32), dev(seg, torch.int32), dev(group, torch.int32), shape[3], shape[4]))
    return Case("instance_overlaps (3, 1, 257, 2, 1) and (2, 5, 1003, 4, 7)", lambda: [instance_overlaps(*s) for s in sets])


def _instance_match(r):
    from gspn_amd.evaluate import instance_match, instance_overlaps
    from tests.test_gpu_evaluate import THRESHOLDS, batch_tensors, random_scene
    rng = np.random.default_rng(100 + r)
    masks, cls, conf, count, seg, group = batch_tensors([random_scene(rng, 600, r, 4, 9, 4, 40) for _ in range(4)])

    def run():
        inter, void, size, gt = instance_overlaps(masks, cls, seg, group, 4, 9)
        return inter, void, size, gt, instance_match(inter, void, size, cls, conf, count, gt, THRESHOLDS, 5)
    return Case("instance_overlaps + instance_match r=%d, four scenes of 600 points" % r, run)


@case
def instance_match_r63():
    return _instance_match(63)


@case
def instance_match_r65():
    return _instance_match(65)


# ---- data_prep.py --------------------------------------------------------------------------------------------------------------------
@case
def segment_labels():
    from gspn_amd import data_prep
    from tests import data_prep_ref as PR
    from tests.test_gpu_data_prep import random_case
    sets = []
    for n in (63, 257):
        seg, groups = random_case(n, 100 * n + 2, 0.3)
        segments, objects = PR.pairs_of(groups)
        sets.append((torch.from_numpy(seg.astype(np.int32)).cuda(), torch.tensor(segments, dtype=torch.int32).cuda(), torch.tensor(objects, dtype=torch.int64).cuda()))
    return Case("segment_labels n=63 and n=257, segments named twice", lambda: [data_prep.segment_labels(*s) for s in sets])


@case
def downsample_scans():
    from gspn_amd import data_prep
    from tests.test_gpu_data_prep import scan_of
    scans = [tuple(torch.from_numpy(a.copy()).cuda() for a in scan_of(n, 5 + n)) for n in (3000, 2500)]
    return Case("downsample_scans: two scans of 3000 and 2500 points to 2000",
                lambda: data_prep.downsample_scans(scans, nsample=2000, batch=2),
                note="prepare_scans and build_cache read and write files; their device work is this function and dataset.py's (geometry file)")


# ---- train.py / parallel.py ----------------------------------------------------------------------------------------------------------
@case
def batch_assemble_and_permutation():
    from gspn_amd.train import batch_perm
    from tests.test_gpu_train import make_cache
    cache, data = make_cache(4, 65, 2, 4, [2, 1, 2, 2], seed=65)
    wide, wide_data = make_cache(3, 1000, 12, 64, [12, 5, 1], seed=7)
    seed = dev_seed(21)

    def run():
        plain = data(is_augment=False, permute_points=True).batch([2, 0, 3], seed)
        aug = data(is_augment=True, permute_points=True).batch([2, 0, 3], seed)
        big = wide_data(is_augment=True, permute_points=False).batch([1, 2], 9)
        return batch_perm(seed, 3, 65), plain, aug, big
    return Case("batch_perm n=65 and DeviceDataset.batch (gspn_batch_assemble): permuted, augmented, 12 groups of 64 points", run)


@case
def scalars_accumulate():
    from gspn_amd.train import ScalarSums
    gen = torch.Generator().manual_seed(9)
    values = (torch.randn(5, 9, generator=gen) * 10.0 ** torch.randint(-6, 7, (5, 9), generator=gen).float()).float().cuda()

    def run():
        sums = ScalarSums(9, "cuda")
        for call in range(5):
            sums.add([values[call, i] for i in range(9)])
        return sums.sums, sums.count
    return Case("scalars_accumulate k=9, five calls", run)


def _optimiser(kind, n):
    from gspn_amd.parallel import FlatAdam, FlatGradBucket
    from gspn_amd.train import FlatAdamTF, FlatMomentum
    init = rand(n, seed=n)
    grads = [rand(n, seed=n + 1 + s) * 10.0 ** (s - 1) for s in range(3)]

    def run():
        p = torch.nn.Parameter(init.clone())
        bucket = FlatGradBucket([p])
        opt = {"adam": lambda: FlatAdam(bucket, lr=1e-2, weight_decay=1e-3), "adam_dev": lambda: FlatAdam(bucket, lr=1e-2, device_step=True),
               "adam_tf": lambda: FlatAdamTF(bucket, lr=1e-2), "momentum": lambda: FlatMomentum(bucket, lr=1e-2, momentum=0.9)}[kind]()
        for g in grads:
            p.grad = g.clone()
            bucket.flatten()
            opt.step(grad_scale=0.5)
        state = [getattr(opt, k) for k in ("m", "v", "accum", "_dev_state") if getattr(opt, k, None) is not None]
        assert opt.t == 3 and p.data_ptr() == opt.flat.data_ptr()
        return opt.flat, bucket.flat, state
    return Case("%s over n=%d parameters, three steps" % (kind, n), run)


for _kind in ("adam", "adam_dev"):
    for _n in (1, 255, 257, 1025):
        def _build(kind=_kind, n=_n):
            return _optimiser(kind, n)
        _build.__name__ = "flat_%s_n%d" % (_kind, _n)
        case(_build)
for _kind in ("adam_tf", "momentum"):
    def _build(kind=_kind):
        return _optimiser(kind, 257)
    _build.__name__ = "flat_%s_n257" % _kind
    case(_build)


@case
def dot():
    from gspn_amd import _lib as L
    n = 4099                                                               # no multiple of 4
    a = rand(n + 1, seed=1)[1:]                                             # 4-byte aligned only
    b = rand(n, seed=2)
    assert a.data_ptr() % 16 == 4

    def run():
        w = torch.empty(int(L.lib().gspn_dot_work_floats()), device="cuda")
        out = []
        for x in (a, b):
            o = torch.empty((), device="cuda")
            L.check(L.lib().gspn_dot(n, L.ptr(x), L.ptr(b), L.ptr(w), L.ptr(o), L.stream()), "dot")
            out.append(o)
        return out
    return Case("gspn_dot n=4099, exact gspn_dot_work_floats work buffer, one operand 4-byte aligned only", run,
                note="the bench's loss kernel has no wrapper: called as bench.py and tests/test_gpu_modules.py call it")


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
MASKED = set()          # names of the rows that carry a mask or a canonical form: none here


@pytest.mark.parametrize("build", CASES, ids=lambda f: f.__name__)
def test_arena(build):
    c = build()
    assert c.masked == (build.__name__ in MASKED)
    sweep(c)


def test_zz_masked_cases():
    print("\ntests/test_gpu_arena_stages.py: %d cases, %d masked" % (len(CASES), len(MASKED)))
    assert not MASKED
