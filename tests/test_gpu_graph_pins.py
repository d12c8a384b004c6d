"""The device stages that replace the TensorFlow graph code of models/model_rpointnet.py, against what the REFERENCE's own lines gave on
recorded inputs: the fixtures of tools/make_golden_graph.py under tests/golden/graph/ (read here, never rebuilt).  The rules of equality,
the derived bounds and the checks of the two randomised stages are those of tests/test_cpu_graph_pins.py, which holds the restatements to
the same files; the two randomised stages run under three seeds."""
import numpy as np
import pytest
import torch

from tests.test_cpu_graph_pins import (DetectConfig, check_box_delta, check_detection_targets, check_get_loss, check_losses, check_mask_selection,
                                       check_points_cropping, check_refine_detections, fixture, get_loss_inputs, same_values, target_args, target_scenes)

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2)


def dev(a, dtype=None):
    x = torch.from_numpy(np.array(a))
    return (x if dtype is None else x.to(dtype)).cuda()


def host(x):
    return x.detach().cpu().numpy()


def test_box_shrink_equals_the_reference():
    from gspn_amd import spn_boxes
    fx = fixture("box_shrink")
    assert same_values(host(spn_boxes.box_shrink(dev(fx["box"]), dev(fx["pc"]))), fx["out"])


def test_spn_target_gen_equals_the_reference():
    from gspn_amd import rpointnet, spn_boxes
    fx = fixture("spn_target_gen")
    args = [dev(fx[k]) for k in ("proposals", "seed_class_ids", "gt_class_ids", "gt_boxes")]
    got = spn_boxes.spn_target_gen_batch(*args)
    assert got.dtype == torch.int32 and same_values(host(got), fx["spn_match"])
    for i in range(len(fx["proposals"])):
        one = rpointnet.spn_target_gen(*[a[i] for a in args])
        assert one.dtype == torch.float32 and same_values(host(one), fx["spn_match"][i].astype(np.float32))


def test_gather_selection_equals_the_reference():
    from gspn_amd.rpointnet import gather_selection
    fx = fixture("gather_selection")
    assert same_values(host(gather_selection(dev(fx["source"]), dev(fx["selected_idx"]), fx["selected_idx"].shape[1])), fx["out"])


def test_box_refinement_and_apply_box_delta_within_the_derived_bound():
    from gspn_amd import roi
    fx = fixture("box_delta")
    box = dev(fx["box"])
    check_box_delta(host(roi.box_refinement(box, dev(fx["gt_box"]))), host(roi.apply_box_delta(box, dev(fx["delta"]))), "roi (device)")


class TargetConfig(object):
    BBOX_STD_DEV = (0.1, 0.1, 0.1, 0.2, 0.2, 0.2)

    def __init__(self):
        self.TRAIN_ROIS_PER_IMAGE, self.ROI_POSITIVE_RATIO, self.NUM_POINT_INS_MASK = target_args()


@pytest.mark.parametrize("seed", SEEDS)
def test_detection_targets_against_the_tables(seed):
    from gspn_amd import roi
    cfg = TargetConfig()
    prop, cls, boxes, label, pc = [dev(a) for a in target_scenes()]
    roi_src, roi_gt = roi.detection_target_select(prop, roi.box_point_count(prop, pc), cls, boxes, cfg.TRAIN_ROIS_PER_IMAGE, cfg.ROI_POSITIVE_RATIO, seed)
    rois, ids, bbox, idx, mask = roi.detection_target_gen_batch(prop, cls, boxes, label, pc, cfg, seed)
    assert same_values(host(rois), host(roi._take_rows(prop, roi_src))), "both entries make the same draw"
    check_detection_targets(host(roi_src), host(roi_gt), host(rois), host(ids), host(bbox), host(idx), host(mask), "roi (device) seed %d" % seed)
    for i in range(len(prop)):                                                           # the reference's per-scene signature, with its (N, G) mask matrix
        gt_masks = (label[i].unsqueeze(1) == torch.arange(cls.shape[1], device=label.device)).float()
        one = roi.detection_target_gen(prop[i], cls[i], boxes[i], gt_masks, pc[i], cfg, seed)
        for a, b in zip(one, (rois[i], ids[i], bbox[i], idx[i], mask[i])):
            assert same_values(host(a), host(b))


@pytest.mark.parametrize("seed", SEEDS)
def test_mask_selection_gen_equals_the_reference(seed):
    from gspn_amd import roi
    fx = fixture("mask_selection")
    cfg = TargetConfig()
    num_rois = int(fx["args"][0])
    cfg.NUM_POINT_INS_MASK = int(fx["args"][1])
    prop, pc = dev(np.stack([fx["s%d/proposals" % i] for i in range(2)])), dev(np.stack([fx["s%d/pc" % i] for i in range(2)]))
    for removal in (True, False):
        rois, idx = roi.mask_selection_gen_batch(prop, pc, num_rois, cfg, removal, seed)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (2, num_rois, cfg.NUM_POINT_INS_MASK)
        for i in range(2):
            check_mask_selection(host(rois[i]), host(idx[i]), i, removal, "roi (device) seed %d removal %s" % (seed, removal))


def test_points_cropping_equals_the_reference():
    from gspn_amd import roi
    fx = fixture("points_cropping")
    args = [dev(fx[k]) for k in ("pc", "pc_fea", "pc_center", "rois", "idx")]
    r, p = fx["idx"].shape[1:]
    check_points_cropping(lambda normalize: [host(a) for a in roi.points_cropping(*args, r, p, normalize)], "roi (device)")


@pytest.mark.parametrize("shrink", [False, True])
def test_refine_detections_equals_the_reference(shrink):
    from gspn_amd import detect
    fx = fixture("refine_detections")
    cfg = DetectConfig(shrink)
    args = [dev(fx[k]) for k in ("rois", "probs", "deltas", "pc")]
    ids, scores, refined = detect.classified_boxes(*args, cfg)
    assert same_values(host(ids), fx["probs"].argmax(-1).astype(np.int32)) and same_values(host(scores), fx["probs"].max(-1))      # numpy's argmax: the first maximum
    det = detect.refine_detections_batch(*args, dev(fx["fb_prob"]), dev(fx["sem_prob"]), cfg)
    check_refine_detections(host(refined), host(det), shrink, "detect (device) SHRINK_BOX %s" % shrink)
    one = detect.refine_detections(*[a[0] for a in args], dev(fx["fb_prob"])[0], dev(fx["sem_prob"])[0], cfg)
    assert same_values(host(one), host(det[0]))
    if not shrink:
        nobody = detect.refine_detections_batch(args[0], dev(fx["probs_no_candidate"]), args[2], args[3], dev(fx["fb_prob"]), dev(fx["sem_prob"]), cfg)
        want = fx["detections_no_candidate"]
        assert same_values(host(nobody)[..., 6:], want[..., 6:]) and not host(nobody)[1].any()


def test_segmentation_equals_the_reference():
    from gspn_amd import detect
    fx = fixture("segmentation")
    masks, rois, class_ids, crops, pc = [dev(fx[k]) for k in ("masks", "rois", "class_ids", "crops", "pc")]
    assert same_values(host(detect.select_segmentation(masks, class_ids)), fx["selected"])
    assert same_values(host(detect.select_segmentation(masks, class_ids.float())), fx["selected"])          # the reference casts the ids
    assert same_values(host(detect.unmold_segmentation(masks, rois, class_ids, crops, pc)), fx["unmolded"])
    idx = host(detect.nearest_in_sets(pc, crops, rois))
    lo, hi = fx["rois"][:, :, None, :3] - fx["rois"][:, :, None, 3:] / 2, fx["rois"][:, :, None, :3] + fx["rois"][:, :, None, 3:] / 2
    inside = ((fx["pc"][:, None] >= lo) & (fx["pc"][:, None] <= hi)).all(-1)             # exact on the raster
    assert np.array_equal(idx >= 0, inside)
    # the FIRST of the nearest crop points (duplicates, and distinct points at one distance): the exact distances of the raster decide
    d2 = ((fx["pc"][:, None, :, None, :].astype(np.float64) - fx["crops"][:, :, None, :, :]) ** 2).sum(-1)
    assert np.array_equal(idx[inside], d2.argmin(-1)[inside])


def test_losses_within_the_derived_bounds():
    from gspn_amd import heads, rpointnet
    check_losses(lambda a, b: host(rpointnet.smooth_l1_loss(a, b)), rpointnet.get_spn_class_loss, heads.get_rpointnet_class_loss, heads.get_rpointnet_bbox_loss,
                 heads.get_rpointnet_mask_loss, "product (device)", convert=dev)


def test_get_loss_within_the_derived_bounds():
    from gspn_amd import rpointnet
    end_points, smpw, alpha = get_loss_inputs(dev)

    class Cfg(rpointnet.Config):
        BATCH_SIZE = int(smpw.shape[0])
        NUM_POINT_INS = int(end_points["pc_ins_centered_seed"].shape[2])
        TRAIN_MODULE = ['SPN']

    loss, end_points = rpointnet.get_loss(end_points, Cfg(), alpha, smpw)
    assert float(loss) == float(end_points["loss"])
    check_get_loss({k: host(v) for k, v in end_points.items()}, "rpointnet.get_loss (device)")
