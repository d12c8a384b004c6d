"""The device stages that replace the reference's plain-numpy code, against what the REFERENCE's own lines gave on recorded inputs: the
fixtures of tools/make_golden_stages.py under tests/golden/ (read here, never rebuilt; the rules of equality are those of
tests/test_cpu_reference_pins.py, which checks the restatements against the same files)."""
import numpy as np
import pytest
import torch

from tests import predict_ref as PR
from tests.test_cpu_reference_pins import BOX_STEPS, box_gap, export_scene, fixture, padded
from tests.test_gpu_dataset import within_one_ulp

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def test_remap_labels_on_the_device_equals_the_reference():
    from gspn_amd import dataset
    fx = fixture("remap")
    for name in fx["scans"].tolist():
        group, seg = fx[name + "/group"], fx[name + "/seg"]
        for dtype in (torch.int32, torch.int64):
            out = dataset.remap_labels(dev(group, dtype)[None], dev(seg, dtype)[None], int(group.max()) + 1)
            assert out[0].is_cuda and out[0].dtype == out[1].dtype == torch.int64 and out[2].dtype == torch.int32
            assert np.array_equal(out[0][0].cpu().numpy(), fx[name + "/group_label"]), name
            assert np.array_equal(out[1][0].cpu().numpy(), fx[name + "/seg_label"]), name
            assert out[2].tolist() == [int(fx[name + "/ngroup"])]


def test_augment_and_box_equals_the_reference():
    from gspn_amd import dataset
    fx = fixture("getitem")
    worst = [0.0, 0.0]
    for name in fx["runs"].tolist():
        cur, full = int(fx[name + "/curngroup"]), padded(fx, name)
        g = full.shape[0]
        plain = name + "/R" not in fx
        rot = np.eye(3) if plain else fx[name + "/R"]                                      # no augmentation: x @ I + 0 in float64 is x
        trans = np.zeros(3) if plain else fx[name + "/t"]
        for valid in (cur, dev(np.array([cur]))):
            pc, ins, ind, box = dataset.augment_and_box(dev(fx[name + "/pc"])[None], dev(full)[None], valid, rotation=dev(rot)[None], translation=dev(trans)[None])
            pc, ins, ind, box = pc[0].cpu().numpy(), ins[0].cpu().numpy(), ind[0].cpu().numpy(), box[0].cpu().numpy()
            assert ind.dtype == np.int32 and np.array_equal(ind, fx[name + "/group_indicator"]), name
            want_pc, want_ins, want_box = fx[name + "/pc_out"], fx[name + "/pc_ins_full"], fx[name + "/bbox_ins_full"]
            if plain:
                assert np.array_equal(pc.view(np.int32), want_pc.view(np.int32)) and np.array_equal(ins.view(np.int32), want_ins.view(np.int32))
                assert np.array_equal(box.view(np.int32), want_box.view(np.int32)), name
                continue
            print("%s: %d of %d pc and %d of %d pc_ins values one float32 step from the reference's" % (
                name, within_one_ulp(pc, want_pc), pc.size, within_one_ulp(ins, want_ins), ins.size))
            rows = np.ones(g, bool)
            rows[1:cur] = False
            assert np.array_equal(ins[rows], np.broadcast_to(trans.astype(np.float32), ins[rows].shape))      # 0 @ R + t
            centre, size = box_gap(box, want_box, ins)
            worst = [max(worst[0], centre), max(worst[1], size)]
            assert centre <= BOX_STEPS and size <= BOX_STEPS, name
    print("bbox_ins against the reference's float64 boxes: worst gap %.3g (centre) and %.3g (size) float32 steps at max(|hi|, |lo|)" % tuple(worst))


def test_segment_labels_equals_the_reference():
    from gspn_amd import data_prep
    fx = fixture("collect_label")
    for name in fx["scans"].tolist():
        seg = fx[name + "/seg_indices"]
        for known in (None, int(seg.max()) + 1):
            label, conflicts = data_prep.segment_labels(dev(seg), dev(fx[name + "/pair_segment"]), dev(fx[name + "/pair_object"]), known)
            assert label.dtype == torch.int32 and conflicts.dtype == torch.int32
            assert np.array_equal(label.cpu().numpy(), fx[name + "/label"]), name
            assert conflicts.tolist() == [int(fx[name + "/conflicts"])], name


def test_scene_predictions_equals_the_reference():
    from gspn_amd.inference import _point_probabilities
    from gspn_amd.predict import scene_predictions
    fx = fixture("export")
    for name in fx["scenes"].tolist():
        pc, arrays, want = export_scene(fx, name)
        masks, crops, det, logits, seeds, fb_prob = arrays
        n, r, nd = pc.shape[0], det.shape[0], len(want["rows"])
        ep = dict(zip(("rpointnet_mask_selected", "pc_coord_cropped_final_unnormalized", "detections", "sem_class_logits", "pc_seed", "fb_prob"),
                      (dev(a)[None] for a in arrays)))
        pred = {k: v[0].cpu().numpy() for k, v in scene_predictions(ep, dev(pc)[None]).items()}
        cls = det[:, 6].astype(np.int32)
        assert pred["count"] == nd, name
        assert np.array_equal(pred["order"][:nd], want["rows"]) and np.array_equal(pred["order"][nd:], np.where(cls <= 0)[0]), name
        assert pred["masks"].dtype == np.uint8 and np.array_equal(pred["masks"][:nd], want["group_label_pred"]) and not pred["masks"][nd:].any(), name
        assert np.array_equal(pred["mask_points"][:nd], want["group_label_pred"].sum(1))
        assert np.array_equal(pred["label_ids"][:nd], want["seg_label_pred"]) and not pred["label_ids"][nd:].any()
        # confidence is float32 on the device: the reference's 1.0 / 0.97 rounded, and the text test.py:111 writes of it is the same
        assert np.array_equal(pred["confidence"][:nd], want["confidence_pred"].astype(np.float32)) and not pred["confidence"][nd:].any()
        assert ["%f" % v for v in pred["confidence"][:nd]] == ["%f" % v for v in want["confidence_pred"]]
        # the two confidences: within_bound of the exact sums over the device's own float32 tables, as
        # test_scene_predictions_against_the_literal_restatement grants it; the nearest seed is the reference's (equal point_fb) ...
        table = _point_probabilities(dev(pc)[None], ep)[0].cpu().numpy()
        host_sem, host_fb = PR.point_tables(pc, logits, seeds, fb_prob)
        assert np.array_equal(table[:, 0], host_fb)
        idx = PR.DR.nearest_in_sets(torch.from_numpy(pc)[None], torch.from_numpy(crops)[None], torch.from_numpy(det[:, :6].copy())[None]).numpy()
        exact = PR.confidence_fsum(idx, masks[None], cls[None], np.ascontiguousarray(table[None, :, 1:]), np.ascontiguousarray(table[None, :, 0]))
        at = pred["order"]
        assert PR.within_bound(pred["sem_conf"], exact[0][0][at], n) and PR.within_bound(pred["fb_conf"], exact[1][0][at], n), name
        # ... and against the reference's own values: fb_conf reads the same table, so the same bound; sem_conf is a weighted mean of
        # softmax values, so it moves by no more than the largest difference between the device's float32 softmax and numpy's
        assert PR.within_bound(pred["fb_conf"][:nd], want["fb_conf"], n), name
        moved = float(np.abs(table[:, 1:].astype(np.float64) - host_sem.astype(np.float64)).max())
        gap = np.abs(pred["sem_conf"][:nd] - want["sem_conf"])
        print("%s: %d predictions; softmax, device against numpy: %.3g; sem_conf against the reference: %.3g" % (name, nd, moved, gap.max(initial=0)))
        assert np.all(gap <= moved + 4.0 * n * 2.0 ** -53 * want["sem_conf"]), name
        assert not pred["sem_conf"][nd:].any() and not pred["fb_conf"][nd:].any() and r == len(at)


def test_semantic_iou_equals_the_reference():
    from gspn_amd.predict import mean_iou, semantic_iou_counts
    fx = fixture("iou")
    inter = union = None
    for batch in range(int(fx["batches"])):
        inter, union = semantic_iou_counts(dev(fx["batch%d/logits" % batch]), dev(fx["batch%d/labels" % batch]), inter, union)
        assert inter.dtype == union.dtype == torch.int64
        assert np.array_equal(inter.cpu().numpy(), fx["batch%d/cum_intersection" % batch])
        assert np.array_equal(union.cpu().numpy(), fx["batch%d/cum_union" % batch])
    got = mean_iou(inter, union)
    assert got.dtype == torch.float64
    print("mean IoU %.17g, the reference's %.17g" % (float(got), float(fx["meaniou"])))
    assert float(got) == float(fx["meaniou"])
