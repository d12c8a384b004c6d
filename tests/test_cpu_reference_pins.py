"""The restatements of the stages the reference runs in plain numpy -- tests/dataset_ref.py, tests/data_prep_ref.py, tests/predict_ref.py --
and the product code that runs on CPU tensors, against what the REFERENCE's own lines gave on recorded inputs: the fixtures
tools/make_golden_stages.py writes under tests/golden/{dataset,data_prep,predict}/ by cutting the line ranges out of a checkout of the
reference and exec'ing them.  Nothing is rebuilt here: inputs and outputs are read from the fixtures.

What "equal" means per stage:
  remap          integer-exact on seg_label, group_label, ngroup, with max_groups = max(group) + 1
  getitem        is_augment False: bit-exact.  True: points within one float32 step of the reference's float64 result cast to float32
                 (tests.test_gpu_dataset.within_one_ulp); boxes within BOX_STEPS float32 steps at max(|hi|, |lo|), derived at box_gap
  collect_label  labels exact, conflicts equal to the counted lines
  export         masks, label ids, confidences and the row order exact; sem_conf and fb_conf within predict_ref.within_bound
  iou            counts exact, iou and meaniou equal as float64"""
import os

import numpy as np
import pytest
import torch

from tests import data_prep_ref as PP
from tests import dataset_ref as DR
from tests import predict_ref as PR
from tests.test_gpu_dataset import within_one_ulp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FIXTURES = {
    "remap": "dataset/remap_ref.npz",
    "getitem": "dataset/getitem_ref.npz",
    "collect_label": "data_prep/collect_label_ref.npz",
    "export": "predict/export_ref.npz",
    "iou": "predict/iou_ref.npz",
}

# the cases every fixture must hold, by the names the generator stores
REQUIRED = {
    "remap": ("mean_exactly_0.5", "mean_exactly_1.5", "mean_exactly_2.5", "mean_just_below_0.5", "mean_just_above_0.5", "id_gap", "group_minus_1",
              "seg_negative", "seg_40_or_more", "seg_in_range_not_a_class", "all_background", "one_valid_group", "id_max_groups_minus_1_valid"),
    "getitem": ("plain", "plain_curngroup_equals_ngroup", "plain_curngroup_1", "augmented", "augmented_padded_rows_equal_t"),
    "collect_label": ("segment_in_two_groups", "segment_twice_in_one_group", "named_segment_without_vertex", "vertex_in_no_group", "object_id_0",
                      "no_pairs"),
    "export": ("class_0_rows", "box_without_point_in_second_partition", "both_partitions", "empty_first_partition", "no_detection",
               "point_on_box_face_in_mask", "mask_value_float32_0.4_set", "mask_value_below_0.4_clear"),
    "iou": ("exact_logit_ties", "class_absent_from_both", "labels_0"),
}

_loaded = {}


def fixture(stage):
    """the arrays of one fixture, read once and never written"""
    if stage not in _loaded:
        with np.load(os.path.join(GOLDEN, FIXTURES[stage]), allow_pickle=False) as f:
            _loaded[stage] = {k: f[k] for k in f.files}
        for a in _loaded[stage].values():
            a.setflags(write=False)
    return _loaded[stage]


@pytest.mark.parametrize("stage", sorted(FIXTURES))
def test_every_fixture_holds_its_cases(stage):
    fx = fixture(stage)
    count = dict(zip(fx["cases"].tolist(), fx["case_counts"].tolist()))
    for name in REQUIRED[stage]:
        assert count.get(name, 0) > 0, "%s: case %s is not in the fixture" % (stage, name)
    assert os.path.getsize(os.path.join(GOLDEN, FIXTURES[stage])) <= os.path.getsize(os.path.join(GOLDEN, "interp_ref_demo.npz"))
    points = [a.shape[0] for k, a in fx.items() if k.split("/")[-1] in ("pc", "group", "seg_indices", "labels")]
    assert stage == "iou" or (points and max(points) <= 4096)


# ---- remap -------------------------------------------------------------------------------------------------------------------------------

def test_remap_restatement_and_cpu_product_equal_the_reference():
    from gspn_amd import dataset
    fx = fixture("remap")
    for name in fx["scans"].tolist():
        group, seg = fx[name + "/group"], fx[name + "/seg"]
        want = fx[name + "/group_label"], fx[name + "/seg_label"], int(fx[name + "/ngroup"])
        assert want[0].dtype == np.int32 and want[1].dtype == np.int64
        got = DR.remap_labels(group, seg)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], name
        for dtype in (torch.int32, torch.int64):
            for bound in (int(group.max()) + 1, int(group.max()) + 7):                    # the reference's bound, and a static one above it
                out = dataset.remap_labels(torch.from_numpy(group.copy())[None].to(dtype), torch.from_numpy(seg.copy())[None].to(dtype), bound)
                assert np.array_equal(out[0][0].numpy(), want[0]) and np.array_equal(out[1][0].numpy(), want[1]), name
                assert out[2].tolist() == [want[2]]


# ---- getitem -----------------------------------------------------------------------------------------------------------------------------

BOX_STEPS = 2


def box_gap(got_box, want_box, pc_ins):
    """The largest gap between two (G, 6) boxes per axis, in float32 steps at max(|hi|, |lo|) of pc_ins (G, M, 3) float32 -> (centre,
    size).  The bound BOX_STEPS = 2, absolute, for both: with u the float32 step at max(|hi|, |lo|), the product's extremes are the
    reference's float64 ones rounded (rounding is monotone, so max and min commute with it), each within u / 2.  hi32 - lo32 and hi64 - lo64
    are therefore two reals within u of each other, and so are the two sums; each is rounded ONCE to float32 (the kernel's mx - mn and
    (mx + mn) / 2.0f, halving is exact; the reference's assignment to its float32 array).  Neither |hi - lo| nor |hi + lo| exceeds twice
    the maximum, where float32 steps are 2 u: two reals within half that step round to the same or to neighbouring values, 2 u apart at
    most; below that binade the steps are u or less and the results are within u + u.  The halved sum: within u."""
    hi, lo = pc_ins.max(1), pc_ins.min(1)
    step = np.spacing(np.maximum(np.abs(hi), np.abs(lo)).astype(np.float32)).astype(np.float64)
    gap = np.abs(got_box.astype(np.float64) - want_box.astype(np.float64))
    return float((gap[:, :3] / step).max()), float((gap[:, 3:] / step).max())


def padded(fx, name):
    pc_ins, g = fx[name + "/pc_ins"], fx[name + "/group_indicator"].shape[0]
    full = np.zeros((g,) + pc_ins.shape[1:], np.float32)
    full[:pc_ins.shape[0]] = pc_ins
    return full


def test_getitem_restatements_equal_the_reference():
    from gspn_amd import dataset
    fx = fixture("getitem")
    for name in fx["runs"].tolist():
        cur, full = int(fx[name + "/curngroup"]), padded(fx, name)
        g = full.shape[0]
        assert np.array_equal(DR.group_indicator(np.array([cur]), g)[0], fx[name + "/group_indicator"])
        want_pc, want_ins, want_box = fx[name + "/pc_out"], fx[name + "/pc_ins_full"], fx[name + "/bbox_ins_full"]
        if name + "/R" not in fx:
            assert np.array_equal(full.view(np.int32), want_ins.view(np.int32)) and np.array_equal(fx[name + "/pc"], want_pc)
            assert np.array_equal(DR.boxes(full).view(np.int32), want_box.view(np.int32))
            continue
        rot, trans = fx[name + "/R"], fx[name + "/t"]
        assert rot.dtype == trans.dtype == np.float64
        got_pc, got_ins = DR.rigid(fx[name + "/pc"], rot, trans), DR.rigid(full, rot, trans)
        ours_pc = dataset._rigid(torch.from_numpy(fx[name + "/pc"].copy())[None], torch.from_numpy(rot.copy())[None], torch.from_numpy(trans.copy())[None])[0].numpy()
        ours_ins = dataset._rigid(torch.from_numpy(full)[None], torch.from_numpy(rot.copy())[None], torch.from_numpy(trans.copy())[None])[0].numpy()
        print("%s: unequal float32 values, restatement %d + %d, dataset._rigid on the CPU %d + %d of %d + %d" % (
            name, within_one_ulp(got_pc, want_pc), within_one_ulp(got_ins, want_ins), within_one_ulp(ours_pc, want_pc),
            within_one_ulp(ours_ins, want_ins), want_pc.size, want_ins.size))
        rows = np.ones(g, bool)
        rows[1:cur] = False                                                               # the background's row and the padding: 0 @ R + t
        for ins in (got_ins, ours_ins, want_ins):
            assert np.array_equal(ins[rows], np.broadcast_to(trans.astype(np.float32), ins[rows].shape))
        for ins in (got_ins, ours_ins):
            centre, size = box_gap(DR.boxes(ins), want_box, ins)
            print("%s: boxes of float32 points against the reference's of float64 points, %.3g (centre) and %.3g (size) float32 steps" % (name, centre, size))
            assert centre <= BOX_STEPS and size <= BOX_STEPS


# ---- collect_label -----------------------------------------------------------------------------------------------------------------------

def seg_groups_of(fx, name):
    """segGroups as the generator built them: the stored pairs split at the stored group sizes"""
    seg, obj, groups, at = fx[name + "/pair_segment"].tolist(), fx[name + "/pair_object"].tolist(), [], 0
    for size in fx[name + "/group_sizes"].tolist():
        groups.append({"segments": seg[at:at + size], "objectId": obj[at] if size else 0})
        at += size
    assert at == len(seg)
    return groups


def test_collect_label_restatement_equals_the_reference():
    fx = fixture("collect_label")
    for name in fx["scans"].tolist():
        groups = seg_groups_of(fx, name)
        label, lines = PP.collect_label_loop(fx[name + "/seg_indices"], groups)
        assert fx[name + "/label"].dtype == np.int32
        assert np.array_equal(label, fx[name + "/label"]) and lines == int(fx[name + "/conflicts"]), name
        seg, obj = PP.pairs_of(groups)
        assert seg == fx[name + "/pair_segment"].tolist() and obj == fx[name + "/pair_object"].tolist()


# ---- export ------------------------------------------------------------------------------------------------------------------------------

EXPORT_KEYS = ("rpointnet_mask_selected", "pc_coord_cropped_final_unnormalized", "detections", "sem_class_logits", "pc_seed", "fb_prob")


def export_scene(fx, name):
    """-> pc (N, 3), the six arrays of one scene, and the reference's outputs with the masks unpacked to (ND, N)"""
    n = fx[name + "/pc"].shape[0]
    want = {k: fx[name + "/" + k] for k in ("rows", "seg_label_pred", "confidence_pred", "sem_conf", "fb_conf")}
    want["group_label_pred"] = np.unpackbits(fx[name + "/group_label_pred"], axis=1, count=n).astype(np.int32).reshape(len(want["rows"]), n)
    return fx[name + "/pc"].copy(), [fx[name + "/" + k].copy() for k in EXPORT_KEYS], want


def test_export_restatement_equals_the_reference():
    fx = fixture("export")
    assert len(fx["scenes"]) >= 3
    for name in fx["scenes"].tolist():
        pc, arrays, want = export_scene(fx, name)
        masks, crops, det, logits, seeds, fb_prob = arrays
        n = pc.shape[0]
        lit = PR.output_prediction(pc, masks, crops, det, logits, seeds, fb_prob)
        nd = len(want["rows"])
        assert np.array_equal(lit["rows"], want["rows"]), name
        assert lit["group_label_pred"].dtype == np.int32 and lit["group_label_pred"].shape == (nd, n)
        assert np.array_equal(lit["group_label_pred"], want["group_label_pred"]), name
        assert np.array_equal(lit["seg_label_pred"], want["seg_label_pred"]) and np.array_equal(lit["confidence_pred"], want["confidence_pred"])
        assert PR.within_bound(lit["sem_conf"], want["sem_conf"], n) and PR.within_bound(lit["fb_conf"], want["fb_conf"], n)
        # the exact sums over the restatement's nearest crop points and numpy's float32 tables, and the ordering restatement on them
        idx = PR.DR.nearest_in_sets(torch.from_numpy(pc.copy())[None], torch.from_numpy(crops.copy())[None], torch.from_numpy(det[:, :6].copy())[None]).numpy()
        sem_prob, fb = PR.point_tables(pc, logits, seeds, fb_prob)
        cls = det[None, :, 6].astype(np.int32)
        sc, fc, mask, _ = PR.confidence_fsum(idx, masks[None], cls, sem_prob[None], fb[None])
        order, count, label_ids, confidence, _ = PR.rank(det[None, :, 7], cls, sc, fc)
        assert count[0] == nd and np.array_equal(order[0, :nd], want["rows"]) and np.array_equal(order[0, nd:], np.where(cls[0] <= 0)[0])
        assert np.array_equal(label_ids[0, :nd], want["seg_label_pred"]) and np.array_equal(confidence[0, :nd], want["confidence_pred"].astype(np.float32))
        assert np.array_equal(mask[0][order[0, :nd]], want["group_label_pred"])
        assert PR.within_bound(sc[0][order[0, :nd]], want["sem_conf"], n) and PR.within_bound(fc[0][order[0, :nd]], want["fb_conf"], n)


# ---- iou ---------------------------------------------------------------------------------------------------------------------------------

def test_iou_restatement_and_cpu_mean_equal_the_reference():
    from gspn_amd import predict
    fx = fixture("iou")
    inter = union = None
    for batch in range(int(fx["batches"])):
        logits, labels = fx["batch%d/logits" % batch], fx["batch%d/labels" % batch]
        inter, union = PR.iou_counts(logits, labels, logits.shape[-1], inter, union)
        assert np.array_equal(inter, fx["batch%d/cum_intersection" % batch]) and np.array_equal(union, fx["batch%d/cum_union" % batch])
    assert fx["iou"].dtype == np.float64 and fx["meaniou"].dtype == np.float64
    assert PR.mean_iou(inter, union) == fx["meaniou"]
    assert np.array_equal(np.divide(inter, union + 1e-8), fx["iou"]) and not fx["iou"][union == 0].any()
    assert float(predict.mean_iou(torch.from_numpy(inter), torch.from_numpy(union))) == float(fx["meaniou"])
