"""CPU tests of gspn_amd/predict.py: ABI 19 and its three symbols, the invariants of the restatements in tests/predict_ref.py (the literal
test.py:155-205 against the exact sums and against the ordering from given confidences), write_predictions and write_ground_truth against
literal text and against the restated exporters, the shape and dtype rules, and mean_iou."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import detect_ref as DR
from tests import predict_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_19_and_the_predict_symbols():
    from gspn_amd import _lib, build
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    assert int(re.search(r"#define GSPN_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gspn_abi_version() >= 19
    assert re.search(r"^ \*\s+19: gspn_scene_confidence / gspn_scene_rank / gspn_sem_iou_counts", text, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("gspn_scene_confidence", 16), ("gspn_scene_rank", 16), ("gspn_sem_iou_counts", 7)):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        declared = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(declared.split(",")) == len(_lib.SIGNATURES[name]) == nargs
        # the thresholds cross the ABI as doubles
        assert [i for i, a in enumerate(declared.split(",")) if a.strip().startswith("double ")] == \
            [i for i, a in enumerate(_lib.SIGNATURES[name]) if a is ctypes.c_double]
    assert _lib.SIGNATURES["gspn_scene_confidence"].count(ctypes.c_double) == 1 and _lib.SIGNATURES["gspn_scene_rank"].count(ctypes.c_double) == 2
    from gspn_amd.build import POLICY_SOURCES
    assert "predict.hip" not in POLICY_SOURCES
    # host-side argument rules (no launch): a null pointer, and more rows than the rank kernel takes
    null = ctypes.c_void_p(0)
    assert lib.gspn_scene_rank(1, 4, 19, null, null, null, null, 0.01, 0.01, null, null, null, null, null, null, null) == -1
    assert lib.gspn_sem_iou_counts(0, 19, null, null, null, null, null) == -1


def test_package_exports_the_stage():
    from gspn_amd import predict, rpointnet
    for name in ("SCANNET_LABEL_MAP", "scene_confidence", "scene_rank", "scene_predictions", "semantic_iou_counts", "mean_iou",
                 "write_predictions", "write_ground_truth"):
        assert name in rpointnet.__all__ and name in predict.__all__ and getattr(rpointnet, name) is getattr(predict, name)
    assert tuple(predict.SCANNET_LABEL_MAP) == tuple(PR.SEG_LABEL_MAP.tolist()) and len(predict.SCANNET_LABEL_MAP) == 19


# ---- the restatements against each other ---------------------------------------------------------------------------------------------------

SHAPE = (2, 9, 700, 16, 19)          # b, r, n, p, c


@pytest.fixture(scope="module")
def stage():
    pc, ep = PR.stage_inputs(*SHAPE, seed=5)
    return pc.numpy(), {k: v.numpy() for k, v in ep.items()}


def test_generator_has_the_rows_it_promises(stage):
    pc, ep = stage
    det = ep["detections"]
    cls = det[:, :, 6]
    assert (cls == 0).any() and (cls > 0).sum() >= 8 and (cls >= SHAPE[4] - 3).any()
    assert cls.max() < SHAPE[4] and (cls[:, 1] > 0).all()
    idx = DR.nearest_in_sets(torch.from_numpy(pc), torch.from_numpy(ep["pc_coord_cropped_final_unnormalized"]), torch.from_numpy(det[:, :, :6])).numpy()
    assert (idx[:, 1] == -1).all()                                                  # the empty row
    inside = (idx >= 0).sum(-1)
    assert (np.delete(inside, 1, axis=1) > 0).all() and inside.max() < SHAPE[2]
    assert idx.max() < SHAPE[3]


def test_literal_restatement_against_the_exact_sums_and_the_ordering(stage):
    pc, ep = stage
    b, r, n, p, c = SHAPE
    det = ep["detections"]
    cls = det[:, :, 6].astype(np.int32)
    idx = DR.nearest_in_sets(torch.from_numpy(pc), torch.from_numpy(ep["pc_coord_cropped_final_unnormalized"]), torch.from_numpy(det[:, :, :6])).numpy()
    groups_seen = set()
    for i in range(b):
        lit = PR.output_prediction(pc[i], ep["rpointnet_mask_selected"][i], ep["pc_coord_cropped_final_unnormalized"][i], det[i],
                                   ep["sem_class_logits"][i], ep["pc_seed"][i], ep["fb_prob"][i])
        sem_prob, fb = PR.point_tables(pc[i], ep["sem_class_logits"][i], ep["pc_seed"][i], ep["fb_prob"][i])
        sc, fc, mask, points = PR.confidence_fsum(idx[i:i + 1], ep["rpointnet_mask_selected"][i:i + 1], cls[i:i + 1], sem_prob[None], fb[None])
        order, count, label_ids, confidence, score = PR.rank(det[i:i + 1, :, 7], cls[i:i + 1], sc, fc)
        nd = int(count[0])
        assert nd == (cls[i] > 0).sum() == len(lit["rows"])
        assert np.array_equal(order[0, :nd], lit["rows"])                           # separated scores: both orders are the same
        assert np.array_equal(order[0, nd:], np.where(cls[i] <= 0)[0])
        assert sorted(order[0].tolist()) == list(range(r))
        assert PR.within_bound(lit["sem_conf"], sc[0][order[0, :nd]], n) and PR.within_bound(lit["fb_conf"], fc[0][order[0, :nd]], n)
        assert np.array_equal(lit["group_label_pred"], mask[0][order[0, :nd]]) and lit["group_label_pred"].dtype == np.int32
        assert np.array_equal(points[0], mask[0].sum(-1))
        assert np.array_equal(label_ids[0, :nd], lit["seg_label_pred"]) and not label_ids[0, nd:].any()
        assert np.array_equal(confidence[0, :nd], lit["confidence_pred"].astype(np.float32)) and not confidence[0, nd:].any()
        assert "%f" % confidence[0, nd - 1] == "%f" % lit["confidence_pred"][-1]
        assert PR.within_bound(score[0, :nd], lit["score"], n) and not score[0, nd:].any()
        groups_seen |= set(lit["confidence_pred"].tolist())
        first = int((lit["confidence_pred"] == 1).sum())
        assert np.all(np.diff(lit["score"][:first]) < 0) and np.all(np.diff(lit["score"][first:]) < 0)
        assert points[0, 1] == 0 and sc[0, 1] == 0 and fc[0, 1] == 0                # the empty row: 0 / 1e-8
    assert groups_seen == {1.0, 0.97}


def test_ordering_restatement_puts_the_lower_row_first_among_equals():
    det_score = np.array([[0.5, 0.5, 0.9, 0.5, 0.2]], np.float32)
    cls = np.array([[2, 2, 0, 2, 18]], np.int32)
    sc, fc = np.full((1, 5), 0.5), np.full((1, 5), 0.5)
    sc[0, 4] = 0.01                                                                 # exactly the threshold: strict >, so group 1
    order, count, label_ids, confidence, score = PR.rank(det_score, cls, sc, fc)
    assert order.tolist() == [[0, 1, 3, 4, 2]] and count.tolist() == [4]
    assert label_ids.tolist() == [[4, 4, 4, 39, 0]]
    assert confidence.tolist() == [[1.0, 1.0, 1.0, np.float32(0.97), 0.0]]
    assert score[0, 0] == 0.5 * 0.5 * 0.5 and score[0, 4] == 0.0


# ---- the host IO ---------------------------------------------------------------------------------------------------------------------------

def hand_pred():
    """two scenes of four points: scene 0 has three predictions, the second with an empty mask; scene 1 has none"""
    masks = torch.zeros(2, 4, 4, dtype=torch.uint8)
    masks[0, 0] = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)
    masks[0, 2] = torch.tensor([0, 1, 1, 1], dtype=torch.uint8)
    return dict(order=torch.tensor([[2, 0, 3, 1], [0, 1, 2, 3]], dtype=torch.int32), count=torch.tensor([3, 0], dtype=torch.int32),
                label_ids=torch.tensor([[3, 5, 39, 0], [0, 0, 0, 0]], dtype=torch.int32),
                confidence=torch.tensor([[1.0, 1.0, 0.97, 0.0], [0, 0, 0, 0]], dtype=torch.float32),
                masks=masks, mask_points=masks.sum(-1).int())


def read(path):
    with open(path) as f:
        return f.read()


def test_write_predictions_matches_literal_text(tmp_path):
    from gspn_amd.predict import write_predictions
    pred = hand_pred()
    out = str(tmp_path / "pred")
    os.makedirs(out)
    assert write_predictions(out, "scene0011_00", pred, 0) == 2
    assert read(os.path.join(out, "scene0011_00.txt")) == ("pred_mask/scene0011_00_0.txt 3 1.000000\n"
                                                           "pred_mask/scene0011_00_2.txt 39 0.970000\n")
    assert read(os.path.join(out, "pred_mask", "scene0011_00_0.txt")) == "1\n0\n1\n0\n"
    assert read(os.path.join(out, "pred_mask", "scene0011_00_2.txt")) == "0\n1\n1\n1\n"
    assert sorted(os.listdir(os.path.join(out, "pred_mask"))) == ["scene0011_00_0.txt", "scene0011_00_2.txt"]      # the empty mask keeps its number
    # a scene with no detection: an empty list file
    assert write_predictions(out, "scene0012_00", pred, 1) == 0
    assert read(os.path.join(out, "scene0012_00.txt")) == ""
    assert len(os.listdir(os.path.join(out, "pred_mask"))) == 2
    # and the restated exporter writes the same bytes
    ref = str(tmp_path / "ref")
    os.makedirs(ref)
    PR.export_instance_ids_for_eval_customized(os.path.join(ref, "scene0011_00.txt"), pred["label_ids"][0, :3].numpy(),
                                               pred["masks"][0, :3].numpy().astype(np.int32), np.array([1.0, 1.0, 0.97]))
    for rel in ("scene0011_00.txt", "pred_mask/scene0011_00_0.txt", "pred_mask/scene0011_00_2.txt"):
        assert read(os.path.join(ref, rel)) == read(os.path.join(out, rel))
    assert sorted(os.listdir(os.path.join(ref, "pred_mask"))) == sorted(os.listdir(os.path.join(out, "pred_mask")))


def test_write_ground_truth_matches_literal_text(tmp_path):
    from gspn_amd.predict import write_ground_truth
    seg = torch.tensor([0, 1, 18, 11, 1], dtype=torch.int32)
    group = torch.tensor([0, 3, 1, 12, 3], dtype=torch.int64)
    out = str(tmp_path / "gt")
    write_ground_truth(out, "scene0011_00", seg, group)
    assert read(os.path.join(out, "scene0011_00.txt")) == "0\n3003\n39001\n14012\n3003\n"
    PR.gen_gt(str(tmp_path / "ref"), "scene0011_00", seg.numpy(), group.numpy())
    assert read(str(tmp_path / "ref" / "scene0011_00.txt")) == read(os.path.join(out, "scene0011_00.txt"))
    write_ground_truth(out, "lists", [2, 0], [7, 0], label_map=(0, 10, 20))        # plain sequences and another map
    assert read(os.path.join(out, "lists.txt")) == "20007\n0\n"
    with pytest.raises(ValueError):
        write_ground_truth(out, "bad", seg, group[:3])


# ---- the shape and dtype rules ------------------------------------------------------------------------------------------------------------

def test_shape_and_dtype_rules_raise_value_error():
    from gspn_amd import predict
    pc, ep = PR.stage_inputs(2, 3, 50, 4, 19, seed=1, ladder=False, empty_row=False)
    with pytest.raises(ValueError):
        predict.scene_predictions({k: v for k, v in ep.items() if k != "detections"}, pc)
    with pytest.raises(ValueError):
        predict.scene_predictions(ep, pc.double())
    with pytest.raises(ValueError):
        predict.scene_predictions(ep, pc[:, :, :2])
    with pytest.raises(ValueError):
        predict.scene_predictions(ep, pc[:, :40])                                   # the logits have another N
    with pytest.raises(ValueError):
        predict.scene_predictions(dict(ep, detections=ep["detections"][:, :, :7]), pc)
    with pytest.raises(ValueError):
        predict.scene_predictions(dict(ep, rpointnet_mask_selected=ep["rpointnet_mask_selected"][:, :2]), pc)
    with pytest.raises(ValueError):
        predict.scene_predictions(dict(ep, pc_coord_cropped_final_unnormalized=ep["pc_coord_cropped_final_unnormalized"][:1]), pc)
    with pytest.raises(ValueError):
        predict.scene_predictions(ep, pc, label_map=(0, 1, 2))                      # not one entry per class
    idx = torch.zeros(2, 3, 50, dtype=torch.int32)
    masks, cls = ep["rpointnet_mask_selected"], ep["detections"][:, :, 6].int()
    sem, fb = torch.zeros(2, 50, 19), torch.zeros(2, 50)
    with pytest.raises(ValueError):
        predict.scene_confidence(idx.long(), masks, cls, sem, fb)
    with pytest.raises(ValueError):
        predict.scene_confidence(idx, masks, cls.float(), sem, fb)
    with pytest.raises(ValueError):
        predict.scene_confidence(idx, masks, cls, sem[:, :49], fb)
    with pytest.raises(ValueError):
        predict.scene_confidence(idx, masks, cls, sem, fb, mask_th=float("nan"))
    conf = torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(ValueError):
        predict.scene_rank(torch.zeros(2, 3), cls, conf.float(), conf)
    with pytest.raises(ValueError):
        predict.scene_rank(torch.zeros(2, 4), cls, conf, conf)
    with pytest.raises(NotImplementedError):
        predict.scene_rank(torch.zeros(1, 1025), torch.zeros(1, 1025, dtype=torch.int32), torch.zeros(1, 1025, dtype=torch.float64),
                           torch.zeros(1, 1025, dtype=torch.float64))
    logits, labels = torch.zeros(4, 10, 19), torch.zeros(4, 10, dtype=torch.int32)
    with pytest.raises(ValueError):
        predict.semantic_iou_counts(logits, labels.long())
    with pytest.raises(ValueError):
        predict.semantic_iou_counts(logits, labels[:, :9])
    with pytest.raises(ValueError):
        predict.semantic_iou_counts(logits[:, :, :1], labels)
    with pytest.raises(ValueError):
        predict.semantic_iou_counts(logits, labels, inter=torch.zeros(18, dtype=torch.int64))
    with pytest.raises(ValueError):
        predict.semantic_iou_counts(logits, labels, torch.zeros(17, dtype=torch.int64), torch.zeros(18, dtype=torch.int64))
    with pytest.raises(ValueError):
        predict.semantic_iou_counts(logits, labels, torch.zeros(18, dtype=torch.int32), torch.zeros(18, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        predict.semantic_iou_counts(torch.zeros(4, 257), torch.zeros(4, dtype=torch.int32))


# ---- mean_iou -------------------------------------------------------------------------------------------------------------------------------

def test_mean_iou_matches_the_restatement():
    from gspn_amd.predict import mean_iou
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((3, 400, 19)).astype(np.float32)
    labels = rng.integers(0, 19, (3, 400)).astype(np.int32)
    labels[labels == 7] = 0
    logits[:, :, 7] = -50.0                                                         # class 7 never occurs: 0 / 1e-8
    inter, union = PR.iou_counts(logits, labels, 19)
    assert union[6] == 0 and inter[6] == 0 and union.sum() > 0 and (inter <= union).all()
    got = mean_iou(torch.from_numpy(inter), torch.from_numpy(union))
    # 18 non-negative quotients, each the same double in both; the two means may add them in another order: the bound of the sums, n = 18
    assert got.dtype == torch.float64 and PR.within_bound(np.float64(float(got)), PR.mean_iou(inter, union), 18)
    # since golden/predict/iou_ref.npz: mean_iou adds in np.mean's order, so the double is the same one, at every length
    assert float(got) == float(PR.mean_iou(inter, union))
    for n in (1, 7, 8, 17, 127, 128, 129, 255):
        i = rng.integers(0, 1000, n)
        u = i + rng.integers(0, 1000, n)
        assert float(mean_iou(torch.from_numpy(i), torch.from_numpy(u))) == float(PR.mean_iou(i, u)), n
    assert torch.equal(torch.from_numpy(inter).double() / (torch.from_numpy(union).double() + 1e-8), torch.from_numpy(inter / (union + 1e-8)))
    again = PR.iou_counts(logits, labels, 19, inter.copy(), union.copy())           # a second batch adds
    assert np.array_equal(again[0], 2 * inter) and np.array_equal(again[1], 2 * union)
    assert float(mean_iou(torch.zeros(18, dtype=torch.int64), torch.zeros(18, dtype=torch.int64))) == 0.0
