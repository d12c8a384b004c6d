"""CPU checks of the detection output stage (no GPU needed): the restatement of the per-class NMS in tests/detect_ref.py equals what the
reference's own nms_3d gives class by class (tests/golden/detect/class_nms_ref.npz, tools/make_golden_detect.py), the one-pass formulation
the kernel uses equals that per-class loop, the golden cases hold what they are there for, select_segmentation's restatement equals plain
indexing, the entry points of csrc/detect.hip exist and reject bad sizes, and the names are exported."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import detect_ref as DR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect", "class_nms_ref.npz")


@pytest.mark.parametrize("name", sorted(DR.CLASS_NMS_CASES))
def test_class_nms_restatement_equals_the_reference_function_per_class(name):
    z = np.load(GOLDEN)
    boxes, scores, class_ids, per_class, m, thr = DR.class_nms_case(name)
    assert np.array_equal(boxes.numpy(), z[name + "/boxes"]) and np.array_equal(scores.numpy(), z[name + "/scores"])
    assert np.array_equal(class_ids.numpy(), z[name + "/class_ids"]) and z[name + "/args"].tolist() == [per_class, m, thr]
    for row in scores:
        assert row.unique().numel() == row.numel()               # the reference's argsort leaves the order of equal scores open
    got = DR.class_nms(boxes, scores, class_ids, per_class, m, thr)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), z[name + "/selected"])


@pytest.mark.parametrize("name", sorted(DR.CLASS_NMS_CASES))
def test_one_pass_formulation_equals_the_per_class_loop(name):
    z = np.load(GOLDEN)
    boxes, scores, class_ids, per_class, m, thr = DR.class_nms_case(name)
    assert np.array_equal(DR.class_nms_one_pass(boxes, scores, class_ids, per_class, m, thr).numpy(), z[name + "/selected"])
    # and with fewer outputs than survivors, fewer picks per class, equal scores
    tied = (torch.floor(scores * 8) / 8).contiguous()
    for pc, mo in ((per_class, 7), (2, m), (1, 3)):
        assert torch.equal(DR.class_nms_one_pass(boxes, tied, class_ids, pc, mo, thr), DR.class_nms(boxes, tied, class_ids, pc, mo, thr))


def test_class_nms_golden_cases_hold_what_they_are_for():
    z = np.load(GOLDEN)
    sel = {name: z[name + "/selected"] for name in DR.CLASS_NMS_CASES}
    assert (sel["detect_384"] >= 0).all() and (sel["detect_zero_volume"] >= 0).all()          # more survivors than outputs
    ids = z["per_class_5/class_ids"]
    for i in range(2):                                                                        # every class reaches max_per_class
        picked = sel["per_class_5"][i][sel["per_class_5"][i] >= 0]
        assert np.bincount(ids[i][picked], minlength=4).tolist() == [0, 5, 5, 5]
    assert (sel["empty_scene"][1] == -1).all() and not (z["empty_scene/class_ids"][1] > 0).any()
    assert (sel["empty_scene"][0] >= 0).all() and (sel["fewer_than_outputs"][0] >= 0).sum() < 40
    # a picked zero-volume box: its class has no pick of lower score (the reference picks it until the class is full), and it comes once
    found = 0
    for name in ("detect_zero_volume", "few_classes_0.5", "empty_scene"):
        boxes, scores, cls = z[name + "/boxes"], z[name + "/scores"], z[name + "/class_ids"]
        per_class, m, thr = z[name + "/args"].tolist()
        full = DR.class_nms(torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(cls), int(per_class), boxes.shape[1], thr).numpy()
        for i in range(len(boxes)):
            picked = full[i][full[i] >= 0]
            assert len(np.unique(picked)) == len(picked)
            assert np.array_equal(picked[:int(m)], sel[name][i][sel[name][i] >= 0])
            for k in picked:
                if boxes[i, k, 3:].prod() == 0:
                    found += 1
                    same = picked[cls[i][picked] == cls[i][k]]
                    assert scores[i][same].min() == scores[i][k]
    assert found >= 5


def test_class_nms_restatement_ties_and_zero_volume():
    # equal scores within and across classes: the lower index first; row 3 (class 1) overlaps row 0 and leaves, row 4 is background
    boxes = torch.tensor([[[0.0, 0, 0, 1, 1, 1], [5.0, 0, 0, 1, 1, 1], [10.0, 0, 0, 1, 1, 1], [0.1, 0, 0, 1, 1, 1], [20.0, 0, 0, 1, 1, 1],
                           [0.1, 0, 0, 1, 1, 1]]])
    scores = torch.tensor([[0.5, 0.9, 0.5, 0.5, 0.95, 0.5]])
    cls = torch.tensor([[1, 2, 2, 1, 0, 2]], dtype=torch.int32)
    for fn in (DR.class_nms, DR.class_nms_one_pass):
        assert fn(boxes, scores, cls, 6, 6, 0.5).tolist() == [[1, 0, 2, 5, -1, -1]]            # 5 overlaps 0, but is of another class
        assert fn(boxes, scores, cls, 1, 6, 0.5).tolist() == [[1, 0, -1, -1, -1, -1]]
    # a zero-volume box on top of class 1 exhausts class 1 only
    boxes[0, 0, 3] = 0.0
    scores[0, 0] = 0.99
    for fn in (DR.class_nms, DR.class_nms_one_pass):
        assert fn(boxes, scores, cls, 6, 6, 0.5).tolist() == [[0, 1, 2, 5, -1, -1]]


def test_select_segmentation_restatement_equals_plain_indexing():
    g = torch.Generator().manual_seed(0)
    masks = torch.randn(2, 5, 7, 4, generator=g)
    ids = torch.randint(0, 4, (2, 5), generator=g)
    got = DR.select_segmentation(masks, ids)
    assert got.shape == (2, 5, 7)
    for i in range(2):
        for k in range(5):
            assert torch.equal(got[i, k], masks[i, k, :, int(ids[i, k])])
    assert torch.equal(DR.select_segmentation(masks, ids.float()), got)


def test_nearest_restatement_first_index_and_gate():
    query = torch.tensor([[[0.0, 0, 0], [1.0, 0, 0], [0.5, 0, 0], [3.0, 0, 0]]])
    sets = torch.tensor([[[[1.0, 0, 0], [0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0]]]])
    assert DR.nearest_in_sets(query, sets).tolist() == [[[1, 0, 0, 0]]]                        # 0.5 is equally far from both: position 0
    rois = torch.tensor([[[0.5, 0, 0, 1.0, 1.0, 1.0]]])
    assert DR.nearest_in_sets(query, sets, rois).tolist() == [[[1, 0, 0, -1]]]                 # the faces 0 and 1 are inside
    first, prob = DR.first_argmax(torch.tensor([[0.2, 0.4, 0.4], [0.5, 0.5, 0.0]]))
    assert first.tolist() == [1, 0] and prob.tolist() == [0.4000000059604645, 0.5]


def test_detect_entry_points_exist_and_reject_bad_sizes():
    from gspn_amd import _lib, build
    build.build()
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    f = ctypes.c_float
    for name in ("gspn_class_nms3d", "gspn_nearest_in_sets"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION >= 14
    for b, n, k, m in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (4, -1, 4, 4), (4, 4, -1, 4), (4, 4, 4, -1)):
        assert lib.gspn_class_nms3d(b, n, k, m, f(0.1), null, null, null, null, null) == -1
    for b, r, n, p in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (4, -1, 4, 4), (4, 4, -1, 4), (4, 4, 4, -1)):
        assert lib.gspn_nearest_in_sets(b, r, n, p, null, null, null, null, null) == -1
    # valid sizes beyond what the kernels support: GSPN_ERR_UNSUPPORTED, before anything is launched
    assert lib.gspn_class_nms3d(1, 4097, 4, 4, f(0.1), null, null, null, null, null) == -2
    assert lib.gspn_nearest_in_sets(1, 1, 4, 4097, null, null, null, null, null) == -2
    assert lib.gspn_nearest_in_sets(1, 1, 32769, 4, null, null, null, null, null) == -2


def test_detect_names_are_exported_and_cpu_tensors_are_refused():
    from gspn_amd import rpointnet as RP
    from gspn_amd._lib import GspnHipError
    for name in ("class_nms_3d", "refine_detections", "refine_detections_batch", "select_segmentation", "nearest_in_sets", "unmold_segmentation"):
        assert name in RP.__all__ and callable(getattr(RP, name))
    with pytest.raises(GspnHipError):
        RP.class_nms_3d(torch.zeros(1, 4, 6), torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int32), 2, 2, 0.1)
    with pytest.raises(GspnHipError):
        RP.nearest_in_sets(torch.zeros(1, 4, 3), torch.zeros(1, 2, 5, 3))
    with pytest.raises(ValueError):
        RP.class_nms_3d(torch.zeros(1, 4, 6, dtype=torch.float64), torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int32), 2, 2, 0.1)
    g =torch.Generator().manual_seed(1)
    masks, ids = torch.randn(2, 3, 5, 4, generator=g), torch.randint(0, 4, (2, 3), generator=g)
    assert torch.equal(RP.select_segmentation(masks, ids), DR.select_segmentation(masks, ids))  # plain tensor code: runs anywhere
    with pytest.raises(ValueError):
        RP.select_segmentation(masks, ids[:, :2])
