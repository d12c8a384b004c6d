"""CPU checks of the ROI stage (no GPU needed): the restatement of nms_3d in tests/roi_ref.py equals the outputs of the reference's own
function stored in tests/golden/roi/nms3d_ref.npz (tools/make_golden_roi.py), the entry points of csrc/roi.hip exist and reject bad
sizes, the restated random number generator is the one include/gspn_hip.h specifies and is uniform, the seeded target inputs have the
properties the GPU tests rely on, and the tensor-only helpers equal the reference's formulas."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import roi_ref as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi", "nms3d_ref.npz")


@pytest.mark.parametrize("name", sorted(RR.NMS_CASES))
def test_nms_restatement_equals_the_reference_function(name):
    z = np.load(GOLDEN)
    boxes, scores, pre, m, thr, sthr = RR.nms_case(name)
    assert np.array_equal(boxes.numpy(), z[name + "/boxes"]) and np.array_equal(scores.numpy(), z[name + "/scores"])
    assert z[name + "/args"].tolist() == [pre, m, thr, sthr]
    for row in scores:
        assert row.unique().numel() == row.numel()               # the reference's argsort leaves the order of equal scores open
    got = RR.nms_3d(boxes, scores, pre, m, thr, sthr)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), z[name + "/selected"])


def test_nms_golden_cases_cover_both_exits_and_the_repeats():
    z = np.load(GOLDEN)
    picks = {name: (z[name + "/selected"] >= 0).sum(1) for name in RR.NMS_CASES}
    assert (picks["train_0.5"] == 128).all() and (picks["infer_0.5"] == 384).all()            # output full
    assert (picks["train_0.25"] < 128).all() and (picks["infer_0.1"] < 384).all()             # candidates exhausted
    assert (picks["score_threshold"] < 128).all() and (picks["fewer_boxes_than_outputs"] < 50).all()
    for name in ("train_zero_rows", "infer_zero_rows"):                                       # a zero-volume pick repeats until the output is full
        sel, boxes = z[name + "/selected"], z[name + "/boxes"]
        for i in range(sel.shape[0]):
            assert (sel[i] >= 0).all() and len(np.unique(sel[i])) < sel.shape[1] // 4
            assert not boxes[i, sel[i, -1]].any() and (sel[i, -40:] == sel[i, -1]).all()


def test_nms_restatement_takes_the_lower_index_among_equal_scores():
    boxes = torch.tensor([[[0.0, 0, 0, 1, 1, 1], [5.0, 0, 0, 1, 1, 1], [10.0, 0, 0, 1, 1, 1], [0.1, 0, 0, 1, 1, 1]]])
    scores = torch.tensor([[0.5, 0.9, 0.5, 0.5]])
    assert RR.nms_3d(boxes, scores, -1, 4).tolist() == [[1, 0, 2, -1]]                        # 3 overlaps 0 (IoU 0.82) and leaves


def test_roi_entry_points_exist_and_reject_bad_sizes():
    from gspn_amd import _lib, build
    build.build()
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    f = ctypes.c_float
    for name in ("gspn_nms3d", "gspn_box_point_count", "gspn_sample_points_in_boxes", "gspn_detection_target_select", "gspn_crop_gather_grad"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION >= 13
    for b, n, m in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -2, 4), (4, 4, -3)):
        assert lib.gspn_nms3d(b, n, 2, m, f(0.5), f(0.0), null, null, null, null) == -1
    for b, s, n in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -2, 4), (4, 4, -3)):
        assert lib.gspn_box_point_count(b, s, n, f(0.0), null, null, null, null) == -1
    for b, r, n, k in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (4, -1, 4, 4), (4, 4, -1, 4), (4, 4, 4, -1)):
        assert lib.gspn_sample_points_in_boxes(b, r, n, k, f(0.0), null, null, null, null, null) == -1
    for b, s, g, r in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (4, -1, 4, 4), (4, 4, -1, 4), (4, 4, 4, -1)):
        assert lib.gspn_detection_target_select(b, s, g, r, 1, f(3.0), null, null, null, null, null, null, null, null) == -1
    for b, n, c, ln in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (4, -1, 4, 4), (4, 4, -1, 4), (4, 4, 4, -1)):
        assert lib.gspn_crop_gather_grad(b, n, c, ln, null, null, null, null, null, null, null) == -1
    assert [lib.gspn_crop_gather_grad_part_floats(b, ln, c) for b, ln, c in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4))] == [0, 0, 0, 0]
    assert lib.gspn_crop_gather_grad_part_floats(2, 16384, 1024) == 2 * 256 * 2 * 1024 and lib.gspn_crop_gather_grad_part_floats(1, 65, 3) == 12
    # valid sizes beyond what the kernels support: GSPN_ERR_UNSUPPORTED, before anything is launched
    assert lib.gspn_nms3d(1, 4097, -1, 4, f(0.5), f(0.0), null, null, null, null) == -2
    assert lib.gspn_sample_points_in_boxes(1, 4, 32769, 4, f(0.0), null, null, null, null, null) == -2
    assert lib.gspn_detection_target_select(1, 1025, 4, 4, 1, f(3.0), null, null, null, null, null, null, null, null) == -2


def _mix_int(z):
    m = (1 << 64) - 1
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & m
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & m
    return z ^ (z >> 31)


def test_restated_generator_is_the_specified_one():
    """tests/roi_ref.py: rand32 (numpy uint64) against the formula of include/gspn_hip.h written with Python integers"""
    m = (1 << 64) - 1
    for seed, scene, a, b in ((0, 0, 0, 0), (1, 0, 0, 0), (7, 1, 63, 255), (-5, 3, 511, RR.SELECT_STREAM), (2 ** 62 + 11, 7, 2 ** 31, 1023)):
        st = _mix_int((seed + 0x9E3779B97F4A7C15 * (scene + 1)) & m)
        want = _mix_int(st ^ ((a << 32) | b)) >> 32
        assert int(RR.rand32(seed, scene, np.array([a]), np.array([b]))[0]) == want
    assert len(set(RR.rand32(3, 0, 5, np.arange(4096)).tolist())) > 4090


def test_generator_ranks_are_uniform():
    """2^16 draws on a box of 8 points: every rank's count within 5 standard deviations of uniform (a fixed property of the generator)"""
    n, k = 1 << 16, 8
    sd = np.sqrt(n * (1 / k) * (1 - 1 / k))
    for seed, scene, roi in ((0, 0, 0), (1, 0, 0), (12345, 1, 63), (2 ** 40, 5, 383)):
        ranks = RR.rank_of(RR.rand32(seed, scene, roi, np.arange(n)), k)
        assert ranks.min() >= 0 and ranks.max() < k
        hist = np.bincount(ranks, minlength=k)
        assert (np.abs(hist - n / k) <= 5 * sd).all(), hist
    keys = RR.rand32(9, 0, np.arange(n), RR.SELECT_STREAM)                                     # the selection keys, over the candidate index
    hist = np.bincount(RR.rank_of(keys, k), minlength=k)
    assert (np.abs(hist - n / k) <= 5 * sd).all(), hist


def test_seeded_target_inputs_have_the_properties_the_gpu_tests_rely_on():
    """per mix: the cap on positives binds / both sides of the negatives' min occur / many positives; empty proposals everywhere; fp32 and
    float64 decide alike, and at most 1 % of a scene's proposals lie within 1e-5 of the 0.5 threshold"""
    sc = RR.target_scene()
    gt = sc["bbox_ins"]
    seen = {name: set() for name in RR.TARGET_MIXES}
    for name, (s, njit) in RR.TARGET_MIXES.items():
        for seed in (3, 4):
            prop = RR.target_proposals(gt, s, njit, 100 + seed)
            cnt = RR.box_point_count(prop, sc["pc"])
            src32, gt32, iou32 = RR.detection_target_select(prop, cnt, gt, 64, 0.33, seed)
            src64, gt64, iou64 = RR.detection_target_select(prop, cnt, gt, 64, 0.33, seed, torch.float64)
            part = ~torch.isnan(iou64)
            assert torch.equal(part, ~torch.isnan(iou32))
            near = ((iou64 - 0.5).abs() <= 1e-5) & part
            assert int(near.sum(1).max()) <= s // 100
            assert torch.equal((iou32 >= 0.5)[part & ~near], (iou64 >= 0.5)[part & ~near])
            assert torch.equal(src32, src64) and torch.equal(gt32, gt64)
            empty = (cnt == 0) & (prop.abs().sum(-1) > 0)
            assert int(empty.sum(1).min()) >= 20 and int((prop.abs().sum(-1) == 0).sum(1).min()) == 8
            for i in range(prop.shape[0]):
                npos_all, nneg_all = int(((iou64[i] >= 0.5) & part[i]).sum()), int(((iou64[i] < 0.5) & part[i]).sum())
                npos, nneg = RR.selection_counts(npos_all, nneg_all, 64, 0.33)
                assert int((gt32[i] >= 0).sum()) == npos and int((src32[i] >= 0).sum()) == npos + nneg
                want = int(np.float32(np.float32(1 / 0.33) * np.float32(npos))) - npos
                seen[name].add(("cap" if npos_all > 21 else "all_pos", "neg_short" if nneg_all < want else "neg_enough"))
    assert seen["many_positives"] == {("cap", "neg_short")}
    assert seen["few_positives"] == {("all_pos", "neg_short"), ("all_pos", "neg_enough")}
    assert seen["wide"] == {("cap", "neg_enough")}
    assert RR.selection_counts(21, 100, 64, 0.33) == (21, 42) and RR.selection_counts(100, 100, 64, 0.33) == (21, 42)


def test_box_refinement_and_apply_box_delta():
    """plain tensor code: the reference's formulas (:553-582) in their [dz, dy, dx, dh, dw, dl] order, and each other's inverse"""
    from gspn_amd import rpointnet as RP
    g = torch.Generator().manual_seed(0)
    box = torch.cat((torch.rand(50, 3, generator=g) * 8, torch.rand(50, 3, generator=g) + 0.2), 1)
    gt = torch.cat((box[:, :3] + 0.3 * torch.randn(50, 3, generator=g), box[:, 3:] * (0.5 + torch.rand(50, 3, generator=g))), 1)
    d = RP.box_refinement(box, gt)
    assert torch.equal(d, RR.box_refinement(box, gt))
    assert torch.equal(RP.apply_box_delta(box, d), RR.apply_box_delta(box, d))
    assert torch.allclose(RP.apply_box_delta(box, d), gt, rtol=1e-5, atol=1e-6)
    assert torch.equal(RP.box_refinement(box.view(5, 10, 6), gt.view(5, 10, 6)).view(50, 6), d)


def test_roi_names_are_exported_and_cpu_tensors_are_refused():
    from gspn_amd import rpointnet as RP
    from gspn_amd._lib import GspnHipError
    for name in ("nms_3d", "detection_target_gen", "detection_target_gen_batch", "mask_selection_gen", "mask_selection_gen_batch", "points_cropping",
                 "box_refinement", "apply_box_delta", "box_point_count", "sample_points_in_boxes"):
        assert name in RP.__all__ and callable(getattr(RP, name))
    assert not hasattr(RP, "sample_points_within_box")              # the mask-matrix form is not offered
    with pytest.raises(GspnHipError):
        RP.nms_3d(torch.zeros(1, 4, 6), torch.zeros(1, 4), 2, 2)
    with pytest.raises(GspnHipError):
        RP.box_point_count(torch.zeros(1, 4, 6), torch.zeros(1, 8, 3))
    with pytest.raises(ValueError):
        RP.nms_3d(torch.zeros(1, 4, 6, dtype=torch.float64), torch.zeros(1, 4), 2, 2)
