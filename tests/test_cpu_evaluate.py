"""CPU tests of gspn_amd/evaluate.py: the two entry points of csrc/evaluate.hip in the library, the header and the binding (additive at
ABI 20), their host-side argument rules (no launch), average_precision on worked cases, the thresholds, the wrappers' errors, the readers on
files the two writers produce, the result file and tools/evaluate.py's arguments."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_symbols_are_exported_declared_and_bound_at_abi_20():
    from gspn_amd import _lib, build
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    assert int(re.search(r"#define GSPN_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gspn_abi_version() >= 20
    assert re.search(r"^/\* Additive at 20: gspn_instance_overlaps / gspn_instance_match\.", text, flags=re.M)
    assert re.search(r"^ \*\s+20: gspn_batch_assemble / gspn_adam_tf_flat / gspn_momentum_flat / gspn_scalars_accumulate\. \*/$", text, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("gspn_instance_overlaps", 14), ("gspn_instance_match", 20)):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        declared = [a.strip() for a in re.search(r"\bint %s\s*\(([^)]*)\)" % name, code).group(1).split(",")]
        bound = _lib.SIGNATURES[name]
        assert len(declared) == len(bound) == nargs
        assert [a.startswith("int ") for a in declared] == [a is ctypes.c_int for a in bound]            # the extents by value, everything else a pointer
        assert all(("*" in a) == (b is ctypes.c_void_p) for a, b in zip(declared, bound))
    from gspn_amd import evaluate
    for macro, value in (("GSPN_INSTANCE_MAX_G", evaluate.INSTANCE_MAX_G), ("GSPN_INSTANCE_MAX_CG", evaluate.INSTANCE_MAX_CG),
                         ("GSPN_INSTANCE_MATCH_MAX_R", evaluate.INSTANCE_MATCH_MAX_R)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == value
    assert "evaluate.hip" not in build.POLICY_SOURCES


def test_host_side_argument_rules_launch_nothing():
    from gspn_amd import _lib
    lib = _lib.lib()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)                               # never dereferenced: every call below returns before a launch
    for at in range(8):
        ptrs = [p] * 8
        ptrs[at] = null
        assert lib.gspn_instance_overlaps(1, 2, 10, 4, 3, *ptrs, null) == -1
    for extents in ((0, 2, 10, 4, 3), (1, 0, 10, 4, 3), (1, 2, 0, 4, 3), (1, 2, 10, 0, 3), (1, 2, 10, 4, 0), (1, 2, -5, 4, 3)):
        assert lib.gspn_instance_overlaps(*extents, *[p] * 8, null) == -1
    assert lib.gspn_instance_overlaps(1, 2, 10, 1, 4097, *[p] * 8, null) == -2
    assert lib.gspn_instance_overlaps(1, 2, 10, 3, 2731, *[p] * 8, null) == -2      # c * g = 8193
    assert lib.gspn_instance_overlaps(1 << 16, 1 << 15, 10, 2, 2, *[p] * 8, null) == -2
    for at in range(13):
        ptrs = [p] * 13
        ptrs[at] = null
        assert lib.gspn_instance_match(1, 4, 3, 2, 10, 100, *ptrs, null) == -1
    for extents in ((0, 4, 3, 2, 10), (1, 0, 3, 2, 10), (1, 4, 0, 2, 10), (1, 4, 3, 0, 10), (1, 4, 3, 2, 0)):
        assert lib.gspn_instance_match(*extents, 100, *[p] * 13, null) == -1
    assert lib.gspn_instance_match(1, 1025, 3, 2, 10, 100, *[p] * 13, null) == -2
    assert lib.gspn_instance_match(1, 4, 3, 2, 10, 0, *[p] * 13, null) == -2        # min_region >= 1


def test_average_precision_worked_cases():
    from gspn_amd.evaluate import average_precision
    assert average_precision([1, 0, 1, 0, 0], [1.0, 1.0, 0.97, 0.97, 0.97], 1) == 0.4
    assert average_precision([1, 1, 0], [0.9, 0.5, 0.7], 0) == 0.7916666666666666
    assert average_precision([0, 1, 1], [0.7, 0.5, 0.9], 0) == 0.7916666666666666  # the order of the records is nothing
    # by hand: scores 0.5 < 0.7 < 0.9, precision 2/3, 1/2, 1 and 1; recall 1, 1/2, 1/2 and 0; four steps of 1/4
    assert average_precision([1, 1, 0], [0.9, 0.5, 0.7], 0) == pytest.approx((2 / 3 + 0.5 + 1 + 1) / 4, abs=1e-15)


def test_average_precision_empty_and_single_record():
    from gspn_amd.evaluate import average_precision
    assert average_precision([], [], 0) == 0.0 and average_precision([], [], 3) == 0.0
    assert average_precision([1], [0.5], 0) == 1.0
    assert average_precision([1], [0.5], 1) == 0.5                                  # precision 1, recall 1/2
    assert average_precision([0], [0.5], 1) == 0.0
    assert average_precision([0], [0.5], 0) == 0.0                                  # no gt at all: recall counts as 0
    with pytest.raises(ValueError):
        average_precision([1, 0], [0.5], 0)


def test_default_overlaps_are_the_numpy_expression_bit_for_bit():
    from gspn_amd import evaluate
    want = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
    assert evaluate.DEFAULT_OVERLAPS.dtype == np.float64 and evaluate.DEFAULT_OVERLAPS.tobytes() == want.tobytes() and len(want) == 10
    assert evaluate.MIN_REGION_SIZE == 100
    metric = evaluate.InstanceAP(19)
    assert metric.overlaps.tobytes() == want.tobytes() and metric.class_names == evaluate.SCANNET_CLASS_NAMES and len(metric.class_names) == 18
    empty = metric.compute()                                                        # nothing added: every class without a gt
    assert empty["ap"].shape == (18, 10) and np.isnan(empty["ap"]).all() and np.isnan(empty["all_ap"]) and empty["class_ids"][:3] == [3, 4, 5]


def test_wrappers_raise_before_a_launch():
    from gspn_amd import _lib, evaluate
    masks = torch.zeros(2, 3, 50, dtype=torch.uint8)
    cls, seg, group = torch.ones(2, 3, dtype=torch.int32), torch.zeros(2, 50, dtype=torch.int32), torch.zeros(2, 50, dtype=torch.int32)
    with pytest.raises(TypeError):
        evaluate.instance_overlaps(masks.numpy(), cls, seg, group, 4, 5)
    for bad in ((masks.int(), cls, seg, group), (masks, cls.long(), seg, group), (masks, cls, seg.long(), group), (masks, cls, seg, group.float()),
                (masks[0], cls, seg, group), (masks, cls[:, :2], seg, group), (masks, cls, seg[:, :49], group), (masks, cls, seg, group[:1]),
                (masks[:, :, :0], cls, seg[:, :0], group[:, :0])):
        with pytest.raises(ValueError):
            evaluate.instance_overlaps(*bad, 4, 5)
    with pytest.raises(ValueError):
        evaluate.instance_overlaps(masks, cls, seg, group, 4, 0)
    with pytest.raises(NotImplementedError):
        evaluate.instance_overlaps(masks, cls, seg, group, 2, 4097)
    with pytest.raises(NotImplementedError):
        evaluate.instance_overlaps(masks, cls, seg, group, 3, 2731)
    with pytest.raises(_lib.GspnHipError):                                          # well-formed CPU tensors: no CPU path
        evaluate.instance_overlaps(masks, cls, seg, group, 4, 5)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    good = dict(inter=z(2, 3, 5), void_count=z(2, 3), pred_count=z(2, 3), pred_class=z(2, 3), confidence=torch.zeros(2, 3), count=z(2), gt_count=z(2, 4, 5))
    for name, bad in (("inter", z(2, 3, 5).long()), ("inter", z(2, 3)), ("void_count", z(2, 4)), ("pred_count", z(3, 3)), ("pred_class", z(2, 3).float()),
                      ("confidence", torch.zeros(2, 3, dtype=torch.float64)), ("count", z(3)), ("count", z(2, 1)), ("gt_count", z(2, 4, 6)),
                      ("gt_count", z(1, 4, 5))):
        with pytest.raises(ValueError):
            evaluate.instance_match(**dict(good, **{name: bad}))
    with pytest.raises(ValueError):
        evaluate.instance_match(**good, thresholds=[])
    with pytest.raises(ValueError):
        evaluate.instance_match(**good, thresholds=[0.5, float("nan")])
    with pytest.raises(ValueError):
        evaluate.instance_match(**good, thresholds=torch.zeros(3))                  # a tensor of thresholds is float64
    with pytest.raises(NotImplementedError):
        evaluate.instance_match(**good, min_region=0)
    with pytest.raises(NotImplementedError):
        evaluate.instance_match(z(1, 1025, 2), z(1, 1025), z(1, 1025), z(1, 1025), torch.zeros(1, 1025), z(1), z(1, 2, 2))
    with pytest.raises(_lib.GspnHipError):
        evaluate.instance_match(**good)
    with pytest.raises(ValueError):
        evaluate.classes_from_label_ids(torch.zeros(3, dtype=torch.int64))
    with pytest.raises(_lib.GspnHipError):
        evaluate.classes_from_label_ids(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        evaluate.InstanceAP(1)
    with pytest.raises(ValueError):
        evaluate.InstanceAP(5)                                                      # the default label map has 19 entries
    with pytest.raises(ValueError):
        evaluate.InstanceAP(3, label_map=(0, 4, 4))
    with pytest.raises(ValueError):
        evaluate.InstanceAP(3, label_map=(0, 4, 5), class_names=("one",))
    with pytest.raises(ValueError):
        evaluate.InstanceAP(19).add_predictions({"masks": masks}, seg, group, 5)


# ---- the readers, on what the two writers write ---------------------------------------------------------------------------------------------

def hand_pred():
    """two scenes of four points: scene 0 has three predictions, the second with an empty mask; scene 1 has none"""
    masks = torch.zeros(2, 4, 4, dtype=torch.uint8)
    masks[0, 0] = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)
    masks[0, 2] = torch.tensor([0, 1, 1, 1], dtype=torch.uint8)
    return dict(count=torch.tensor([3, 0], dtype=torch.int32), label_ids=torch.tensor([[3, 5, 39, 0], [0, 0, 0, 0]], dtype=torch.int32),
                confidence=torch.tensor([[1.0, 1.0, 0.97, 0.0], [0, 0, 0, 0]], dtype=torch.float32), masks=masks, mask_points=masks.sum(-1).int())


def test_readers_read_what_the_writers_write(tmp_path):
    from gspn_amd.evaluate import read_ground_truth, read_predictions
    from gspn_amd.predict import write_ground_truth, write_predictions
    pred, out = hand_pred(), str(tmp_path / "pred")
    write_predictions(out, "scene0011_00", pred, 0)
    write_predictions(out, "scene0012_00", pred, 1)
    masks, labels, confidence = read_predictions(out, "scene0011_00", 4)
    assert masks.dtype == np.uint8 and labels.dtype == np.int32 and confidence.dtype == np.float32
    assert masks.tolist() == [[1, 0, 1, 0], [0, 1, 1, 1]] and labels.tolist() == [3, 39]          # the empty row 1 was skipped
    assert confidence.tolist() == [1.0, float(np.float32(0.97))]
    masks, labels, confidence = read_predictions(out, "scene0012_00", 4)
    assert masks.shape == (0, 4) and labels.shape == (0,) and confidence.shape == (0,)
    with pytest.raises(ValueError):
        read_predictions(out, "scene0011_00", 5)                                    # a mask of the wrong length
    seg, group = torch.tensor([0, 1, 18, 11, 1, 0], dtype=torch.int32), torch.tensor([0, 3, 1, 12, 3, 7], dtype=torch.int64)
    gt = str(tmp_path / "gt")
    write_ground_truth(gt, "scene0011_00", seg, group)
    got_seg, got_group = read_ground_truth(gt, "scene0011_00")
    assert got_seg.dtype == got_group.dtype == np.int32 and got_seg.tolist() == seg.tolist() and got_group.tolist() == group.tolist()
    write_ground_truth(gt, "other", [2, 0, 1], [7, 0, 999], label_map=(0, 10, 20))
    assert [a.tolist() for a in read_ground_truth(gt, "other", (0, 10, 20))] == [[2, 0, 1], [7, 0, 999]]
    with pytest.raises(ValueError):
        read_ground_truth(gt, "other")                                              # 20 is no label id of the ScanNet map
    with pytest.raises(ValueError):
        read_ground_truth(gt, "scene0011_00", (0, 3, 4))


def test_write_result_file_format(tmp_path):
    from gspn_amd.evaluate import write_result_file
    result = {"class_names": ["cabinet", "shower curtain"], "class_ids": [3, 28],
              "classes": {"cabinet": {"ap": 0.25, "ap50%": 0.5, "ap25%": 1.0}, "shower curtain": {"ap": float("nan"), "ap50%": float("nan"), "ap25%": float("nan")}}}
    path = str(tmp_path / "result.txt")
    write_result_file(path, result)
    assert open(path).read() == "class,class id,ap,ap50,ap25\ncabinet,3,0.25,0.5,1.0\nshower curtain,28,nan,nan,nan\n"


def test_tool_arguments(tmp_path):
    spec = importlib.util.spec_from_file_location("evaluate_tool", os.path.join(ROOT, "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(["--pred_path", "eva/pred", "--gt_path", "eva/gt"])
    assert (a.pred_path, a.gt_path, a.scan_list) == ("eva/pred", "eva/gt", "") and a.output_file == os.path.join("eva/pred", "semantic_instance_evaluation.txt")
    a = tool.parse_args(["--pred_path", "p", "--gt_path", str(tmp_path), "--output_file", "out.csv"])
    assert a.output_file == "out.csv"
    with pytest.raises(SystemExit):
        tool.parse_args(["--pred_path", "p"])
    for name in ("scene0002_00.txt", "scene0001_00.txt", "notes.md"):
        (tmp_path / name).write_text("")
    assert tool.scan_names(a) == ["scene0001_00", "scene0002_00"]                   # every *.txt of gt_path
    (tmp_path / "list").write_text("scene0002_00\n\n")
    a = tool.parse_args(["--pred_path", "p", "--gt_path", str(tmp_path), "--scan_list", str(tmp_path / "list")])
    assert tool.scan_names(a) == ["scene0002_00"]
    result = {"class_names": ["bed"], "classes": {"bed": {"ap": 0.5, "ap50%": 0.75, "ap25%": 1.0}}, "all_ap": 0.5, "all_ap_50%": 0.75, "all_ap_25%": 1.0}
    lines = tool.format_table(result)
    assert any(re.fullmatch(r"bed\s+:\s+0\.500\s+0\.750\s+1\.000", line) for line in lines)
    assert any(re.fullmatch(r"average\s+:\s+0\.500\s+0\.750\s+1\.000", line) for line in lines)
