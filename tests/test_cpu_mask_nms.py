"""CPU tests of mask NMS (gspn_amd/mask_nms.py): the four symbols in the header, the library and the binding with the ABI
still 21; the host-side declines of the entry points, which launch nothing; the sanitized host-side check program; the numpy restatement
(tests/mask_nms_ref.py) on hand-written cases and its own invariants; the wrappers' and the drivers' guards, which raise before the
library is touched; and the flag errors of tools/test.py."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import mask_nms_ref as ref
from tests.args_check import run_args_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_mask_nms_symbols_are_declared_exported_and_bound_at_abi_21():
    from gspn_amd import _lib, build, mask_nms
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    assert "#define GSPN_ABI_VERSION 21" in text and int(lib.gspn_abi_version()) == 21 == _lib.ABI_VERSION
    assert "Additive at 21: gspn_mask_overlaps, gspn_mask_nms (+ their _ws_bytes)" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("gspn_mask_overlaps", 8), ("gspn_mask_nms", 12)):
        declared = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        assert len(declared) == len(_lib.SIGNATURES[name]) == nargs and hasattr(raw, name)
    assert _lib.SIGNATURES["gspn_mask_nms"][6] is ctypes.c_double                                       # iou_th is a double across the ABI
    three = ([ctypes.c_int] * 3, ctypes.c_long)
    for name in ("gspn_mask_overlaps_ws_bytes", "gspn_mask_nms_ws_bytes"):
        assert re.search(r"\blong %s\s*\(int b, int r, int v\)" % name, code) and _lib.SPECIAL[name] == three and hasattr(raw, name)
    assert mask_nms.MASK_NMS_MAX_R == int(re.search(r"#define GSPN_MASK_NMS_MAX_R (\d+)", text).group(1)) == 1024
    assert mask_nms.MASK_NMS_MAX_V == 1 << int(re.search(r"#define GSPN_MASK_NMS_MAX_V \(1 << (\d+)\)", text).group(1)) == 1 << 24
    assert mask_nms.MASK_NMS_MAX_B == int(re.search(r"#define GSPN_MASK_NMS_MAX_B (\d+)", text).group(1)) == 65535
    assert "mask_nms.hip" not in build.POLICY_SOURCES and os.path.exists(os.path.join(build.CSRC, "mask_nms.hip"))
    # host-side declines, nothing launched
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(24)
    mo = lambda b=2, r=3, v=9, p=(one,) * 4: lib.gspn_mask_overlaps(b, r, v, p[0], p[1], p[2], p[3], null)                      # noqa: E731
    mn = lambda b=2, r=3, v=9, th=0.5, labels=one, p=(one,) * 6: lib.gspn_mask_nms(b, r, v, p[0], p[1], labels, th, p[2], p[3], p[4], p[5], null)      # noqa: E731
    assert mo(b=-1) == mo(r=-1) == mo(v=-1) == mn(b=-1) == mn(r=-1) == mn(v=-1) == -1
    assert all(mo(p=tuple(null if i == k else one for i in range(4))) == -1 for k in range(4))
    assert all(mn(p=tuple(null if i == k else one for i in range(6))) == -1 for k in range(6))
    assert all(mn(th=th) == -1 for th in (float("nan"), -1e-9, 1.0, 2.0, float("inf"), float("-inf")))
    assert mo(r=1025) == mo(v=(1 << 24) + 1) == mo(b=65536) == mn(r=1025) == mn(v=(1 << 24) + 1) == mn(b=65536) == -2
    assert mo(p=(one, odd, one, one)) == -2 and mn(p=(one, one, odd, one, one, one)) == -2              # a ws that is not 16-byte aligned
    assert mn(r=1025, th=1.0) == -1                                                                     # an argument error goes first
    assert mo(b=0) == mo(r=0) == mo(v=0) == mn(b=0) == mn(r=0) == mn(v=0) == mn(r=0, labels=null) == 0  # nothing to do
    # the workspaces: b * r * ceil(v / 64) words; then, each 16-byte aligned, b * r and b * r * r int32; 0 for what the calls decline
    ob, nb = lib.gspn_mask_overlaps_ws_bytes, lib.gspn_mask_nms_ws_bytes
    up = lambda n: (n + 15) // 16 * 16                                                                  # noqa: E731
    for b, r, v in ((1, 1, 1), (2, 3, 9), (1, 100, 500000), (1, 1024, (1 << 21) + 3), (3, 7, 65), (65535, 1024, 1 << 24)):
        words = (v + 63) // 64
        assert ob(b, r, v) == up(8 * b * r * words)
        assert nb(b, r, v) == up(up(8 * b * r * words) + 4 * b * r) + 4 * b * r * r
    for args in ((-1, 3, 9), (2, -1, 9), (2, 3, -1), (0, 3, 9), (2, 0, 9), (2, 3, 0), (2, 1025, 9), (2, 3, (1 << 24) + 1), (65536, 3, 9)):
        assert ob(*args) == 0 and nb(*args) == 0, args


def test_the_argument_checks_hold_under_the_host_sanitizers(tmp_path):
    """tools/mask_nms_args_check.cpp: the launchers' host-side checks and workspace layouts as a program of their own, built with the
    address and undefined-behaviour sanitizers and run over the decline table -- never loaded into Python"""
    run_args_check("mask_nms_args_check", tmp_path)


# 12 vertices, 6 rows
MASKS = np.array([[1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0],              # A
                  [0, 255, 2, 1, 1, 0, 0, 0, 0, 0, 0, 0],            # B: inter 3 with A, union 5
                  [0, 0, 0, 7, 7, 7, 0, 0, 0, 0, 0, 0],              # C: inter 1 with A, 2 with B (union 5)
                  [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],              # an empty row
                  [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0],              # A again
                  [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9, 9]], np.uint8)   # alone


def test_the_restatement_on_a_hand_written_case():
    sizes, inter = ref.mask_overlaps_ref(MASKS)
    assert sizes.dtype == np.int32 and inter.dtype == np.int32 and sizes.tolist() == [4, 4, 3, 0, 4, 2]
    assert inter.tolist() == [[4, 3, 1, 0, 4, 0], [3, 4, 2, 0, 3, 0], [1, 2, 3, 0, 1, 0], [0] * 6, [4, 3, 1, 0, 4, 0], [0, 0, 0, 0, 0, 2]]
    assert np.array_equal(inter, inter.T) and np.array_equal(np.diagonal(inter), sizes)                 # symmetric, the sizes on the diagonal
    out, keep, points = ref.mask_nms_ref(MASKS, iou_th=0.5)          # A-B 0.6: B goes; B-C 0.4, A-C 1/6: C stays either way; A again goes
    assert out.dtype == np.uint8 and keep.dtype == np.uint8 and points.dtype == np.int32
    assert keep.tolist() == [1, 0, 1, 1, 0, 1] and points.tolist() == [4, 0, 3, 0, 0, 2]
    assert np.array_equal(out, (MASKS != 0) * np.array(keep, bool)[:, None])
    keep = ref.mask_nms_ref(MASKS, iou_th=0.39)[1]                    # the greedy chain: B alone would suppress C (0.4), but B is gone
    assert keep.tolist() == [1, 0, 1, 1, 0, 1] and ref.mask_nms_ref(MASKS[1:], iou_th=0.39)[1].tolist() == [1, 0, 1, 0, 1]
    assert 0.6 * 5.0 == 3.0 and ref.mask_nms_ref(MASKS, iou_th=0.6)[1].tolist() == [1, 1, 1, 1, 0, 1]   # 0.6 * 5 rounds to 3 in doubles: at the threshold
    assert ref.mask_nms_ref(MASKS, iou_th=0.75)[1].tolist() == [1, 1, 1, 1, 0, 1]
    assert ref.mask_nms_ref(MASKS[[1, 2]], iou_th=0.4)[1].tolist() == [1, int(not 2.0 > 0.4 * 5.0)]         # the compare is the doubles', whatever it says
    assert ref.mask_nms_ref(MASKS, iou_th=0.0)[1].tolist() == [1, 0, 0, 1, 0, 1]                        # one shared vertex; the empty row stays
    # an IoU exactly at the threshold does not suppress: inter 2, union 4
    pair = np.array([[1, 1, 1, 0], [0, 1, 1, 1]], np.uint8)
    assert ref.mask_nms_ref(pair, iou_th=0.5)[1].tolist() == [1, 1] and ref.mask_nms_ref(pair, iou_th=0.49)[1].tolist() == [1, 0]
    # labels: only rows of equal label suppress each other
    assert ref.mask_nms_ref(MASKS, labels=[1, 2, 2, 2, 1, 1], iou_th=0.39)[1].tolist() == [1, 1, 0, 1, 0, 1]
    # the count: rows at or beyond it are not kept and not touched apart from the normalisation
    out, keep, points = ref.mask_nms_ref(MASKS, count=4, iou_th=0.5)
    assert keep.tolist() == [1, 0, 1, 1, 0, 0] and points.tolist() == [4, 0, 3, 0, 4, 2] and out[4].tolist() == [1, 1, 1, 1] + [0] * 8
    assert ref.mask_nms_ref(MASKS, count=-2, iou_th=0.5)[1].tolist() == [0] * 6 and ref.mask_nms_ref(MASKS, count=99, iou_th=0.5)[1].tolist() == [1, 0, 1, 1, 0, 1]
    both = ref.mask_nms_batch_ref(np.stack([MASKS, MASKS]), [6, 4], None, 0.5)
    assert both[1].tolist() == [[1, 0, 1, 1, 0, 1], [1, 0, 1, 1, 0, 0]]


def test_the_restatement_s_walk_is_the_definition():
    """the vectorised walk of greedy_ref against the rule written as two loops, on random symmetric tables"""
    rng = np.random.default_rng(0)
    for _ in range(60):
        r, v = int(rng.integers(1, 12)), int(rng.integers(1, 40))
        masks = (rng.random((r, v)) < rng.choice([0.2, 0.7])).astype(np.uint8)
        sizes, inter = ref.mask_overlaps_ref(masks)
        labels = rng.integers(0, 2, size=r) if rng.random() < 0.5 else None
        count = int(rng.integers(-1, r + 2))
        for th in (0.0, 0.25, 1.0 / 3.0, 0.5, 0.999):
            supp, live = ref.greedy_ref(sizes, inter, count, labels, th)
            want = np.zeros(r, bool)
            for k in range(live):
                for i in range(k):
                    if not want[i] and (labels is None or labels[i] == labels[k]):
                        n = int(inter[i, k])
                        if float(n) > th * float(int(sizes[i]) + int(sizes[k]) - n):
                            want[k] = True
            assert live == min(max(count, 0), r) and np.array_equal(supp, want)


def test_the_wrappers_raise_before_anything_runs(monkeypatch):
    from gspn_amd import _lib, mask_nms as M
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    masks = torch.zeros(3, 12, dtype=torch.uint8)
    for bad in (masks[0], masks[None, None], masks.int(), masks[:0], masks[:, :0], torch.zeros(0, 3, 12, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            M.mask_overlaps(bad)
        with pytest.raises(ValueError):
            M.mask_nms(bad, iou_th=0.5)
    with pytest.raises(TypeError):
        M.mask_nms(masks.numpy(), iou_th=0.5)
    with pytest.raises(TypeError):
        M.mask_nms(masks)                                             # the threshold has no default
    for th in (float("nan"), -0.5, 1.0, 7.0):
        with pytest.raises(ValueError, match=r"iou_th must lie in \[0, 1\)"):
            M.mask_nms(masks, iou_th=th)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)        # noqa: E731
    for kw in (dict(count=i32(1)), dict(count=torch.zeros((), dtype=torch.int64)), dict(labels=i32(2)), dict(labels=i32(1, 3)),
               dict(labels=torch.zeros(3)), dict(out=torch.zeros(3, 11, dtype=torch.uint8)), dict(out=torch.zeros(3, 12)),
               dict(out=torch.zeros(1, 3, 12, dtype=torch.uint8)), dict(ws=torch.zeros(4096)), dict(ws=torch.zeros(8, 8, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            M.mask_nms(masks, iou_th=0.5, **kw)
    for kw in (dict(count=i32()), dict(count=i32(3)), dict(labels=i32(3)), dict(labels=i32(2, 4))):
        with pytest.raises(ValueError):
            M.mask_nms(masks[None].expand(2, 3, 12), iou_th=0.5, **kw)
    with pytest.raises(ValueError):
        M.mask_overlaps(masks, ws=torch.zeros(4096))
    for bad in (torch.zeros(1025, 1, dtype=torch.uint8), torch.zeros(1, (1 << 24) + 1, dtype=torch.uint8)):
        with pytest.raises(NotImplementedError):
            M.mask_overlaps(bad)
        with pytest.raises(NotImplementedError):
            M.mask_nms(bad, iou_th=0.5)
    # tensors that are not on a device are refused: there is no CPU fallback
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        M.mask_overlaps(masks)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        M.mask_nms(masks, i32(), i32(3), iou_th=0.5)


def test_the_drivers_check_their_threshold_before_anything_runs(monkeypatch):
    from gspn_amd import _lib, lift, predict
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    b, n, r, p, c, sd, v = 1, 20, 3, 8, 5, 6, 30
    ep = {"detections": torch.zeros(b, r, 8), "rpointnet_mask_selected": torch.zeros(b, r, p),
          "pc_coord_cropped_final_unnormalized": torch.zeros(b, r, p, 3), "pc_seed": torch.zeros(b, sd, 3), "fb_prob": torch.zeros(b, sd, 2),
          "sem_class_logits": torch.zeros(b, n, c)}
    for th in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"mask_nms_th must lie in \[0, 1\)"):
            lift.scan_predictions(ep, 0, torch.zeros(v, 3), pc=torch.zeros(b, n, 3), label_map=list(range(c)), mask_nms_th=th)
        with pytest.raises(ValueError, match=r"mask_nms_th must lie in \[0, 1\)"):
            predict.scene_predictions(ep, torch.zeros(b, n, 3), label_map=list(range(c)), mask_nms_th=th)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        lift.scan_predictions(ep, 0, torch.zeros(v, 3), pc=torch.zeros(b, n, 3), label_map=list(range(c)), mask_nms_th=0.5)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        predict.scene_predictions(ep, torch.zeros(b, n, 3), label_map=list(range(c)), mask_nms_th=0.5)


def test_the_tool_s_mask_nms_flag():
    spec = importlib.util.spec_from_file_location("tools_test", os.path.join(ROOT, "tools", "test.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.parse(["--synthetic", "2"]).mask_nms is None
    assert tool.parse(["--synthetic", "2", "--synthetic_vertices", "20000", "--mask_nms", "0.3"]).mask_nms == 0.3
    with pytest.raises(SystemExit, match="--mask_nms goes with the vertex modes"):
        tool.main(["--synthetic", "2", "--mask_nms", "0.5"])
    for th in ("1.0", "-0.1", "nan"):
        with pytest.raises(SystemExit, match="--mask_nms must lie in"):
            tool.main(["--synthetic", "2", "--synthetic_vertices", "20000", "--mask_nms", th])
