"""CPU tests of segment voting (gspn_amd/segments.py): the four symbols in the header, the library and the binding with the
ABI still 21; the host-side declines of the entry points, which launch nothing; the numpy restatement (tests/segments_ref.py) on a
hand-written case with its expected output written out; the wrappers' guards, which raise before the library is touched;
compact_segments, synth.scan_segments, data_prep.read_segments and the flag errors of tools/test.py."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import segments_ref as ref
from tests.args_check import run_args_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_segment_symbols_are_declared_exported_and_bound_at_abi_21():
    from gspn_amd import _lib, build, segments
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    assert "#define GSPN_ABI_VERSION 21" in text and int(lib.gspn_abi_version()) == 21 == _lib.ABI_VERSION
    assert "Additive at 21: gspn_segment_vote, gspn_segment_label_vote (+ their _ws_bytes)" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("gspn_segment_vote", 10), ("gspn_segment_label_vote", 8)):
        declared = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        assert len(declared) == len(_lib.SIGNATURES[name]) == nargs and hasattr(raw, name)
    assert _lib.SIGNATURES["gspn_segment_vote"][5] is ctypes.c_double                                   # vote_th is a double across the ABI
    assert re.search(r"\blong gspn_segment_vote_ws_bytes\s*\(int r, int v, int s\)", code)
    assert re.search(r"\blong gspn_segment_label_vote_ws_bytes\s*\(int v, int s, int c\)", code)
    three = ([ctypes.c_int] * 3, ctypes.c_long)
    assert _lib.SPECIAL["gspn_segment_vote_ws_bytes"] == three and _lib.SPECIAL["gspn_segment_label_vote_ws_bytes"] == three
    assert hasattr(raw, "gspn_segment_vote_ws_bytes") and hasattr(raw, "gspn_segment_label_vote_ws_bytes")
    limit = lambda name: int(re.search(r"#define %s \(1 << (\d+)\)" % name, text).group(1))            # noqa: E731
    assert segments.SEGMENT_MAX_V == 1 << limit("GSPN_SEGMENT_VOTE_MAX_V") == 1 << 24
    assert segments.SEGMENT_MAX_S == 1 << limit("GSPN_SEGMENT_VOTE_MAX_S") == 1 << 24
    assert segments.SEGMENT_MAX_COUNTERS == 1 << limit("GSPN_SEGMENT_VOTE_MAX_COUNTERS") == 1 << 28
    assert "segments.hip" not in build.POLICY_SOURCES
    # host-side declines, nothing launched
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(24)
    sv = lambda r=3, v=9, s=4, th=0.5, p=(one,) * 5: lib.gspn_segment_vote(r, v, s, p[0], p[1], th, p[2], p[3], p[4], null)      # noqa: E731
    sl = lambda v=9, s=4, c=5, p=(one,) * 4: lib.gspn_segment_label_vote(v, s, c, p[0], p[1], p[2], p[3], null)                  # noqa: E731
    assert sv(r=-1) == sv(v=-1) == sv(s=-1) == -1
    assert all(sv(p=tuple(null if i == k else one for i in range(5))) == -1 for k in range(5))
    assert all(sv(th=th) == -1 for th in (float("nan"), -1e-9, 1.0, 2.0, float("inf"), float("-inf")))
    assert sv(v=(1 << 24) + 1) == sv(r=65536) == sv(s=(1 << 24) + 1) == sv(r=100, s=(1 << 28) // 101 + 1) == -2
    assert sv(p=(one, one, odd, one, one)) == -2                                                        # a ws that is not 16-byte aligned
    assert sv(r=0) == sv(v=0) == 0                                                                      # nothing to do
    assert sl(v=-1) == sl(s=-1) == sl(c=0) == sl(c=-1) == -1
    assert all(sl(p=tuple(null if i == k else one for i in range(4))) == -1 for k in range(4))
    assert sl(v=(1 << 24) + 1) == sl(s=(1 << 24) + 1) == sl(s=1 << 20, c=257) == sl(p=(one, one, odd, one)) == -2
    assert sl(v=0) == 0
    # the workspaces: (r + 1) * s counters, 16-byte aligned decision words; s * c counters and s winners; 0 for what the calls decline
    wsb, wlb = lib.gspn_segment_vote_ws_bytes, lib.gspn_segment_label_vote_ws_bytes
    for r, v, s in ((1, 1, 1), (3, 9, 4), (100, 150000, 20000), (7, 33, 65), (1024, (1 << 21) + 3, 32768), (100, 5, (1 << 28) // 101)):
        assert wsb(r, v, s) == (4 * (r + 1) * s + 15) // 16 * 16 + 8 * r * ((s + 63) // 64)
    for v, s, c in ((1, 1, 1), (9, 4, 5), (500000, 20000, 19), (5, 1 << 20, 256)):
        assert wlb(v, s, c) == 4 * s * c + 4 * s
    for args in ((-1, 9, 4), (3, -1, 4), (3, 9, -1), (0, 9, 4), (3, 0, 4), (3, (1 << 24) + 1, 4), (65536, 9, 4), (3, 9, (1 << 24) + 1),
                 (100, 9, (1 << 28) // 101 + 1)):
        assert wsb(*args) == 0, args
    for args in ((-1, 4, 5), (9, -1, 5), (9, 4, 0), (0, 4, 5), ((1 << 24) + 1, 4, 5), (9, (1 << 24) + 1, 5), (9, 1 << 20, 257)):
        assert wlb(*args) == 0, args


def test_the_argument_checks_hold_under_the_host_sanitizers(tmp_path):
    """tools/segments_args_check.cpp: the launchers' host-side checks and workspace layouts as a program of their own, built with the
    address and undefined-behaviour sanitizers and run over the decline table -- never loaded into Python"""
    run_args_check("segments_args_check", tmp_path)


# 12 vertices, 4 segments, 3 rows: segment 0 has four vertices, 1 two, 2 three, 3 one; vertex 9 is unsegmented (-1), vertex 10 carries an id
# equal to S
SEG = np.array([0, 0, 0, 0, 1, 1, 2, 2, 2, -1, 4, 3])
MASKS = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],              # an all-zero row
                  [1, 255, 0, 0, 2, 2, 1, 0, 0, 255, 0, 1],          # segment 0 exactly half set; the unsegmented vertex holds 255
                  [1, 1, 1, 0, 0, 7, 0, 9, 9, 0, 3, 0]], np.uint8)   # segment 1 exactly half set; the vertex with id S holds 3
LABELS = np.array([2, 2, 1, 1, 0, 4, 3, 5, -1, 1, 2, 9])             # 5 classes: a 2-2 tie, a 1-1 tie, one voter among three, nobody in segment 3


def test_the_restatement_on_a_hand_written_case():
    out, points = ref.segment_vote_ref(MASKS, SEG, 4)
    assert out.dtype == np.uint8 and points.dtype == np.int32
    assert out.tolist() == [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                            [0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 1],     # half of segment 0 is not a majority; 1 of 3 is not; 255 becomes 1
                            [1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0]]     # 3 of 4 and 2 of 3 are; half of segment 1 is not; 3 becomes 1
    assert points.tolist() == [0, 4, 8]
    out, points = ref.segment_vote_ref(MASKS, SEG, 4, 0.0)             # at 0 any vote sets the segment
    assert out.tolist() == [[0] * 12, [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1], [1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0]] and points.tolist() == [0, 11, 10]
    out, points = ref.segment_vote_ref(MASKS, SEG, 4, 0.7)             # 3 of 4 still is, 2 of 3 no longer
    assert out[2].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0] and points.tolist() == [0, 4, 5]
    none = ref.segment_vote_ref(MASKS, np.full(12, -1), 0)             # no segmented vertex at all: the normalised input
    assert np.array_equal(none[0], (MASKS != 0).astype(np.uint8)) and none[1].tolist() == [0, 7, 7]
    single = ref.segment_vote_ref(MASKS, np.arange(12)[::-1], 12)      # singleton segments: the same
    assert np.array_equal(single[0], none[0])
    labels = ref.segment_label_vote_ref(LABELS, SEG, 4, 5)
    assert labels.dtype == np.int32 and labels.tolist() == [1, 1, 1, 1, 0, 0, 3, 3, 3, 1, 2, 9]
    rng = np.random.default_rng(0)                                    # the loop-free form used for the larger GPU cases says the same
    for _ in range(40):
        r, v, s = int(rng.integers(1, 5)), int(rng.integers(1, 300)), int(rng.integers(0, 9))
        masks = (rng.integers(0, 3, size=(r, v)) * (rng.random((r, v)) < 0.5)).astype(np.uint8)
        seg = rng.integers(-2, s + 2, size=v)
        for th in (0.0, 0.25, 1.0 / 3.0, 0.5, 0.999):
            a, b = ref.segment_vote_ref(masks, seg, s, th), ref.fast_segment_vote_ref(masks, seg, s, th)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_wrappers_raise_before_anything_runs(monkeypatch):
    from gspn_amd import _lib, segments
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    masks, seg, labels = torch.zeros(3, 12, dtype=torch.uint8), torch.zeros(12, dtype=torch.int32), torch.zeros(12, dtype=torch.int32)
    for bad in ((masks[0], seg), (masks, seg[:11]), (masks, seg[None]), (masks.int(), seg), (masks, seg.long()), (masks[:0], seg),
                (masks[:, :0], seg[:0])):
        with pytest.raises(ValueError):
            segments.segment_vote(*bad, 4)
    with pytest.raises(TypeError):
        segments.segment_vote(masks.numpy(), seg, 4)
    with pytest.raises(ValueError, match="num_segments"):
        segments.segment_vote(masks, seg, -1)
    for th in (float("nan"), -0.5, 1.0, 7.0):
        with pytest.raises(ValueError, match=r"vote_th must lie in \[0, 1\)"):
            segments.segment_vote(masks, seg, 4, th)
    for out in (torch.zeros(3, 11, dtype=torch.uint8), torch.zeros(3, 12), torch.zeros(36, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            segments.segment_vote(masks, seg, 4, out=out)
    for ws in (torch.zeros(4096), torch.zeros(8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            segments.segment_vote(masks, seg, 4, ws=ws)
        with pytest.raises(ValueError):
            segments.segment_label_vote(labels, seg, 4, 19, ws=ws)
    big = (1 << 24) + 1
    for bad in ((torch.zeros(1, big, dtype=torch.uint8), torch.zeros(big, dtype=torch.int32), 4), (torch.zeros(65536, 1, dtype=torch.uint8), seg[:1], 4),
                (masks, seg, big), (torch.zeros(100, 12, dtype=torch.uint8), seg, (1 << 28) // 101 + 1)):
        with pytest.raises(NotImplementedError):
            segments.segment_vote(*bad)
    for bad in ((labels[None], seg), (labels, seg[:5]), (labels.long(), seg), (labels, seg.short()), (labels[:0], seg[:0])):
        with pytest.raises(ValueError):
            segments.segment_label_vote(*bad, 4, 19)
    with pytest.raises(ValueError, match="num_segments"):
        segments.segment_label_vote(labels, seg, -2, 19)
    with pytest.raises(ValueError, match="num_classes must be positive"):
        segments.segment_label_vote(labels, seg, 4, 0)
    for bad in ((torch.zeros(big, dtype=torch.int32), torch.zeros(big, dtype=torch.int32), 4, 19), (labels, seg, big, 19), (labels, seg, 1 << 20, 257)):
        with pytest.raises(NotImplementedError):
            segments.segment_label_vote(*bad)
    # tensors that are not on a device are refused: there is no CPU fallback
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        segments.segment_vote(masks, seg, 4)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        segments.segment_label_vote(labels, seg, 4, 19)


def test_scan_predictions_checks_its_segments_before_anything_runs(monkeypatch):
    from gspn_amd import _lib, lift
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    b, n, r, p, c, sd, v = 1, 20, 3, 8, 5, 6, 30
    ep = {"detections": torch.zeros(b, r, 8), "rpointnet_mask_selected": torch.zeros(b, r, p),
          "pc_coord_cropped_final_unnormalized": torch.zeros(b, r, p, 3), "pc_seed": torch.zeros(b, sd, 3), "fb_prob": torch.zeros(b, sd, 2),
          "sem_class_logits": torch.zeros(b, n, c)}
    call = lambda **kw: lift.scan_predictions(ep, 0, torch.zeros(v, 3), pc=torch.zeros(b, n, 3), label_map=list(range(c)), **kw)      # noqa: E731
    seg = torch.zeros(v, dtype=torch.int32)
    for kw in (dict(num_segments=4), dict(segments=seg), dict(segments=seg, num_segments=-1), dict(segments=seg[:7], num_segments=4),
               dict(segments=seg.long(), num_segments=4), dict(segments=seg, num_segments=4, vote_th=1.0),
               dict(segments=seg, num_segments=4, vote_th=float("nan"))):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(NotImplementedError):
        call(segments=seg, num_segments=(1 << 24) + 1)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        call(segments=seg, num_segments=4)


def test_compact_segments_numbers_the_ids_in_ascending_order():
    from gspn_amd.segments import compact_segments
    raw = torch.tensor([40, -7, 40, 3, (1 << 26) - 1, 3, -1, 1000, 0], dtype=torch.int64)
    seg, s = compact_segments(raw)
    assert s == 5 and seg.dtype == torch.int32 and seg.tolist() == [2, -1, 2, 1, 4, 1, -1, 3, 0]
    seg, s = compact_segments(torch.tensor([7, 7, 900], dtype=torch.int32))       # no negative id: nothing is shifted
    assert s == 2 and seg.tolist() == [0, 0, 1]
    seg, s = compact_segments(torch.tensor([-3, -1], dtype=torch.int64))
    assert s == 0 and seg.tolist() == [-1, -1]
    seg, s = compact_segments(torch.zeros(0, dtype=torch.int64))
    assert s == 0 and seg.shape == (0,)
    rng = np.random.default_rng(1)
    ids = rng.choice(1 << 26, size=300, replace=False)[rng.integers(0, 300, size=5000)]
    ids[rng.random(5000) < 0.1] = -rng.integers(1, 50)
    seg, s = compact_segments(torch.from_numpy(ids))
    values = np.unique(ids[ids >= 0])
    assert s == values.size and np.array_equal(seg.numpy(), np.where(ids >= 0, np.searchsorted(values, ids), -1))
    with pytest.raises(ValueError):
        compact_segments(torch.zeros(3, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        compact_segments(torch.zeros(3))
    with pytest.raises(TypeError):
        compact_segments([1, 2, 3])


def test_scan_segments_nests_in_the_instances_and_is_seeded():
    from gspn_amd import synth
    rng = np.random.default_rng(2)
    v = 3000
    xyz = (rng.random((v, 3), dtype=np.float32) * np.array([8, 6, 3], np.float32)).astype(np.float32)
    group = rng.integers(0, 7, size=v).astype(np.int32)
    sem = (group % 3).astype(np.int32)
    sem[group == 6] = rng.integers(0, 3, size=int((group == 6).sum()))                                  # one group that spans classes
    ids = synth.scan_segments(xyz, sem, group, 0.5, 4)
    assert ids.shape == (v,) and ids.dtype == np.int64 and ids.min() >= 0
    values, inverse = np.unique(ids, return_inverse=True)
    cube = np.floor(xyz.astype(np.float64) / 0.5).astype(np.int64)
    for g in range(values.size):                                      # one (class, group) pair and one cube per segment
        at = np.nonzero(inverse == g)[0]
        assert np.unique(sem[at]).size == 1 and np.unique(group[at]).size == 1 and np.unique(cube[at], axis=0).shape[0] == 1
    keys = np.unique(np.concatenate((sem[:, None], group[:, None], cube), 1), axis=0)
    assert values.size == keys.shape[0]                               # and no two segments share them
    assert values.max() > values.size - 1                             # gaps: compaction has something to do
    first = ids[np.sort(np.unique(inverse, return_index=True)[1])]
    assert not np.array_equal(first, np.sort(first))                  # and the ids do not ascend with the segments
    assert np.array_equal(ids, synth.scan_segments(xyz, sem, group, 0.5, 4))
    assert not np.array_equal(ids, synth.scan_segments(xyz, sem, group, 0.5, 5))
    assert np.unique(synth.scan_segments(xyz, sem, group, 100.0, 4)).size == np.unique(np.stack((sem, group), 1), axis=0).shape[0]
    for bad in (dict(cell=0.0), dict(cell=-1.0), dict(seg_label=sem[:5]), dict(group_label=group[:5]), dict(xyz=xyz[:, :2])):
        args = dict(xyz=xyz, seg_label=sem, group_label=group, cell=0.5, seed=0)
        args.update(bad)
        with pytest.raises(ValueError):
            synth.scan_segments(**args)


def test_read_segments_reads_the_seg_indices(tmp_path):
    from gspn_amd import data_prep
    scan = "scene0000_00"
    os.makedirs(tmp_path / scan)
    ids = [5, 5, 70001, 0, (1 << 26) - 1, 5, 12]
    with open(tmp_path / scan / (scan + "_vh_clean_2.0.010000.segs.json"), "w") as f:
        json.dump({"params": {"kThresh": "0.0001"}, "sceneId": scan, "segIndices": ids}, f)
    got = data_prep.read_segments(str(tmp_path), scan)
    assert got.dtype == np.int64 and got.shape == (7,) and got.tolist() == ids
    assert "read_segments" in data_prep.__all__
    with pytest.raises(FileNotFoundError):
        data_prep.read_segments(str(tmp_path), "scene0001_00")


def test_the_tool_s_segment_flags():
    spec = importlib.util.spec_from_file_location("tools_test", os.path.join(ROOT, "tools", "test.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse(["--synthetic", "2"])
    assert a.segments is False and a.vote_th == 0.5
    assert tool.parse(["--synthetic", "2", "--segments", "--vote_th", "0.3"]).vote_th == 0.3
    with pytest.raises(SystemExit, match="--segments goes with"):
        tool.main(["--synthetic", "2", "--segments"])
    with pytest.raises(SystemExit, match="--segments goes with"):
        tool.main(["--cache", "val.pt", "--list", "val.txt", "--mesh_path", "mesh", "--segments"])       # the segs.json lie under --label_path
    for th in ("1.0", "-0.1", "nan"):
        with pytest.raises(SystemExit, match="--vote_th must lie in"):
            tool.main(["--synthetic", "2", "--synthetic_vertices", "20000", "--segments", "--vote_th", th])
    with pytest.raises(SystemExit, match="--segment_cell must be positive"):
        tool.main(["--synthetic", "2", "--synthetic_vertices", "20000", "--segments", "--segment_cell", "0"])
    # the synthetic scans bring their segments only when asked
    cache = {"pc": torch.rand(1, 64, 3), "seg_label": torch.randint(0, 3, (1, 64)), "group_label": torch.randint(0, 4, (1, 64))}
    assert set(tool.synthetic_vertices(cache, 100, 0)(0)) == {"xyz", "seg_label", "group_label"}
    scan = tool.synthetic_vertices(cache, 100, 0, 0.25)(0)
    assert set(scan) == {"xyz", "seg_label", "group_label", "segments"} and scan["segments"].shape == (100,)
