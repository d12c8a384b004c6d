"""CPU tests of gspn_amd/dataset.py: ABI 18 and its two symbols, remap_labels on CPU tensors against the numpy restatement
(tests/dataset_ref.py), the shape and dtype rules, and the generator of the padding draws in its three restatements."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import dataset_ref as DR
from tests import roi_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_18_and_the_segment_symbols():
    from gspn_amd import _lib, build
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    # the three agree, on the version that brought these symbols or a later one
    assert int(re.search(r"#define GSPN_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gspn_abi_version() >= 18
    assert re.search(r"^ \*\s+18: gspn_fps_segments", text, flags=re.M)           # the history line of the header comment
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, table in (("gspn_fps_segments", _lib.SIGNATURES), ("gspn_fps_segments_ws_bytes", _lib.SPECIAL)):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        declared = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        bound = table[name] if table is _lib.SIGNATURES else table[name][0]
        assert len(declared.split(",")) == len(bound) == {"gspn_fps_segments": 13, "gspn_fps_segments_ws_bytes": 3}[name]
    assert _lib.SPECIAL["gspn_fps_segments_ws_bytes"][1] is ctypes.c_long
    # host-side argument rules (no launch): the sizes of the neighbouring launchers
    assert lib.gspn_fps_segments_ws_bytes(2, 18000, 40) >= 0
    assert lib.gspn_fps_segments_ws_bytes(2, 32769, 40) == -2 and lib.gspn_fps_segments_ws_bytes(-1, 100, 4) == -1
    from gspn_amd.build import POLICY_SOURCES
    assert "sampling_segments.hip" in POLICY_SOURCES


def raw_scan(seed, n=3000, ngroup=12):
    """raw labels of one scan: group ids in [-1, ngroup) with id 3 absent, semantic labels in [-2, 45); group 5 is half class 0 (after the
    table) and half class 1, so its mean is exactly 0.5, and group 6 is three quarters class 1 (mean 0.75)"""
    rng = np.random.default_rng(seed)
    group = rng.integers(-1, ngroup, n)
    group[group == 3] = 4
    seg = rng.integers(-2, 45, n)
    # most groups carry one valid raw class each, so that their mean is far from 0
    for gid, cls in ((0, 3), (1, 39), (2, 1), (4, 24), (7, 5), (8, 0), (9, 12)):
        seg[group == gid] = cls
    for gid, every in ((5, 2), (6, 4)):
        members = np.nonzero(group == gid)[0]
        members = members[: len(members) // every * every]
        group[np.setdiff1d(np.nonzero(group == gid)[0], members)] = -1
        seg[members] = 3                                            # raw 3 -> class 1
        seg[members[::every]] = 2                                   # raw 2 -> class 0
    return group, seg


def test_remap_labels_equals_the_restatement_on_cpu_tensors():
    from gspn_amd import dataset
    scans = [raw_scan(1), raw_scan(2)]
    group, seg = np.stack([g for g, _ in scans]), np.stack([s for _, s in scans])
    for gid, mean in ((5, 0.5), (6, 0.75)):
        table = np.zeros(40, np.int64)
        table[DR.VALID_CLASS_IDS] = np.arange(1, 19)
        assert np.mean(table[seg[0][group[0] == gid]]) == mean
    assert (group == 3).sum() == 0 and (group == -1).any() and (seg >= 40).any() and (seg < 0).any()
    for dtype in (torch.int64, torch.int32):
        got = dataset.remap_labels(torch.from_numpy(group).to(dtype), torch.from_numpy(seg).to(dtype), 12)
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.int64 and got[2].dtype == torch.int32
        for s in range(2):
            want_group, want_seg, want_n = DR.remap_labels(group[s], seg[s])
            assert np.array_equal(got[0][s].numpy(), want_group) and np.array_equal(got[1][s].numpy(), want_seg)
            assert int(got[2][s]) == want_n
    # group 5 (mean exactly 0.5 rounds to 0), the absent id 3, group 2 (raw class 1 is not a valid class) and group 8 are not instances
    want_group, _, want_n = DR.remap_labels(group[0], seg[0])
    for gid in (5, 2, 8):
        assert (want_group[group[0] == gid] == 0).all()
    assert (want_group[group[0] == 6] > 0).all() and (want_group[group[0] == -1] == 0).all()
    for rank, gid in enumerate((0, 1, 4), start=1):                 # ascending original id: 0 -> 1, 1 -> 2, 4 -> 3 (2 and 3 are skipped)
        assert (want_group[group[0] == gid] == rank).all()
    # a larger static bound changes nothing
    wide = dataset.remap_labels(torch.from_numpy(group), torch.from_numpy(seg), 20)
    narrow = dataset.remap_labels(torch.from_numpy(group), torch.from_numpy(seg), 12)
    assert all(torch.equal(a, b) for a, b in zip(wide, narrow))


def test_shape_and_dtype_rules_raise_value_error():
    from gspn_amd import dataset
    pc, label = torch.zeros(2, 64, 3), torch.zeros(2, 64, dtype=torch.int64)
    with pytest.raises(ValueError):
        dataset.remap_labels(label.float(), label, 4)
    with pytest.raises(ValueError):
        dataset.remap_labels(label, label[:, :32], 4)
    with pytest.raises(ValueError):
        dataset.remap_labels(label, label, 0)
    with pytest.raises(ValueError):
        dataset.fps_segments(pc.double(), label, 4, 16)
    with pytest.raises(ValueError):
        dataset.fps_segments(pc[:, :, :2], label, 4, 16)
    with pytest.raises(ValueError):
        dataset.fps_segments(pc, label.float(), 4, 16)
    with pytest.raises(ValueError):
        dataset.fps_segments(pc, label[:, :32], 4, 16)
    with pytest.raises(ValueError):
        dataset.fps_segments(pc, label, 4, 0)
    with pytest.raises(ValueError):
        dataset.resample_scene(pc, pc[:, :32], label, label, 128)
    with pytest.raises(ValueError):
        dataset.resample_scene(pc, pc, label, label.float(), 128)
    with pytest.raises(ValueError):
        dataset.augment_and_box(pc[:, :, :2], torch.zeros(2, 4, 8, 3), 4)


def test_padding_draws_agree_across_the_restatements():
    from gspn_amd import dataset
    assert dataset.SCENE_STREAM == DR.SCENE_STREAM
    for seed in (0, 7, -3, (1 << 62) + 12345):
        for a, count in ((4, 10), (DR.SCENE_STREAM, 1000), (1, 1)):
            got = dataset._rand_rank(torch.tensor([seed], dtype=torch.int64), 3, a, 54, count).numpy()
            for scene in range(3):
                want = RR.rank_of(RR.rand32(seed, scene, a, np.arange(54)), count)
                assert np.array_equal(DR.padding_draws(seed, scene, a, 54, count), want)
                assert np.array_equal(got[scene], want) and want.min() >= 0 and want.max() < count


def test_package_exports_the_dataset_functions():
    import gspn_amd
    from gspn_amd import dataset
    assert gspn_amd.dataset is dataset
    for name in ("fps_segments", "instance_point_sets", "resample_scene", "remap_labels", "augment_and_box"):
        assert getattr(gspn_amd, name) is getattr(dataset, name) and name in gspn_amd.__all__
