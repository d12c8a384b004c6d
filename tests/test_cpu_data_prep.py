"""CPU tests of gspn_amd/data_prep.py and gspn_amd/io_util.py: the two entry points of csrc/data_prep.hip in the library, the header and the
binding (additive at ABI 21), their host-side argument rules (no launch), the PLY reader on both encodings, the writers' round trip, the label
writer's bytes, the wrappers' errors, the chunk rule of build_cache and the arguments of tools/data_prep.py and tools/make_cache.py."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import data_prep_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_symbols_are_exported_declared_and_bound_additive_at_abi_21():
    from gspn_amd import _lib, build, data_prep
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    assert int(re.search(r"#define GSPN_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gspn_abi_version() == 21
    assert re.search(r"^/\* Additive at 21: gspn_segment_labels \(\+ _ws_bytes\)\.", text, flags=re.M)
    assert re.search(r"^/\* Additive at 20: gspn_instance_overlaps / gspn_instance_match\.", text, flags=re.M)      # the lines above stay
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "gspn_segment_labels") and hasattr(handle, "gspn_segment_labels_ws_bytes")
    declared = [a.strip() for a in re.search(r"\bint gspn_segment_labels\s*\(([^)]*)\)", code).group(1).split(",")]
    bound = _lib.SIGNATURES["gspn_segment_labels"]
    assert len(declared) == len(bound) == 10
    assert [a.startswith("int ") for a in declared] == [a is ctypes.c_int for a in bound]            # n, p, s by value, everything else a pointer
    assert all(("*" in a) == (b is ctypes.c_void_p) for a, b in zip(declared, bound))
    assert re.search(r"\blong gspn_segment_labels_ws_bytes\s*\(\s*int s\s*\)", code)
    assert _lib.SPECIAL["gspn_segment_labels_ws_bytes"] == ([ctypes.c_int], ctypes.c_long)
    for macro, value in (("GSPN_SEGMENT_LABELS_MAX_N", data_prep.SEGMENT_LABELS_MAX_N), ("GSPN_SEGMENT_LABELS_MAX_S", data_prep.SEGMENT_LABELS_MAX_S)):
        shift = int(re.search(r"#define %s \(1 << (\d+)\)" % macro, text).group(1))
        assert 1 << shift == value
    assert data_prep.SEGMENT_LABELS_MAX_N == 1 << 24 and data_prep.SEGMENT_LABELS_MAX_S == 1 << 26
    assert "data_prep.hip" not in build.POLICY_SOURCES
    assert os.path.exists(os.path.join(ROOT, "gspn_amd", "csrc", "data_prep.hip"))


def test_host_side_argument_rules_launch_nothing():
    from gspn_amd import _lib
    lib = _lib.lib()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)                               # never dereferenced: every call below returns before a launch
    for at in range(6):
        ptrs = [p] * 6
        ptrs[at] = null
        assert lib.gspn_segment_labels(10, 3, 5, *ptrs, null) == -1
        assert lib.gspn_segment_labels(10, 0, 5, *ptrs, null) == -1                 # also without a pair
    for extents in ((0, 3, 5), (-4, 3, 5), (10, 3, 0), (10, 3, -1), (10, -1, 5)):
        assert lib.gspn_segment_labels(*extents, *[p] * 6, null) == -1
    assert lib.gspn_segment_labels((1 << 24) + 1, 3, 5, *[p] * 6, null) == -2
    assert lib.gspn_segment_labels(10, 3, (1 << 26) + 1, *[p] * 6, null) == -2
    assert lib.gspn_segment_labels(0, 3, (1 << 26) + 1, *[p] * 6, null) == -1       # an invalid argument before an unsupported one
    assert lib.gspn_segment_labels_ws_bytes(0) == -1 and lib.gspn_segment_labels_ws_bytes(-3) == -1
    assert lib.gspn_segment_labels_ws_bytes((1 << 26) + 1) == -2
    assert lib.gspn_segment_labels_ws_bytes(1) == 12 and lib.gspn_segment_labels_ws_bytes(1 << 26) == 12 << 26


def test_wrappers_raise_before_a_launch(tmp_path):
    from gspn_amd import _lib, data_prep
    seg, ps, po = torch.zeros(10, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), torch.ones(3, dtype=torch.int64)
    with pytest.raises(TypeError):
        data_prep.segment_labels(seg.numpy(), ps, po)
    for bad in ((seg.float(), ps, po), (seg, ps.float(), po), (seg, ps, po.double()), (seg.reshape(2, 5), ps, po), (seg, ps, po[:2]), (seg[:0], ps, po)):
        with pytest.raises(ValueError):
            data_prep.segment_labels(*bad)
    with pytest.raises(_lib.GspnHipError):                                          # well-formed CPU tensors: no CPU path
        data_prep.segment_labels(seg, ps, po)
    xyz = torch.zeros(5, 3)
    for bad in ([(xyz, xyz, xyz[:, 0])], [(xyz.double(), xyz, xyz[:, 0], xyz[:, 0])], [(xyz, xyz[:4], xyz[:, 0], xyz[:, 0])], [(xyz[:, :2], xyz, xyz[:, 0], xyz[:, 0])]):
        with pytest.raises(ValueError):
            data_prep.downsample_scans(bad, 3)
    with pytest.raises(ValueError):
        data_prep.downsample_scans([], 0)
    with pytest.raises(ValueError):
        data_prep.downsample_scans([], 3, batch=0)
    assert data_prep.downsample_scans([], 3) == []
    with pytest.raises(_lib.GspnHipError):
        data_prep.downsample_scans([(xyz, xyz, xyz[:, 0], xyz[:, 0])], 3)
    (tmp_path / "empty.txt").write_text("\n")
    with pytest.raises(ValueError):
        data_prep.build_cache(str(tmp_path), str(tmp_path), str(tmp_path / "empty.txt"), device="cpu")


def test_a_scene_beyond_fps_segments_limit_is_refused_by_name(tmp_path):
    from gspn_amd import data_prep, io_util
    n = data_prep.FPS_SEGMENTS_MAX_N + 1
    io_util.write_color_ply(np.zeros((n, 6), np.float32), str(tmp_path / "big.ply"), text=False)
    for kind in ("sem_", "group_"):
        io_util.write_label_txt(np.zeros(n, np.int64), str(tmp_path / (kind + "big.txt")))
    (tmp_path / "list.txt").write_text("big\n")
    with pytest.raises(ValueError, match="fps_segments.*32768"):
        data_prep.build_cache(str(tmp_path), str(tmp_path), str(tmp_path / "list.txt"), device="cpu")


def test_cache_chunks_follow_the_documented_rule():
    from gspn_amd.data_prep import cache_chunks, flatten_seg_groups
    assert cache_chunks([30000, 30000, 900, 30000, 900, 30000], 2) == [[0, 1], [2, 4], [3, 5]]
    assert cache_chunks([5, 5, 5], 8) == [[0, 1, 2]] and cache_chunks([5, 6, 5], 1) == [[0], [1], [2]]
    groups = [{"objectId": 4, "segments": [9, 2]}, {"objectId": 0, "segments": []}, {"objectId": 1, "segments": [2]}]
    assert flatten_seg_groups(groups) == ([9, 2, 2], [4, 4, 1]) == PR.pairs_of(groups)


def test_lazy_names_of_the_package():
    import gspn_amd
    from gspn_amd import data_prep, io_util
    assert gspn_amd.data_prep is data_prep and gspn_amd.io_util is io_util
    for name in ("segment_labels", "collect_label", "downsample_scans", "prepare_scans", "build_cache"):
        assert getattr(gspn_amd, name) is getattr(data_prep, name) and name in gspn_amd.__all__
    assert gspn_amd.remap_labels is gspn_amd.dataset.remap_labels
    assert not hasattr(io_util, "toRed")                                            # the termcolor helpers are not provided


def test_restated_loop_on_a_worked_case():
    seg = [5, 5, 7, 9, 11, 7]
    groups = [{"objectId": 3, "segments": [5, 7]}, {"objectId": 8, "segments": [7, 7, 13]}, {"objectId": 2, "segments": []}]
    label, errors = PR.collect_label_loop(seg, groups)
    assert label.tolist() == [3, 3, 8, -1, -1, 8] and errors == 2                  # 7 by a second group, then again inside it; 13 has no vertex


# ---- io_util -----------------------------------------------------------------------------------------------------------------------------

def cloud(n=37, seed=3):
    rng = np.random.default_rng(seed)
    xyz = (rng.standard_normal((n, 3)) * 5).astype(np.float32)
    xyz[0] = (np.float32(1) / np.float32(3), np.float32(1e-7), np.float32(-0.0))
    xyz[1] = (np.float32(16777217.0), np.float32(-1e30), np.float32(1.17549435e-38))
    xyz[2] = (np.float32(1e-45), np.float32(3.4028235e38), np.float32(0.1))        # a denormal, the largest float32
    color = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    color[0], color[1] = (0, 255, 128), (255, 0, 1)
    return xyz, color, rng.integers(0, 41, n)


def write_ascii_ply(path, xyz, color, label):
    """the same cloud as ASCII, float text by repr of the float32 (shortest digits), comments in the header, a face element behind"""
    lines = ["ply", "comment first", "format ascii 1.0", "element vertex %d" % len(xyz), "property float32 x", "property float y", "property float z",
             "comment inside", "property uint8 red", "property uchar green", "property uchar blue", "property uchar alpha", "property uint16 label",
             "element face 1", "property list uchar int vertex_indices", "end_header"]
    for p, c, l in zip(xyz, color, label):
        lines.append(" ".join([str(v) for v in p] + [str(int(v)) for v in c] + ["255", str(int(l))]))
    lines.append("3 0 1 2")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_binary_and_ascii_files_read_equal_and_skip_alpha_and_faces(tmp_path):
    from gspn_amd import io_util
    xyz, color, label = cloud()
    binary, text = str(tmp_path / "b.ply"), str(tmp_path / "a.ply")
    PR.write_binary_ply(binary, xyz, color, label)
    write_ascii_ply(text, xyz, color, label)
    for path in (binary, text):
        got = io_util.read_ply(path)
        assert got.dtype == np.float32 and got.shape == (37, 3) and np.array_equal(got.view(np.int32), xyz.view(np.int32))
        got_xyz, got_label = io_util.read_label_ply(path)
        assert np.array_equal(got_xyz.view(np.int32), xyz.view(np.int32))
        assert got_label.dtype == np.uint16 and got_label.shape == (37,) and np.array_equal(got_label, label)
        rows = io_util.read_color_ply(path)
        assert rows.dtype == np.float32 and rows.shape == (37, 6)                   # what numpy's stack makes of float and uchar columns
        assert np.array_equal(rows[:, :3].view(np.int32), xyz.view(np.int32)) and np.array_equal(rows[:, 3:], color.astype(np.float32))
    PR.write_binary_ply(binary, xyz, color)                                         # ScanNet's _vh_clean_2.ply: no label
    assert io_util.read_color_ply(binary).shape == (37, 6)
    with pytest.raises(ValueError, match="label"):
        io_util.read_label_ply(binary)


@pytest.mark.parametrize("text", [True, False], ids=["ascii", "binary"])
def test_written_files_read_back_bit_for_bit(tmp_path, text):
    from gspn_amd import io_util
    xyz, color, _ = cloud()
    path = str(tmp_path / "out.ply")
    io_util.write_color_ply(np.concatenate((xyz, color.astype(np.float32)), 1), path, text=text)
    rows = io_util.read_color_ply(path)
    assert rows.dtype == np.float32 and np.array_equal(rows[:, :3].view(np.int32), xyz.view(np.int32))             # -0.0 and the denormal included
    assert np.array_equal(rows[:, 3:].astype(np.uint8), color) and np.array_equal(rows[:, 3:], color.astype(np.float32))
    head = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii").splitlines()
    assert head == ["ply", "format %s 1.0" % ("ascii" if text else "binary_little_endian"), "comment vertices", "element vertex 37",
                    "property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue"]
    io_util.write_ply(xyz.astype(np.float64), path, text=text)
    assert np.array_equal(io_util.read_ply(path).view(np.int32), xyz.view(np.int32))
    with pytest.raises(ValueError):
        io_util.read_color_ply(path)                                                # write_ply's file has no colours


def test_label_txt_bytes_equal_the_restated_writer(tmp_path):
    from gspn_amd import io_util
    label = np.array([0, -1, 39, 7, -1, 65535, 1234567, 0], dtype=np.int64)
    path = str(tmp_path / "l.txt")
    for values in (label, label.astype(np.int32), torch.from_numpy(label).numpy(), label.tolist()):
        io_util.write_label_txt(values, path)
        assert open(path, "rb").read() == PR.label_lines(label) == b"0\n-1\n39\n7\n-1\n65535\n1234567\n0\n"
    got = io_util.read_label_txt(path)
    assert isinstance(got, np.ndarray) and got.tolist() == label.tolist()
    assert io_util.read_txt(path) == [str(v) for v in label.tolist()]
    (tmp_path / "names.txt").write_text("scene0000_00 \n  scene0001_00\n")
    assert io_util.read_txt(str(tmp_path / "names.txt")) == ["scene0000_00", "scene0001_00"]


def test_files_the_reader_does_not_take_raise_by_name(tmp_path):
    from gspn_amd import io_util
    head = "ply\nformat %s 1.0\nelement vertex 1\n%sproperty float x\nproperty float y\nproperty float z\nend_header\n"
    big = tmp_path / "big_endian.ply"
    big.write_bytes((head % ("binary_big_endian", "")).encode() + b"\0" * 12)
    with pytest.raises(ValueError, match="big_endian.ply"):
        io_util.read_ply(str(big))
    lst = tmp_path / "list_first.ply"
    lst.write_bytes((head % ("ascii", "property list uchar int weights\n")).encode() + b"0 1 2 3\n")
    with pytest.raises(ValueError, match="list_first.ply.*list"):
        io_util.read_ply(str(lst))
    short = tmp_path / "short.ply"
    short.write_bytes((head % ("binary_little_endian", "")).encode() + b"\0" * 11)
    with pytest.raises(ValueError, match="short.ply"):
        io_util.read_ply(str(short))
    nothing = tmp_path / "nothing.ply"
    nothing.write_bytes(b"solid\n")
    with pytest.raises(ValueError, match="nothing.ply"):
        io_util.read_ply(str(nothing))


# ---- the tools ---------------------------------------------------------------------------------------------------------------------------

def load_tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_arguments():
    tool = load_tool("data_prep")
    a = tool.parse_args(["./data/scannet", "./data/scannet_preprocessed"])          # the reference's form
    assert (a.dataset_path, a.out_path, a.nsample, a.scans) == ("./data/scannet", "./data/scannet_preprocessed", 30000, None)
    assert a.batch == tool.DEFAULT_BATCH >= 1
    a = tool.parse_args(["in", "out", "--nsample", "2000", "--batch", "4", "--scans", "scene0001_00,scene0000_00"])
    assert (a.nsample, a.batch, a.scans) == (2000, 4, ["scene0001_00", "scene0000_00"])
    for argv in ([], ["./data/scannet"], ["a", "b", "c"]):
        with pytest.raises(SystemExit):
            tool.parse_args(argv)
    cache = load_tool("make_cache")
    a = cache.parse_args(["--mesh_path", "m", "--label_path", "l", "--list", "train.txt", "--out", "train.pt"])
    assert (a.mesh_path, a.label_path, a.list, a.out, a.npoint, a.npoint_ins, a.seed) == ("m", "l", "train.txt", "train.pt", 18000, 512, 0)
    a = cache.parse_args(["--mesh_path", "m", "--label_path", "l", "--list", "t", "--out", "o", "--npoint", "1024", "--npoint_ins", "64", "--seed", "5"])
    assert (a.npoint, a.npoint_ins, a.seed) == (1024, 64, 5)
    for missing in range(4):
        argv = [["--mesh_path", "m"], ["--label_path", "l"], ["--list", "t"], ["--out", "o"]]
        del argv[missing]
        with pytest.raises(SystemExit):
            cache.parse_args([w for pair in argv for w in pair])
