"""CPU tests of mask components (gspn_amd/components.py): the four symbols in the header, the library and the binding with
the ABI still 21; the host-side declines of the entry points, which launch nothing; the workspace sizes against the layout; the sanitized
host-side check program; the mesh reader and writer of io_util; synth.scan_faces' properties; the numpy restatement
(tests/components_ref.py) against a brute-force search; the wrappers' and the drivers' guards, which raise before the library is touched;
and the flag errors of tools/test.py."""
import ctypes
import importlib.util
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import components_ref as ref
from tests.args_check import run_args_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_components_symbols_are_declared_exported_and_bound_at_abi_21():
    from gspn_amd import _lib, build, components
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    assert "#define GSPN_ABI_VERSION 21" in text and int(lib.gspn_abi_version()) == 21 == _lib.ABI_VERSION
    assert "Additive at 21: gspn_mask_components, gspn_mask_component_filter (+ their _ws_bytes)" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("gspn_mask_components", 10), ("gspn_mask_component_filter", 13)):
        declared = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        assert len(declared) == len(_lib.SIGNATURES[name]) == nargs and hasattr(raw, name)
    assert _lib.SIGNATURES["gspn_mask_component_filter"][6] is ctypes.c_double                          # min_share is a double across the ABI
    assert _lib.SIGNATURES["gspn_mask_component_filter"][5] is ctypes.c_int
    three = ([ctypes.c_int] * 3, ctypes.c_long)
    for name in ("gspn_mask_components_ws_bytes", "gspn_mask_component_filter_ws_bytes"):
        assert re.search(r"\blong %s\s*\(int r, int v, int f\)" % name, code) and _lib.SPECIAL[name] == three and hasattr(raw, name)
    assert components.COMPONENTS_MAX_R == int(re.search(r"#define GSPN_MASK_COMPONENTS_MAX_R (\d+)", text).group(1)) == 1024
    assert components.COMPONENTS_MAX_V == 1 << int(re.search(r"#define GSPN_MASK_COMPONENTS_MAX_V \(1 << (\d+)\)", text).group(1)) == 1 << 24
    assert components.COMPONENTS_MAX_F == 1 << int(re.search(r"#define GSPN_MASK_COMPONENTS_MAX_F \(1 << (\d+)\)", text).group(1)) == 1 << 26
    assert "components.hip" not in build.POLICY_SOURCES and os.path.exists(os.path.join(build.CSRC, "components.hip"))


def test_every_decline_comes_back_before_a_launch_and_the_workspaces_follow_the_layout():
    """null and dangling pointers throughout: a call that launched anything would fault"""
    from gspn_amd import _lib, build
    build.build()
    lib = _lib.lib()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(24)
    # p: masks, faces, ws, comp, ncomp, largest / masks, faces, ws, out, mask_points, ncomp, nkept
    mc = lambda r=3, v=9, f=5, p=(one,) * 6: lib.gspn_mask_components(r, v, f, p[0], p[1], p[2], p[3], p[4], p[5], null)                   # noqa: E731
    mf = lambda r=3, v=9, f=5, mv=1, sh=0.5, p=(one,) * 7: lib.gspn_mask_component_filter(r, v, f, p[0], p[1], mv, sh, p[2], p[3], p[4], p[5], p[6], null)      # noqa: E731
    assert mc(r=-1) == mc(v=-1) == mc(f=-1) == mf(r=-1) == mf(v=-1) == mf(f=-1) == -1
    assert all(mc(p=tuple(null if i == k else one for i in range(6))) == -1 for k in range(6))
    assert all(mf(p=tuple(null if i == k else one for i in range(7))) == -1 for k in range(7))
    assert mf(mv=0) == mf(mv=-3) == -1
    assert all(mf(sh=sh) == -1 for sh in (float("nan"), -1e-9, 1.0000001, 2.0, float("inf"), float("-inf")))
    big_v, big_f = (1 << 24) + 1, (1 << 26) + 1
    assert mc(r=1025) == mc(v=big_v) == mc(f=big_f) == mf(r=1025) == mf(v=big_v) == mf(f=big_f) == -2
    assert mc(p=(one, one, odd, one, one, one)) == -2 and mf(p=(one, one, odd, one, one, one, one)) == -2                 # a ws that is not 16-byte aligned
    assert mf(r=1025, mv=0) == -1 and mc(r=1025, p=(null,) + (one,) * 5) == -1                                       # an argument error goes first
    assert mc(r=0) == mc(v=0) == mf(r=0) == mf(v=0) == 0                                                              # nothing to do
    assert mc(r=0, f=0, p=(one, null, one, one, one, one)) == 0 and mf(v=0, f=0, p=(one, null) + (one,) * 5) == 0        # no faces: faces may be null
    # the workspaces: v * ceil(r / 64) words, then r * v and r int32; the filter r * v and r int32 more; every part 16-byte aligned
    cb, fb = lib.gspn_mask_components_ws_bytes, lib.gspn_mask_component_filter_ws_bytes
    up = lambda n: (n + 15) // 16 * 16                                                                  # noqa: E731
    for r, v, f in ((1, 1, 0), (3, 9, 5), (3, 100, 5), (64, 17, 9), (65, 17, 9), (130, 20001, 40000), (100, 500000, 1 << 20), (129, 1 << 24, 7),
                    (1024, 1 << 24, 1 << 26)):
        words = (r + 63) // 64
        bad = up(up(8 * v * words) + 4 * r * v)
        assert cb(r, v, f) == bad + 4 * r, (r, v, f)
        assert fb(r, v, f) == up(up(bad + 4 * r) + 4 * r * v) + 4 * r, (r, v, f)
    for args in ((-1, 9, 5), (3, -1, 5), (3, 9, -1), (0, 9, 5), (3, 0, 5), (1025, 9, 5), (3, big_v, 5), (3, 9, big_f)):
        assert cb(*args) == 0 and fb(*args) == 0, args


def test_the_argument_checks_hold_under_the_host_sanitizers(tmp_path):
    """tools/components_args_check.cpp: the launchers' host-side checks and workspace layouts as a program of their own, built with the
    address and undefined-behaviour sanitizers and run over the decline table -- never loaded into Python"""
    run_args_check("components_args_check", tmp_path)


# ---- the mesh files --------------------------------------------------------------------------------------------------------------------
def test_the_faces_of_a_mesh_file_round_trip(tmp_path):
    from gspn_amd import io_util
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((37, 3)).astype(np.float32)
    faces = rng.integers(0, 37, size=(55, 3)).astype(np.int32)
    for text, kind in itertools.product((True, False), ("int", "uint")):
        path = str(tmp_path / ("mesh_%d_%s.ply" % (text, kind)))
        io_util.write_mesh_ply(pts, faces, path, text=text, index_type=kind)
        got = io_util.read_ply_faces(path)
        assert got.dtype == np.int32 and got.shape == (55, 3) and got.flags.c_contiguous and np.array_equal(got, faces)
        assert np.array_equal(io_util.read_ply(path), pts)            # the vertex readers pass the face element over, as they did
    path = str(tmp_path / "none.ply")
    io_util.write_mesh_ply(pts, np.zeros((0, 3), np.int64), path)     # no faces
    assert io_util.read_ply_faces(path).shape == (0, 3)
    io_util.write_mesh_ply(pts, np.array([[0, -1, 5]]), path)         # a negative int index is the reader's to return
    assert io_util.read_ply_faces(path).tolist() == [[0, -1, 5]]
    # the type names int32 / uint32 / uint8, and a vertex element with colours in front (ScanNet's)
    body = np.zeros(2, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
    rows = np.zeros(2, dtype=[("n", "u1"), ("i", "<u4", (3,))])
    rows["n"], rows["i"] = 3, [[0, 1, 1], [1, 0, 7]]
    header = ("ply\nformat binary_little_endian 1.0\ncomment x\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face 2\n"
              "property list uint8 uint32 vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode() + body.tobytes() + rows.tobytes())
    assert io_util.read_ply_faces(path).tolist() == [[0, 1, 1], [1, 0, 7]] and io_util.read_color_ply(path).shape == (2, 6)
    with open(path, "wb") as f:
        f.write(header.replace("uint8 uint32", "uchar int32").encode() + body.tobytes() + rows.tobytes())
    assert io_util.read_ply_faces(path).tolist() == [[0, 1, 1], [1, 0, 7]]


def test_the_face_reader_refuses_what_it_cannot_read(tmp_path):
    from gspn_amd import io_util
    pts = np.zeros((4, 3), np.float32)
    faces = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    path, bad = str(tmp_path / "good.ply"), str(tmp_path / "bad.ply")

    def rewritten(text, change):
        io_util.write_mesh_ply(pts, faces, path, text=text)
        with open(path, "rb") as f:
            data = f.read()
        with open(bad, "wb") as f:
            f.write(change(data))
        return bad

    for text in (True, False):
        with pytest.raises(ValueError):                               # truncated: the last face is missing
            io_util.read_ply_faces(rewritten(text, lambda d: d[:-8] if text else d[:-5]))
        with pytest.raises(ValueError, match="no face element"):      # a file of vertices alone
            io_util.write_ply(pts, bad, text=text)
            io_util.read_ply_faces(bad)
        with pytest.raises(ValueError, match="face element must hold one list property"):
            io_util.read_ply_faces(rewritten(text, lambda d: d.replace(b"list uchar int", b"list ushort int")))
        with pytest.raises(ValueError, match="face element must hold one list property"):
            io_util.read_ply_faces(rewritten(text, lambda d: d.replace(b"list uchar int", b"list uchar short")))
        with pytest.raises(ValueError, match="is not read"):
            io_util.read_ply_faces(rewritten(text, lambda d: d.replace(b"format ascii", b"format binary_big_endian").replace(b"format binary_little_endian", b"format binary_big_endian")))
    with pytest.raises(ValueError, match="face 1 is not a triangle"):
        io_util.read_ply_faces(rewritten(True, lambda d: d.replace(b"3 1 2 3\n", b"4 1 2 3 0\n")))
    with pytest.raises(ValueError, match="face 0 is not a triangle"):
        io_util.read_ply_faces(rewritten(False, lambda d: d[:-26] + b"\x04" + d[-25:]))
    with pytest.raises(ValueError, match="not a PLY file"):
        io_util.read_ply_faces(rewritten(True, lambda d: b"xx" + d))
    for wrong in (np.zeros((2, 4), np.int32), np.zeros((2, 3), np.float32), np.zeros(3, np.int32)):
        with pytest.raises(ValueError):
            io_util.write_mesh_ply(pts, wrong, bad)
    with pytest.raises(ValueError):
        io_util.write_mesh_ply(pts, faces, bad, index_type="short")


def test_the_existing_writers_keep_their_bytes(tmp_path):
    from gspn_amd import io_util
    pts = np.array([[0.5, -1.25, 3.0], [1e-3, 2.0, -0.0]], np.float32)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    io_util.write_ply(pts, a)
    assert open(a, "rb").read() == (b"ply\nformat ascii 1.0\ncomment vertices\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                                    b"end_header\n0.5 -1.25 3\n0.00100000005 2 -0\n")
    io_util.write_mesh_ply(pts, np.zeros((0, 3), np.int32), b)
    assert open(b, "rb").read().replace(b"element face 0\nproperty list uchar int vertex_indices\n", b"") == open(a, "rb").read()


# ---- the synthetic mesh ------------------------------------------------------------------------------------------------------------------
def scan(seed, v=900):
    rng = np.random.default_rng(seed)
    xyz = rng.random((v, 3)).astype(np.float32) * 2
    seg = rng.integers(0, 3, size=v).astype(np.int32)
    group = rng.integers(0, 5, size=v).astype(np.int32)
    seg[:3], group[:3] = [7, 8, 8], [9, 9, 9]                         # an instance of one vertex and one of two
    return xyz, seg, group


def test_scan_faces_joins_every_instance_and_nothing_else():
    from gspn_amd import synth
    xyz, seg, group = scan(5)
    v = xyz.shape[0]
    inst = seg.astype(np.int64) * 100 + group
    faces = synth.scan_faces(xyz, seg, group, 0.5, seed=4)
    assert faces.dtype == np.int32 and faces.ndim == 2 and faces.shape[1] == 3 and faces.flags.c_contiguous
    assert faces.min() >= 0 and faces.max() < v
    edges = ref.edges_ref(faces, v)
    assert (inst[edges[:, 0]] == inst[edges[:, 1]]).all()             # no edge joins two instances
    comp = ref.row_components_ref(np.ones(v, bool), edges)
    for g in np.unique(inst):
        assert np.unique(comp[inst == g]).size == 1                   # every instance is one connected piece
    assert np.unique(comp).size == np.unique(inst).size
    assert np.array_equal(faces, synth.scan_faces(xyz, seg, group, 0.5, seed=4))                      # seeded
    assert not np.array_equal(faces, synth.scan_faces(xyz, seg, group, 0.5, seed=5))
    for bridges in (1, 7):
        more = synth.scan_faces(xyz, seg, group, 0.5, seed=4, bridges=bridges)
        e = ref.edges_ref(more, v)
        cross = e[inst[e[:, 0]] != inst[e[:, 1]]]
        assert np.unique(np.sort(cross, axis=1), axis=0).shape[0] == bridges                        # exactly the asked number of edges
        assert cross.shape[0] == 2 * bridges                          # (a face (a, b, b) names its one edge twice)
        assert more.shape[0] == faces.shape[0] + bridges
    for bad in (dict(cell=0.0), dict(bridges=-1)):
        with pytest.raises(ValueError):
            synth.scan_faces(xyz, seg, group, **{"cell": 0.5, "seed": 1, **bad})
    with pytest.raises(ValueError):
        synth.scan_faces(xyz[:5], seg, group, 0.5, 1)
    with pytest.raises(ValueError, match="two instances"):
        synth.scan_faces(xyz, np.zeros(v, np.int32), np.zeros(v, np.int32), 0.5, 1, bridges=1)
    assert synth.scan_faces(np.zeros((0, 3), np.float32), [], [], 0.5, 1).shape == (0, 3)


def test_the_other_synthetic_draws_are_what_they_were():
    """scan_faces has its own generator: scan_vertices and scan_segments keep their draws (the values below are the parent's)"""
    from gspn_amd import synth
    pc = synth.cloud_u(50, 1)
    xyz, seg, group = synth.scan_vertices(pc, np.arange(50) % 3, np.arange(50) % 4, 80, seed=2)
    ids = synth.scan_segments(xyz, seg, group, 0.3, seed=2)
    rng = np.random.default_rng(7919 * 2 + 3)
    parent = rng.integers(0, 50, size=30)
    assert np.array_equal(seg[50:], (np.arange(50) % 3)[parent]) and np.array_equal(xyz[:50], pc)
    assert ids.dtype == np.int64 and ids.shape == (80,)
    faces = synth.scan_faces(xyz, seg, group, 0.3, seed=2)            # drawing faces in between changes neither
    assert np.array_equal(ids, synth.scan_segments(xyz, seg, group, 0.3, seed=2)) and faces.shape[1] == 3


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def brute(masks, faces):
    """breadth-first search from every set vertex in index order, on an adjacency matrix"""
    r, v = masks.shape
    adj = np.zeros((v, v), bool)
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        for u, w in ((a, b), (b, c), (a, c)):
            if 0 <= u < v and 0 <= w < v:
                adj[u, w] = adj[w, u] = True
    comp = np.full((r, v), -1, np.int32)
    for k in range(r):
        on = masks[k] != 0
        for x in range(v):
            if on[x] and comp[k, x] < 0:
                todo, comp[k, x] = [x], x
                while todo:
                    u = todo.pop()
                    for w in np.flatnonzero(adj[u] & on).tolist():
                        if comp[k, w] < 0:
                            comp[k, w] = x
                            todo.append(w)
    return comp


def test_the_restatement_against_a_brute_force_search():
    rng = np.random.default_rng(0)
    for _ in range(150):
        r, v, f = int(rng.integers(1, 5)), int(rng.integers(1, 13)), int(rng.integers(0, 14))
        masks = (rng.integers(0, 256, size=(r, v)) * (rng.random((r, v)) < rng.choice([0.3, 0.8]))).astype(np.uint8)
        faces = rng.integers(-2, v + 2, size=(f, 3))                  # ends outside [0, v), duplicate and degenerate faces included
        comp, ncomp, largest = ref.mask_components_ref(masks, faces)
        want = brute(masks, faces)
        assert comp.dtype == np.int32 and np.array_equal(comp, want)
        sizes = [np.bincount(w[w >= 0], minlength=v) for w in want]
        assert ncomp.tolist() == [int((s > 0).sum()) for s in sizes] and largest.tolist() == [int(s.max()) for s in sizes]
        for mv, share in ((1, 0.0), (2, 0.0), (1, 0.5), (3, 1.0), (1, 1.0)):
            out, points, nc, nk = ref.component_filter_ref(masks, faces, mv, share)
            for k in range(r):
                kept = [x for x in range(v) if sizes[k][x] >= mv and sizes[k][x] > 0 and float(sizes[k][x]) >= share * float(sizes[k].max())]
                assert out[k].tolist() == [int(want[k, x] in kept) for x in range(v)] and nk[k] == len(kept)
            assert np.array_equal(nc, ncomp) and np.array_equal(points, out.sum(1)) and out.dtype == np.uint8
        assert np.array_equal(ref.component_filter_ref(masks, faces, 1, 0.0)[0], (masks != 0).astype(np.uint8))          # the identity


def test_the_restatement_on_a_hand_written_case():
    # 0-1-2 a triangle; 4-5 a pair; 7 alone; the edges 2-3 and 3-4 would join them, but 3 is not set in row 0
    faces = np.array([[0, 1, 2], [2, 3, 3], [3, 3, 4], [4, 5, 5], [7, 7, 7], [9, 5, 9]])
    masks = np.array([[1, 1, 1, 0, 1, 1, 0, 1], [1, 1, 1, 9, 1, 1, 0, 0], [0] * 8], np.uint8)
    comp, ncomp, largest = ref.mask_components_ref(masks, faces)
    assert comp.tolist() == [[0, 0, 0, -1, 4, 4, -1, 7], [0, 0, 0, 0, 0, 0, -1, -1], [-1] * 8]
    assert ncomp.tolist() == [3, 1, 0] and largest.tolist() == [3, 6, 0]
    out, points, _, nkept = ref.component_filter_ref(masks, faces, 2, 0.0)
    assert out.tolist() == [[1, 1, 1, 0, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1, 0, 0], [0] * 8] and points.tolist() == [5, 6, 0] and nkept.tolist() == [2, 1, 0]
    assert ref.component_filter_ref(masks, faces, 1, 1.0)[0][0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert ref.component_filter_ref(masks, faces, 1, 2.0 / 3.0)[3].tolist() == [2 if 2.0 >= 2.0 / 3.0 * 3.0 else 1, 1, 0]   # the doubles' compare


# ---- the guards ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_raise_before_anything_runs(monkeypatch):
    from gspn_amd import _lib, components as C
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    masks = torch.zeros(3, 12, dtype=torch.uint8)
    faces = torch.zeros(4, 3, dtype=torch.int32)
    for bad in (masks[0], masks[None], masks.int(), masks[:0], masks[:, :0]):
        with pytest.raises(ValueError):
            C.mask_components(bad, faces)
        with pytest.raises(ValueError):
            C.component_filter(bad, faces, min_vertices=1)
    for bad in (faces.long(), faces[:, :2], faces[0], faces.float()):
        with pytest.raises(ValueError):
            C.mask_components(masks, bad)
        with pytest.raises(ValueError):
            C.component_filter(masks, bad, min_vertices=1)
    with pytest.raises(TypeError):
        C.mask_components(masks.numpy(), faces)
    with pytest.raises(TypeError):
        C.component_filter(masks, faces)                              # min_vertices has no default
    for kw in (dict(min_vertices=0), dict(min_vertices=-1), dict(min_vertices=1.5), dict(min_vertices=True), dict(min_vertices=1, min_share=-0.1),
               dict(min_vertices=1, min_share=1.01), dict(min_vertices=1, min_share=float("nan")),
               dict(min_vertices=1, out=torch.zeros(3, 11, dtype=torch.uint8)), dict(min_vertices=1, out=torch.zeros(3, 12)),
               dict(min_vertices=1, ws=torch.zeros(4096)), dict(min_vertices=1, ws=torch.zeros(8, 8, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            C.component_filter(masks, faces, **kw)
    with pytest.raises(ValueError):
        C.mask_components(masks, faces, ws=torch.zeros(4096))
    for bad in (torch.zeros(1025, 1, dtype=torch.uint8), torch.zeros(1, (1 << 24) + 1, dtype=torch.uint8)):
        with pytest.raises(NotImplementedError):
            C.mask_components(bad, faces)
        with pytest.raises(NotImplementedError):
            C.component_filter(bad, faces, min_vertices=1)
    many = torch.zeros(1, dtype=torch.int32).expand((1 << 26) + 1, 3)
    with pytest.raises(NotImplementedError):
        C.mask_components(masks, many)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):         # there is no CPU fallback
        C.mask_components(masks, faces)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        C.component_filter(masks, faces, min_vertices=1)
    # mesh_faces
    for bad in (np.zeros((2, 4), np.int32), np.zeros(3, np.int64), np.zeros((2, 3), np.float32), torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.bool),
                np.array([[0, 1, -1]]), torch.tensor([[0, 1, 1 << 31]])):
        with pytest.raises(ValueError):
            C.mesh_faces(bad, 10)
    with pytest.raises(ValueError):
        C.mesh_faces(np.zeros((2, 3), np.int32), -1)
    with pytest.raises(TypeError):
        C.mesh_faces([[0, 1, 2]], 10)


def test_the_drivers_check_their_arguments_before_anything_runs(monkeypatch):
    from gspn_amd import _lib, lift
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    b, n, r, p, c, sd, v = 1, 20, 3, 8, 5, 6, 30
    ep = {"detections": torch.zeros(b, r, 8), "rpointnet_mask_selected": torch.zeros(b, r, p),
          "pc_coord_cropped_final_unnormalized": torch.zeros(b, r, p, 3), "pc_seed": torch.zeros(b, sd, 3), "fb_prob": torch.zeros(b, sd, 2),
          "sem_class_logits": torch.zeros(b, n, c)}
    call = lambda **kw: lift.scan_predictions(ep, 0, torch.zeros(v, 3), pc=torch.zeros(b, n, 3), label_map=list(range(c)), **kw)      # noqa: E731
    faces = torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="faces and min_component go together"):
        call(faces=faces)
    with pytest.raises(ValueError, match="faces and min_component go together"):
        call(min_component=5)
    for kw in (dict(min_component=0), dict(min_component=2.5), dict(min_component=1, min_component_share=1.5),
               dict(min_component=1, min_component_share=float("nan"))):
        with pytest.raises(ValueError, match="scan_predictions: min_"):
            call(faces=faces, **kw)
    for bad in (faces.long(), faces[:, :2], faces[0]):
        with pytest.raises(ValueError):
            call(faces=bad, min_component=1)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        call(faces=faces, min_component=1)


def test_the_tester_and_the_tool_check_the_parameters():
    from gspn_amd import components as C
    assert C._parameters(1, 0, "x") == (1, 0.0) and C._parameters(np.int64(7), 1, "x") == (7, 1.0)
    spec = importlib.util.spec_from_file_location("tools_test", os.path.join(ROOT, "tools", "test.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.parse(["--synthetic", "2"]).components is None and tool.parse(["--synthetic", "2"]).component_share == 0.0
    a = tool.parse(["--synthetic", "2", "--synthetic_vertices", "20000", "--components", "50", "--component_share", "0.25"])
    assert a.components == 50 and a.component_share == 0.25
    with pytest.raises(SystemExit, match="--components goes with the vertex modes"):
        tool.main(["--synthetic", "2", "--components", "5"])
    with pytest.raises(SystemExit, match="--component_share goes with --components"):
        tool.main(["--synthetic", "2", "--synthetic_vertices", "20000", "--component_share", "0.5"])
    for extra in (["--components", "0"], ["--components", "5", "--component_share", "1.5"], ["--components", "5", "--component_share", "nan"]):
        with pytest.raises(SystemExit, match="--components must be at least 1"):
            tool.main(["--synthetic", "2", "--synthetic_vertices", "20000"] + extra)
    xyz, seg, group = scan(6, 300)
    cache = {"pc": torch.from_numpy(xyz[None, :200]), "seg_label": torch.from_numpy(seg[None, :200]), "group_label": torch.from_numpy(group[None, :200])}
    got = tool.synthetic_vertices(cache, 300, 3, None, 0.5)(0)
    assert set(got) == {"xyz", "seg_label", "group_label", "faces"} and got["faces"].shape[1] == 3 and got["faces"].max() < 300
    assert set(tool.synthetic_vertices(cache, 300, 3)(0)) == {"xyz", "seg_label", "group_label"}
