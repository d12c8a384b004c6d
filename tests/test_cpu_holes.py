"""CPU tests of mask holes (gspn_amd/holes.py): the two symbols in the header, the library and the binding with the ABI
still 21; the host-side declines of the entry point, which launches nothing; the workspace size against the layout; the sanitized
host-side check program; the numpy restatement (tests/holes_ref.py) against a brute-force search and on a hand-written lattice that pins
each clause of the rule; the wrapper's, the drivers', the tester's and the tool's guards, which raise before the library is touched."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import holes_ref as ref
from tests.args_check import run_args_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_hole_fill_symbols_are_declared_exported_and_bound_at_abi_21():
    from gspn_amd import _lib, build, holes
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    assert "#define GSPN_ABI_VERSION 21" in text and int(lib.gspn_abi_version()) == 21 == _lib.ABI_VERSION
    assert "Additive at 21: gspn_mask_hole_fill (+ gspn_mask_hole_fill_ws_bytes)" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    declared = re.search(r"\bint gspn_mask_hole_fill\s*\(([^)]*)\)", code).group(1).split(",")
    assert len(declared) == len(_lib.SIGNATURES["gspn_mask_hole_fill"]) == 15 and hasattr(raw, "gspn_mask_hole_fill")
    assert _lib.SIGNATURES["gspn_mask_hole_fill"][7] is ctypes.c_double and _lib.SIGNATURES["gspn_mask_hole_fill"][6] is ctypes.c_int     # max_share is a double across the ABI
    assert re.search(r"\blong gspn_mask_hole_fill_ws_bytes\s*\(int r, int v, int f\)", code) and hasattr(raw, "gspn_mask_hole_fill_ws_bytes")
    assert _lib.SPECIAL["gspn_mask_hole_fill_ws_bytes"] == ([ctypes.c_int] * 3, ctypes.c_long)
    assert holes.HOLE_FILL_MAX_R == int(re.search(r"#define GSPN_MASK_HOLE_FILL_MAX_R (\d+)", text).group(1)) == 1024
    assert holes.HOLE_FILL_MAX_V == 1 << int(re.search(r"#define GSPN_MASK_HOLE_FILL_MAX_V \(1 << (\d+)\)", text).group(1)) == 1 << 24
    assert holes.HOLE_FILL_MAX_F == 1 << int(re.search(r"#define GSPN_MASK_HOLE_FILL_MAX_F \(1 << (\d+)\)", text).group(1)) == 1 << 26
    source = open(os.path.join(build.CSRC, "components.hip")).read()
    assert 'extern "C" int gspn_mask_hole_fill(' in source            # beside the kernels it reuses


def test_every_decline_comes_back_before_a_launch_and_the_workspace_follows_the_layout():
    """null and dangling pointers throughout: a call that launched anything would fault"""
    from gspn_amd import _lib, build
    build.build()
    lib = _lib.lib()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(24)
    # p: masks, faces, xyz, ws, out, mask_points, nholes, nfilled, label
    hf = lambda r=3, v=9, f=5, mv=4, sh=0.5, p=(one,) * 9: lib.gspn_mask_hole_fill(r, v, f, p[0], p[1], p[2], mv, sh, p[3], p[4], p[5], p[6], p[7], p[8], null)      # noqa: E731
    assert hf(r=-1) == hf(v=-1) == hf(f=-1) == -1
    assert all(hf(p=tuple(null if i == k else one for i in range(9))) == -1 for k in range(8))
    assert hf(mv=-1) == hf(mv=-(1 << 31)) == -1
    assert all(hf(sh=sh) == -1 for sh in (float("nan"), -1e-9, 1.0000001, 2.0, float("inf"), float("-inf")))
    big_v, big_f = (1 << 24) + 1, (1 << 26) + 1
    assert hf(r=1025) == hf(v=big_v) == hf(f=big_f) == -2
    assert hf(p=(one, one, one, odd) + (one,) * 5) == -2                                                               # a ws that is not 16-byte aligned
    assert hf(r=1025, mv=-1) == -1 and hf(v=big_v, p=(null,) + (one,) * 8) == -1 and hf(r=1025, sh=float("nan"), p=(one, one, one, odd) + (one,) * 5) == -1   # an argument error goes first
    assert hf(r=0) == hf(v=0) == 0                                                                                     # nothing to do
    assert hf(r=0, p=(one,) * 8 + (null,)) == 0 and hf(v=0, f=0, p=(one, null) + (one,) * 6 + (null,)) == 0               # label, and faces without faces, may be null
    assert hf(r=0, f=5, p=(one, null) + (one,) * 7) == -1                                                                # faces with faces may not
    # the workspace: two tables of v * ceil(r / 64) words, then r * v, r, 6 r, r and r * v int32; every part 16-byte aligned
    wb = lib.gspn_mask_hole_fill_ws_bytes
    up = lambda n: (n + 15) // 16 * 16                                                                  # noqa: E731
    for r, v, f in ((1, 1, 0), (3, 9, 5), (3, 100, 5), (64, 17, 9), (65, 17, 9), (130, 20001, 40000), (100, 500000, 1 << 20), (129, 1 << 24, 7),
                    (1024, 1 << 24, 1 << 26)):
        table = 8 * v * ((r + 63) // 64)
        at = up(up(table) + table)                                    # size
        at = up(at + 4 * r * v)                                       # bad
        at = up(at + 4 * r)                                           # box
        at = up(at + 24 * r)                                          # points_in
        at = up(at + 4 * r)                                           # parent
        assert wb(r, v, f) == at + 4 * r * v, (r, v, f)
    for args in ((-1, 9, 5), (3, -1, 5), (3, 9, -1), (0, 9, 5), (3, 0, 5), (1025, 9, 5), (3, big_v, 5), (3, 9, big_f)):
        assert wb(*args) == 0, args
    layout = open(os.path.join(ROOT, "gspn_amd", "csrc", "holes_args.h")).read()
    assert "cand[v][words]" in layout and "set[v][words]" in layout and "int size[r][v]" in layout and "int box[r][6]" in layout          # the layout is stated
    assert "int points_in[r]" in layout and "int parent[r][v]" in layout and "int bad[r]" in layout


def test_the_argument_checks_hold_under_the_host_sanitizers(tmp_path):
    """tools/holes_args_check.cpp: the launcher's host-side checks and workspace layout as a program of their own, built with the address
    and undefined-behaviour sanitizers and run over the decline table -- never loaded into Python"""
    run_args_check("holes_args_check", tmp_path)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def brute(masks, faces, xyz, max_vertices, max_share):
    """The rule read another way round: breadth-first search on an adjacency matrix over the FULL complement of the row; a complement
    component is a hole iff every vertex of it is inside the box, it touches, and its size fits.  A candidate component that is not open
    is a whole complement component inside the box, and the other way round."""
    r, v = masks.shape
    adj = np.zeros((v, v), bool)
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        for u, w in ((a, b), (b, c), (a, c)):
            if 0 <= u < v and 0 <= w < v and u != w:
                adj[u, w] = adj[w, u] = True
    out = (masks != 0).astype(np.uint8)
    nholes, nfilled = np.zeros(r, np.int32), np.zeros(r, np.int32)
    for k in range(r):
        on = masks[k] != 0
        finite = [x for x in range(v) if on[x] and all(np.isfinite(float(c)) for c in xyz[x])]
        inside = np.zeros(v, bool)
        if finite:
            lo = [min(float(xyz[x][a]) for x in finite) for a in range(3)]
            hi = [max(float(xyz[x][a]) for x in finite) for a in range(3)]
            inside = np.array([all(lo[a] <= float(xyz[x][a]) <= hi[a] for a in range(3)) for x in range(v)])
        seen = on.copy()
        for x in range(v):
            if seen[x]:
                continue
            piece, todo = [x], [x]
            seen[x] = True
            while todo:
                u = todo.pop()
                for w in np.flatnonzero(adj[u] & ~on).tolist():
                    if not seen[w]:
                        seen[w] = True
                        piece.append(w)
                        todo.append(w)
            touches = any((adj[u] & on).any() for u in piece)
            s = len(piece)
            if all(inside[u] for u in piece) and touches and s <= max_vertices and float(s) <= max_share * float(on.sum()):
                out[k, piece] = 1
                nholes[k] += 1
                nfilled[k] += s
    return out, (on_count(masks) + nfilled).astype(np.int32), nholes, nfilled


def on_count(masks):
    return (masks != 0).sum(axis=1)


def test_the_restatement_against_a_brute_force_search():
    rng = np.random.default_rng(0)
    filled = 0
    for _ in range(150):
        r, v, f = int(rng.integers(1, 5)), int(rng.integers(1, 13)), int(rng.integers(0, 16))
        masks = (rng.integers(0, 256, size=(r, v)) * (rng.random((r, v)) < rng.choice([0.3, 0.6]))).astype(np.uint8)
        faces = rng.integers(-2, v + 2, size=(f, 3))                  # ends outside [0, v), duplicate and degenerate faces included
        xyz = rng.integers(0, 3, size=(v, 3)).astype(np.float32)      # a coarse lattice: many vertices on a box face, and on one another
        xyz[rng.random(v) < 0.08, int(rng.integers(0, 3))] = rng.choice([np.nan, np.inf, -np.inf, -0.0])
        for mv, share in ((12, 1.0), (2, 1.0), (12, 0.5), (1, 0.25), (0, 1.0)):
            out, points, nholes, nfilled, label = ref.hole_fill_ref(masks, faces, xyz, mv, share)
            want = brute(masks, faces, xyz, mv, share)
            for g, w in zip((out, points, nholes, nfilled), want):
                assert g.dtype == w.dtype and np.array_equal(g, w), (masks, faces, xyz, mv, share)
            assert label.dtype == np.int32 and ((label == -2) == (masks != 0)).all() and (label[(label >= 0)] <= np.nonzero(label >= 0)[1]).all()
            assert np.array_equal(points, out.sum(axis=1))
            filled += int(nfilled.sum())
        assert np.array_equal(ref.hole_fill_ref(masks, faces, xyz, 0)[0], (masks != 0).astype(np.uint8))          # the identity
    assert filled > 100                                               # the cases fill something


def lattice(w, h):
    """-> xyz (w * h, 3), faces, at (h, w): vertex y * w + x at (x, y, 0), two triangles a cell"""
    ys, xs = np.mgrid[0:h, 0:w]
    at = np.arange(w * h).reshape(h, w)
    xyz = np.stack((xs.ravel(), ys.ravel(), np.zeros(w * h)), axis=1).astype(np.float32)
    a, b, c, d = at[:-1, :-1].ravel(), at[:-1, 1:].ravel(), at[1:, :-1].ravel(), at[1:, 1:].ravel()
    return xyz, np.concatenate((np.stack((a, b, c), axis=1), np.stack((b, d, c), axis=1))), at


def test_the_restatement_on_a_hand_written_lattice():
    xyz, faces, at = lattice(9, 7)
    v = 63

    def fill(rows, mv=40, share=1.0, xyz=xyz, faces=faces):
        masks = np.zeros((len(rows), xyz.shape[0]), np.uint8)
        for k, row in enumerate(rows):
            masks[k, row] = 200
        return ref.hole_fill_ref(masks, faces, xyz, mv, share)

    ring = np.ones((5, 5), bool)
    ring[1:-1, 1:-1] = False
    closed = at[1:6, 1:6][ring]                                       # a ring around the 3 x 3 block at[2:5, 2:5]
    inner = at[2:5, 2:5].ravel()
    out, points, nholes, nfilled, label = fill([closed])
    assert nholes.tolist() == [1] and nfilled.tolist() == [9] and points.tolist() == [25] and out[0, inner].all() and out.sum() == 25
    assert (label[0, inner] == inner.min()).all() and (label[0, closed] == -2).all() and label[0, 0] == -1          # a closed ring is filled
    gap = [x for x in closed if x != at[1, 3]]                        # the ring without one vertex of its top side: the gap leads outside the box
    out, _, nholes, nfilled, label = fill([gap])
    assert nholes.tolist() == [0] and out.sum() == 15 and label[0, at[1, 3]] == label[0, inner[0]] == at[1, 3]      # a ring with a gap is open
    # a U: the ring without the inside of its right side; the mouth faces the vertices at hi + 1
    u_shape = [x for x in closed if x not in at[2:5, 5]]
    out, _, nholes, _, label = fill([u_shape])
    assert nholes.tolist() == [0] and (label[0, at[2:5, 5]] >= 0).all() and label[0, at[3, 6]] == -1 and out.sum() == 13
    # the same U with its mouth at the mesh's own border: a lattice that ends at the ring's right side
    xyz6, faces6, at6 = lattice(6, 7)
    ring6 = at6[1:6, 1:6][ring]
    u6 = [x for x in ring6 if x not in at6[2:5, 5]]
    out, _, nholes, nfilled, _ = fill([u6], xyz=xyz6, faces=faces6)
    assert nholes.tolist() == [1] and nfilled.tolist() == [12] and out[0, at6[2:5, 2:6].ravel()].all()
    # a fragment inside the box with no edge to the row, and an isolated unset vertex: two more vertices at the ring's centre, joined to
    # one another alone, and one on no edge; the centre itself is set here, so the hole is the 8 around it
    more = np.concatenate((xyz, np.array([[3, 3, 0]] * 3, np.float32)))
    faces_more = np.concatenate((faces, [[v, v + 1, v + 1]]))
    out, _, nholes, nfilled, label = fill([list(closed) + [at[3, 3]]], xyz=more, faces=faces_more)
    assert nholes.tolist() == [1] and nfilled.tolist() == [8] and out[0, v:].tolist() == [0, 0, 0] and label[0, v:].tolist() == [v, v, v + 2]
    # the size limit and the share rule, each at equality
    assert fill([closed], mv=9)[2].tolist() == [1] and fill([closed], mv=8)[2].tolist() == [0]
    assert fill([closed], share=9.0 / 16.0)[2].tolist() == [1 if 9.0 <= 9.0 / 16.0 * 16.0 else 0] == [1]          # s = 9, 16 set: 9 <= 0.5625 * 16
    assert fill([closed], share=0.5624999999999999)[2].tolist() == [0] and fill([closed], share=0.0)[2].tolist() == [0]
    assert fill([closed], mv=0)[0].sum() == 16
    # an empty row, and a row whose set vertices all carry a NaN
    out, points, nholes, nfilled, label = fill([[], closed])
    assert nholes.tolist() == [0, 1] and not out[0].any() and points.tolist() == [0, 25] and (label[0] == -1).all()
    nan = xyz.copy()
    nan[closed, 2] = np.nan
    out, points, nholes, _, label = fill([closed], xyz=nan)
    assert nholes.tolist() == [0] and points.tolist() == [16] and (label[0][label[0] != -2] == -1).all()


# ---- the guards ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_raises_before_anything_runs(monkeypatch):
    from gspn_amd import _lib, holes as H
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    masks = torch.zeros(3, 12, dtype=torch.uint8)
    faces = torch.zeros(4, 3, dtype=torch.int32)
    xyz = torch.zeros(12, 3)
    for bad in (masks[0], masks[None], masks.int(), masks[:0], masks[:, :0]):
        with pytest.raises(ValueError):
            H.hole_fill(bad, faces, xyz, max_vertices=1)
    for bad in (faces.long(), faces[:, :2], faces[0], faces.float()):
        with pytest.raises(ValueError):
            H.hole_fill(masks, bad, xyz, max_vertices=1)
    for bad in (xyz.double(), xyz[:11], xyz[:, :2], xyz[0], torch.zeros(13, 3), xyz.int()):
        with pytest.raises(ValueError):
            H.hole_fill(masks, faces, bad, max_vertices=1)
    with pytest.raises(TypeError):
        H.hole_fill(masks.numpy(), faces, xyz, max_vertices=1)
    with pytest.raises(TypeError):
        H.hole_fill(masks, faces, xyz)                                # max_vertices has no default
    for kw in (dict(max_vertices=-1), dict(max_vertices=1.5), dict(max_vertices=True), dict(max_vertices=1, max_share=-0.1),
               dict(max_vertices=1, max_share=1.01), dict(max_vertices=1, max_share=float("nan")),
               dict(max_vertices=1, out=torch.zeros(3, 11, dtype=torch.uint8)), dict(max_vertices=1, out=torch.zeros(3, 12)),
               dict(max_vertices=1, ws=torch.zeros(4096)), dict(max_vertices=1, ws=torch.zeros(8, 8, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            H.hole_fill(masks, faces, xyz, **kw)
    for bad, coords in ((torch.zeros(1025, 1, dtype=torch.uint8), torch.zeros(1, 3)),
                        (torch.zeros(1, dtype=torch.uint8).expand(1, (1 << 24) + 1), torch.zeros(1, 3).expand((1 << 24) + 1, 3))):
        with pytest.raises(NotImplementedError):
            H.hole_fill(bad, faces, coords, max_vertices=1)
    many = torch.zeros(1, dtype=torch.int32).expand((1 << 26) + 1, 3)
    with pytest.raises(NotImplementedError):
        H.hole_fill(masks, many, xyz, max_vertices=1)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):         # there is no CPU fallback
        H.hole_fill(masks, faces, xyz, max_vertices=0)


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
        call(faces=faces)                                             # faces alone, as before
    with pytest.raises(ValueError, match="faces and min_component go together"):
        call(min_component=5)
    with pytest.raises(ValueError, match="faces and max_hole go together"):
        call(max_hole=5)
    with pytest.raises(ValueError, match="faces and min_component go together"):
        call(max_hole=5, min_component=5)
    for kw in (dict(max_hole=-1), dict(max_hole=2.5), dict(max_hole=True), dict(max_hole=1, max_hole_share=1.5), dict(max_hole=1, max_hole_share=float("nan")),
               dict(max_hole=1, min_component=0)):
        with pytest.raises(ValueError, match="scan_predictions: m(ax|in)_"):
            call(faces=faces, **kw)
    for bad in (faces.long(), faces[:, :2], faces[0]):
        with pytest.raises(ValueError):
            call(faces=bad, max_hole=1)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):         # every check passed: max_hole alone goes with faces
        call(faces=faces, max_hole=0)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        call(faces=faces, max_hole=3, min_component=2)


def test_the_tester_and_the_tool_check_the_parameters():
    from gspn_amd import _args
    assert _args._hole_parameters(0, 1, "x") == (0, 1.0) and _args._hole_parameters(np.int64(7), 0, "x") == (7, 0.0)
    for bad in ((-1, 1.0), (1.5, 1.0), (True, 1.0), (1, -0.1), (1, float("nan")), (1 << 31, 1.0)):
        with pytest.raises(ValueError, match="x: max_"):
            _args._hole_parameters(*bad, "x")
    spec = importlib.util.spec_from_file_location("tools_test", os.path.join(ROOT, "tools", "test.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.parse(["--synthetic", "2"]).holes is None and tool.parse(["--synthetic", "2"]).hole_share == 1.0
    a = tool.parse(["--synthetic", "2", "--synthetic_vertices", "20000", "--holes", "50", "--hole_share", "0.25"])
    assert a.holes == 50 and a.hole_share == 0.25 and a.components is None
    with pytest.raises(SystemExit, match="--holes goes with the vertex modes"):
        tool.main(["--synthetic", "2", "--holes", "5"])
    with pytest.raises(SystemExit, match="--hole_share goes with --holes"):
        tool.main(["--synthetic", "2", "--synthetic_vertices", "20000", "--hole_share", "0.5"])
    for extra in (["--holes", "-1"], ["--holes", "5", "--hole_share", "1.5"], ["--holes", "5", "--hole_share", "nan"]):
        with pytest.raises(SystemExit, match="--holes must not be negative"):
            tool.main(["--synthetic", "2", "--synthetic_vertices", "20000"] + extra)
    import inspect
    from gspn_amd.tester import Tester
    sig = inspect.signature(Tester.__init__).parameters
    assert sig["max_hole"].default is None and sig["max_hole_share"].default == 1.0
