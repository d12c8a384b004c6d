"""CPU tests of the lift to a scan's vertices (gspn_amd/lift.py): the two symbols in the header, the library and the
binding with the ABI still 21; the two restatements of tests/lift_ref.py against each other; the pin -- on the scenes of
tests/golden/predict/export_ref.npz, with the vertices the scene's own points, the restatement reproduces what the reference's own lines
recorded, and the one new rule (src) is the identity there --; the wrappers' argument rules, which raise before the library is touched;
and the synthetic scan generator of tools/test.py --synthetic_vertices."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import lift_ref as LR
from tests import predict_ref as PR
from tests.test_cpu_reference_pins import export_scene, fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_lift_symbols_are_declared_exported_and_bound_at_abi_21():
    from gspn_amd import _lib, build
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    assert "#define GSPN_ABI_VERSION 21" in text and int(lib.gspn_abi_version()) == 21 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.search(r"\bint gspn_lift_masks\s*\(([^)]*)\)", code).group(1).split(",")
    assert len(declared) == len(_lib.SIGNATURES["gspn_lift_masks"]) == 20 and hasattr(ctypes.CDLL(_lib.LIB_PATH), "gspn_lift_masks")
    assert [i for i, a in enumerate(declared) if a.strip().startswith("double ")] == \
        [i for i, a in enumerate(_lib.SIGNATURES["gspn_lift_masks"]) if a is ctypes.c_double] == [13]      # mask_th crosses as a double
    assert re.search(r"\blong gspn_lift_part_doubles\s*\(int r, int v\)", code)
    assert _lib.SPECIAL["gspn_lift_part_doubles"] == ([ctypes.c_int, ctypes.c_int], ctypes.c_long)
    from gspn_amd.build import POLICY_SOURCES
    assert "lift.hip" not in POLICY_SOURCES
    # host-side rules, nothing launched: sizes, null pointers, the three limits, and the workspace size
    null = ctypes.c_void_p(0)
    args = [null] * 8 + [ctypes.c_double(0.4)] + [null] * 6
    assert lib.gspn_lift_masks(1, 1, 1, 1, 2, *args) == -1 and lib.gspn_lift_masks(0, 1, 1, 1, 2, *args) == -1
    from gspn_amd import lift
    assert (lift.LIFT_MAX_P, lift.LIFT_MAX_V) == (4096, 1 << 24)
    for r, v in ((1, 1), (1, 255), (1, 256), (1, 257), (3, 4099), (5, 32769), (511, 1024), (512, 1024), (512, 1025), (1024, (1 << 21) + 3), (100, 500000)):
        tile = lift.lift_tile(r, v)
        assert tile == (1024 if r * ((v + 1023) // 1024) >= 512 else 256)
        assert lib.gspn_lift_part_doubles(r, v) == 4 * r * ((v + tile - 1) // tile)
    assert lift.lift_tile(511, 1024) == 256 and lift.lift_tile(512, 1024) == 1024
    assert lib.gspn_lift_part_doubles(0, 5) == 0 and lib.gspn_lift_part_doubles(5, (1 << 24) + 1) == 0 and lib.gspn_lift_part_doubles(65536, 5) == 0


# ---- the restatements against each other -----------------------------------------------------------------------------------------------------

def scan_of(pc, v, seed):
    """the scene's points followed by jittered copies of some: a scan the scene is a subset of"""
    from gspn_amd import synth
    n = pc.shape[0]
    return synth.scan_vertices(pc, np.zeros(n, np.int32), np.zeros(n, np.int32), v, seed, jitter=0.02)[0]


def test_the_two_restatements_agree():
    b, r, n, p, c = 1, 9, 500, 16, 19
    pc, ep = PR.stage_inputs(b, r, n, p, c, seed=5, ladder=False)
    pc, ep = pc.numpy()[0], {k: t.numpy()[0] for k, t in ep.items()}
    verts = scan_of(pc, 2 * n + 7, 3)
    det, masks, crops = ep["detections"], ep["rpointnet_mask_selected"], ep["pc_coord_cropped_final_unnormalized"]
    cls = det[:, 6].astype(np.int32)
    sem_prob = PR.point_tables(pc, ep["sem_class_logits"], ep["pc_seed"], ep["fb_prob"])[0]
    src, vert_fb = LR.vertex_tables(verts, pc, ep["pc_seed"], ep["fb_prob"])
    assert np.array_equal(src[:n], np.arange(n)) and (src[n:] != np.arange(n, len(verts))).all() and src.max() < n
    boxes = np.ascontiguousarray(det[:, :6])
    sem_conf, fb_conf, mask, points = LR.lift(verts, crops, boxes, masks, cls, src, sem_prob, vert_fb)
    rows, lit_sem, lit_fb, lit_mask = LR.literal(verts, crops, boxes, masks, cls, src, sem_prob, vert_fb)
    v = len(verts)
    assert np.array_equal(rows, np.where(cls > 0)[0]) and (cls == 0).any() and len(rows) >= 4
    assert np.array_equal(lit_mask, mask[rows]) and lit_mask.dtype == np.int32 and np.array_equal(points, mask.sum(-1))
    assert PR.within_bound(lit_sem, sem_conf[rows], v) and PR.within_bound(lit_fb, fb_conf[rows], v)
    assert (points[rows] > 0).sum() >= 3 and points[1] == 0 and sem_conf[1] == 0 and fb_conf[1] == 0    # the empty row: 0 / 1e-8
    dead = cls <= 0
    assert not sem_conf[dead].any() and not fb_conf[dead].any() and not mask[dead].any()
    # restricted to the scene's own points the values are the scene stage's
    idx = PR.DR.nearest_in_sets(torch.from_numpy(pc)[None], torch.from_numpy(crops)[None], torch.from_numpy(boxes)[None])[0].numpy()
    g = LR.values(verts, crops, boxes, masks)
    assert np.array_equal(g[:, :n], np.where(idx >= 0, np.take_along_axis(masks, np.maximum(idx, 0), 1), np.float32(0)))
    # a src value outside [0, N) is clamped, a class outside [1, C) is dropped
    wild = src.copy()
    wild[::7], wild[3::7] = -1, n
    clamped = np.clip(wild, 0, n - 1)
    for a, w in zip(LR.lift(verts, crops, boxes, masks, cls, wild, sem_prob, vert_fb), LR.lift(verts, crops, boxes, masks, cls, clamped, sem_prob, vert_fb)):
        assert np.array_equal(a, w)
    high = cls.copy()
    high[0] = c
    out = LR.lift(verts, crops, boxes, masks, high, src, sem_prob, vert_fb)
    assert out[0][0] == 0 and out[1][0] == 0 and not out[2][0].any() and out[3][0] == 0 and np.array_equal(out[2][1:], mask[1:])


def test_box_test_and_first_minimum_of_the_restatement():
    box = np.array([0.5, 0.5, 0.5, 0.25, 0.5, 1.0], np.float32)
    verts = np.array([[0.375, 0.25, 0.0], [0.625, 0.75, 1.0], [0.3749999, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, 0.5, 0.5]], np.float32)
    assert LR.inside(verts, box).tolist() == [True, True, False, False, True]                           # faces included, NaN inside nothing
    pts = np.array([[1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    assert LR.nearest(np.zeros((1, 3), np.float32), pts).tolist() == [0]                                # four at distance 1: the first
    assert LR.nearest(np.array([[0, 0.9, 0]], np.float32), pts).tolist() == [1]                         # duplicated points: the first
    # the threaded search is the same function: a raster, where equal distances are the rule
    rng = np.random.default_rng(1)
    q = (rng.integers(0, 8, (3000, 3)) / 8).astype(np.float32)
    known = (rng.integers(0, 8, (700, 3)) / 8).astype(np.float32)
    a, b = LR.nearest(q, known), LR.nearest_threads(q, known, chunk=512)
    assert np.array_equal(a, b) and a.dtype == b.dtype == np.int32
    d = ((q[:, None] - known[None]) ** 2).sum(-1)
    assert ((d == d.min(1, keepdims=True)).sum(1) > 1).mean() > 0.5 and np.array_equal(a, d.argmin(1))


# ---- the pin -----------------------------------------------------------------------------------------------------------------------------------

def test_restatement_on_the_scene_s_own_points_equals_the_reference():
    """tests/golden/predict/export_ref.npz holds what the reference's own lines (test.py:155-205, with its ball tree) gave.  With the
    vertices the scene's points, src must be the identity and everything pinned about scene_predictions pins the lift at V = N."""
    fx = fixture("export")
    assert len(fx["scenes"]) >= 4
    for name in fx["scenes"].tolist():
        pc, arrays, want = export_scene(fx, name)
        masks, crops, det, logits, seeds, fb_prob = arrays
        n, nd = pc.shape[0], len(want["rows"])
        got = LR.scan_prediction(pc, pc, masks, crops, det, logits, seeds, fb_prob)
        assert np.array_equal(got["src"], np.arange(n)), name                                           # the one new rule: the identity here
        cls = det[:, 6].astype(np.int32)
        assert got["count"] == nd and np.array_equal(got["order"][:nd], want["rows"]) and np.array_equal(got["order"][nd:], np.where(cls <= 0)[0])
        assert np.array_equal(got["label_ids"][:nd], want["seg_label_pred"]), name
        assert np.array_equal(got["confidence"][:nd], want["confidence_pred"].astype(np.float32)), name
        assert np.array_equal(got["masks"][:nd], want["group_label_pred"]) and np.array_equal(got["mask_points"], got["masks"].sum(-1)), name
        assert PR.within_bound(got["sem_conf"][:nd], want["sem_conf"], n) and PR.within_bound(got["fb_conf"][:nd], want["fb_conf"], n)
        # and exactly as predict_ref does: the same bits as its exact sums
        idx = PR.DR.nearest_in_sets(torch.from_numpy(pc.copy())[None], torch.from_numpy(crops.copy())[None], torch.from_numpy(det[:, :6].copy())[None]).numpy()
        sem_prob, fb = PR.point_tables(pc, logits, seeds, fb_prob)
        sc, fc, mask, points = PR.confidence_fsum(idx, masks[None], cls[None], sem_prob[None], fb[None])
        at = got["order"]
        assert np.array_equal(got["sem_conf"], sc[0][at]) and np.array_equal(got["fb_conf"], fc[0][at])
        assert np.array_equal(got["masks"], mask[0][at]) and np.array_equal(got["mask_points"], points[0][at])
        if nd:
            rows, lit_sem, lit_fb, lit_mask = LR.literal(pc, crops, np.ascontiguousarray(det[:, :6]), masks, cls, got["src"], sem_prob, fb)
            back = {int(k): j for j, k in enumerate(rows)}
            pick = [back[int(k)] for k in want["rows"]]
            assert np.array_equal(lit_mask[pick], want["group_label_pred"]) and PR.within_bound(lit_sem[pick], want["sem_conf"], n)


# ---- the wrappers' rules -------------------------------------------------------------------------------------------------------------------

def stage(b=2, r=3, n=40, p=4, c=19):
    pc, ep = PR.stage_inputs(b, r, n, p, c, seed=9, ladder=False)
    return pc, ep


def test_scan_predictions_raises_before_anything_runs(monkeypatch):
    from gspn_amd import _lib, lift
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    pc, ep = stage()
    verts = pc[0].clone()
    call = lambda ep_=ep, s=0, v=verts, **kw: lift.scan_predictions(ep_, s, v, **dict(dict(pc=pc), **kw))          # noqa: E731
    for k in ep:
        with pytest.raises(ValueError, match="end_points has no %r" % k):
            call({q: t for q, t in ep.items() if q != k})
    with pytest.raises(ValueError, match="pass pc"):
        lift.scan_predictions(ep, 0, verts)
    for bad in (verts.double(), verts[None], verts[:, :2], torch.zeros(0, 3)):
        with pytest.raises(ValueError):
            call(v=bad)
    with pytest.raises(TypeError):
        call(v=verts.numpy())
    for k, bad in (("detections", ep["detections"][:, :, :7]), ("rpointnet_mask_selected", ep["rpointnet_mask_selected"][:1]),
                   ("pc_coord_cropped_final_unnormalized", ep["pc_coord_cropped_final_unnormalized"][:, :, :3]),
                   ("sem_class_logits", ep["sem_class_logits"][:, :39]), ("fb_prob", ep["fb_prob"][:, :5]),
                   ("pc_seed", ep["pc_seed"].double()), ("detections", ep["detections"].int())):
        with pytest.raises(ValueError):
            call(dict(ep, **{k: bad}))
    for s in (-1, 2):
        with pytest.raises(ValueError, match="scene must lie in"):
            call(s=s)
    with pytest.raises(ValueError, match="label_map must have one entry per class, 19, got 18"):
        call(label_map=lift.SCANNET_LABEL_MAP[:18])
    for kw in (dict(mask_th=float("nan")), dict(sem_conf_th=float("nan")), dict(fb_conf_th=float("nan"))):
        with pytest.raises(ValueError, match="threshold is NaN"):
            call(**kw)
    big_pc, big = stage(1, 1025, 8, 2)
    with pytest.raises(NotImplementedError, match="R <= 1024"):
        lift.scan_predictions(big, 0, big_pc[0], pc=big_pc)
    monkeypatch.undo()
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):                       # well-formed, on the wrong device: no CPU fallback
        call()
    assert lift.scan_predictions.__doc__ and "end_points['pc']" in lift.scan_predictions.__doc__
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        lift.scan_predictions(dict(ep, pc=pc), 1, verts)                            # pc as a key of end_points


def test_vertex_tables_and_lift_masks_raise_before_anything_runs(monkeypatch):
    from gspn_amd import _lib, lift
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    v, r, p, n, c = 10, 3, 4, 7, 5
    verts, pc, seeds, fb = torch.zeros(v, 3), torch.zeros(n, 3), torch.zeros(6, 3), torch.zeros(6, 2)
    for bad in ((verts[:, :2], pc, seeds, fb), (verts, pc[None], seeds, fb), (verts, pc, seeds, fb[:5]), (verts, pc, seeds.double(), fb),
                (verts[:0], pc, seeds, fb), (verts, pc, seeds, fb[:, :1])):
        with pytest.raises(ValueError):
            lift.vertex_tables(*bad)
    good = dict(verts=verts, crops=torch.zeros(r, p, 3), boxes=torch.ones(r, 6), masks=torch.zeros(r, p), class_ids=torch.ones(r, dtype=torch.int32),
                src=torch.zeros(v, dtype=torch.int32), sem_prob=torch.zeros(n, c), vert_fb=torch.zeros(v))
    for k, bad in (("verts", verts[:, :2]), ("crops", torch.zeros(r, p + 1, 3)), ("boxes", torch.ones(r, 5)), ("class_ids", torch.ones(r + 1, dtype=torch.int32)),
                   ("class_ids", torch.ones(r)), ("src", torch.zeros(v - 1, dtype=torch.int32)), ("src", torch.zeros(v, dtype=torch.int64)),
                   ("vert_fb", torch.zeros(v + 1)), ("sem_prob", torch.zeros(n, c, 1)), ("masks", torch.zeros(r, p).double())):
        with pytest.raises(ValueError):
            lift.lift_masks(**dict(good, **{k: bad}))
    with pytest.raises(ValueError, match="mask_th is NaN"):
        lift.lift_masks(**good, mask_th=float("nan"))
    with pytest.raises(NotImplementedError, match="P <= 4096"):
        lift.lift_masks(**dict(good, crops=torch.zeros(r, 4097, 3), masks=torch.zeros(r, 4097)))
    monkeypatch.undo()
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        lift.vertex_tables(verts, pc, seeds, fb)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        lift.lift_masks(**good)


# ---- the synthetic scans of tools/test.py ---------------------------------------------------------------------------------------------------

def _tool():
    spec = importlib.util.spec_from_file_location("tools_test", os.path.join(ROOT, "tools", "test.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_synthetic_vertices_hold_the_scene_and_inherit_its_labels():
    T = _tool()
    a = T.parse(["--synthetic", "2", "--num_point", "300", "--num_point_ins", "16", "--num_category", "5", "--num_group", "4", "--seed", "3",
                 "--synthetic_vertices", "701"])
    assert (a.synthetic_vertices, a.mesh_path, a.label_path) == (701, None, None)
    assert T.parse([]).synthetic_vertices == 0
    b = T.parse(["--mesh_path", "mesh/scans", "--label_path", "label/scans"])
    assert (b.mesh_path, b.label_path) == ("mesh/scans", "label/scans")
    cache = T.synthetic_cache(a)
    vertices = T.synthetic_vertices(cache, a.synthetic_vertices, a.seed)
    for k in range(2):
        scan, again = vertices(k), vertices(k)
        n = a.num_point
        assert scan["xyz"].shape == (701, 3) and scan["xyz"].dtype == np.float32
        assert scan["seg_label"].shape == scan["group_label"].shape == (701,) and scan["seg_label"].dtype == scan["group_label"].dtype == np.int32
        assert all(np.array_equal(scan[q], again[q]) for q in scan)                 # seeded
        pc = cache["pc"][k].numpy()
        assert np.array_equal(scan["xyz"][:n], pc)                                  # the scene is a subset of its scan
        assert np.array_equal(scan["seg_label"][:n], cache["seg_label"][k].numpy()) and np.array_equal(scan["group_label"][:n], cache["group_label"][k].numpy())
        # every added vertex lies by a scene point and has that point's labels
        near = LR.nearest(scan["xyz"][n:], pc)
        assert np.abs(scan["xyz"][n:] - pc[near]).max() < 0.1 and not np.array_equal(scan["xyz"][n:], pc[near])
        labels = {(int(s), int(g)) for s, g in zip(cache["seg_label"][k].tolist(), cache["group_label"][k].tolist())}
        assert {(int(s), int(g)) for s, g in zip(scan["seg_label"][n:], scan["group_label"][n:])} <= labels
    assert not np.array_equal(vertices(0)["xyz"][300:], vertices(1)["xyz"][300:])
    from gspn_amd import synth
    with pytest.raises(ValueError):
        synth.scan_vertices(np.zeros((5, 3), np.float32), np.zeros(5), np.zeros(5), 4, 0)


@pytest.mark.parametrize("argv,text", [
    (["--synthetic", "2", "--mesh_path", "m", "--synthetic_vertices", "20000"], "at most one of --mesh_path DIR and --synthetic_vertices V"),
    (["--synthetic", "2", "--mesh_path", "m"], "--mesh_path needs --list FILE"),
    (["--synthetic", "2", "--label_path", "l"], "--label_path goes with --mesh_path"),
    (["--cache", "val.pt", "--synthetic_vertices", "20000"], "--synthetic_vertices V goes with --synthetic S"),
    (["--synthetic", "2", "--synthetic_vertices", "100"], "--synthetic_vertices V goes with --synthetic S and V >= --num_point"),
])
def test_the_vertex_flags_exclude_each_other(argv, text):
    with pytest.raises(SystemExit) as e:
        _tool().main(argv)
    assert text in str(e.value)
