"""CPU tests of nearest_point (gspn_amd/nearest.py): the two symbols in the header, the library and the binding with the ABI
still 21; the host-side rules of the entry point, which launch nothing; the wrapper's argument rules, which raise before the library is
touched; vertex_tables' search keyword."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_nearest_symbols_are_declared_exported_and_bound_at_abi_21():
    from gspn_amd import _lib, build, nearest
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    assert "#define GSPN_ABI_VERSION 21" in text and int(lib.gspn_abi_version()) == 21 == _lib.ABI_VERSION
    assert "Additive at 21: gspn_nearest_point (+ gspn_nearest_point_ws_bytes)" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.search(r"\bint gspn_nearest_point\s*\(([^)]*)\)", code).group(1).split(",")
    assert len(declared) == len(_lib.SIGNATURES["gspn_nearest_point"]) == 9 and hasattr(ctypes.CDLL(_lib.LIB_PATH), "gspn_nearest_point")
    assert re.search(r"\blong gspn_nearest_point_ws_bytes\s*\(int b, int m\)", code)
    assert _lib.SPECIAL["gspn_nearest_point_ws_bytes"] == ([ctypes.c_int, ctypes.c_int], ctypes.c_long)
    assert int(re.search(r"#define GSPN_NEAREST_MAX_M \(1 << (\d+)\)", text).group(1)) == 24 and nearest.NEAREST_MAX_M == 1 << 24
    assert "nearest.hip" not in build.POLICY_SOURCES
    # host-side rules, nothing launched: sizes, null pointers, the limit
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    assert lib.gspn_nearest_point(-1, 1, 1, one, one, one, one, one, null) == -1 and lib.gspn_nearest_point(1, 1, -1, one, one, one, one, one, null) == -1
    assert lib.gspn_nearest_point(1, 1, 0, one, one, one, one, one, null) == -1                         # no known point for a query
    for k in range(5):
        assert lib.gspn_nearest_point(1, 1, 1, *[null if i == k else one for i in range(5)], null) == -1
    assert lib.gspn_nearest_point(1, 1, (1 << 24) + 1, one, one, one, one, one, null) == -2
    assert lib.gspn_nearest_point(0, 5, 5, null, null, null, null, null, null) == 0 and lib.gspn_nearest_point(5, 0, 0, null, null, null, null, null, null) == 0
    # the workspace: sorted points, a plan per scene, counters, starts, (cell, rank) per point; 0 for what the call declines
    cells = lambda m: min(max(m // 4, 1), 1 << 16)                                                       # noqa: E731
    for b, m in ((1, 1), (1, 3), (3, 257), (2, 18000), (1, 300000), (5, 1 << 24)):
        start = 16 * b * m + 128 * b + 4 * b * cells(m) + 4 * b * (cells(m) + 1)
        assert lib.gspn_nearest_point_ws_bytes(b, m) == (start + 7) // 8 * 8 + 8 * b * m
    assert lib.gspn_nearest_point_ws_bytes(0, 5) == 0 and lib.gspn_nearest_point_ws_bytes(5, 0) == 0 and lib.gspn_nearest_point_ws_bytes(1, (1 << 24) + 1) == 0


def test_nearest_point_raises_before_anything_runs(monkeypatch):
    from gspn_amd import _lib, nearest
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    q, known = torch.zeros(2, 10, 3), torch.zeros(2, 7, 3)
    for bad in ((q[0], known), (q, known[0]), (q[:, :, :2], known), (q, known[:, :, :2]), (q[:1], known), (q.double(), known), (q, known.int()),
                (q, known[:, :0])):
        with pytest.raises(ValueError):
            nearest.nearest_point(*bad)
    with pytest.raises(ValueError, match="no known points"):
        nearest.nearest_point(q, known[:, :0])
    with pytest.raises(TypeError):
        nearest.nearest_point(q.numpy(), known)
    for bad in (torch.zeros(4096), torch.zeros(8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            nearest.nearest_point(q, known, bad)
    huge = torch.zeros(1, 3).expand(1, (1 << 24) + 1, 3)                                                 # (a view: no memory behind it)
    with pytest.raises(NotImplementedError, match="m <= 16777216"):
        nearest.nearest_point(q[:1], huge)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):                       # well-formed, on the wrong device: no CPU fallback
        nearest.nearest_point(q, known)
    with pytest.raises(_lib.GspnHipError, match="is on cpu"):
        nearest.nearest_point(q, known, torch.zeros(1 << 16, dtype=torch.uint8))
    assert nearest.nearest_point.__doc__ and set(nearest.__all__) == {"NEAREST_MAX_M", "nearest_point"}


def test_vertex_tables_names_its_searches(monkeypatch):
    from gspn_amd import _lib, lift
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    verts, pc, seeds, fb = torch.zeros(10, 3), torch.zeros(7, 3), torch.zeros(6, 3), torch.zeros(6, 2)
    with pytest.raises(ValueError, match="search must be one of"):
        lift.vertex_tables(verts, pc, seeds, fb, search="brute")
    for search in (None, "three_nn", "nearest_point"):
        with pytest.raises(_lib.GspnHipError, match="is on cpu"):
            lift.vertex_tables(verts, pc, seeds, fb, search=search)
    assert lift.NEAREST_FROM_M >= 1024 and "NEAREST_FROM_M" in lift.__all__
