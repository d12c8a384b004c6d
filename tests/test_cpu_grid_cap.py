"""The gate behind tests/test_gpu_grid_cap.py, without a GPU: every kernel that csrc/*.hip launches through the capped grid of grid_for()
(csrc/common.h) -- and the two launchers that cap a grid of their own -- has an entry in that module's COVERED table, every case's shape still
takes its launch through one full and one ragged trip under the cap of THIS build (gspn_grid_blocks), and gspn_grid_blocks is what the
header says.  A new grid_for launch site fails here until it has a case."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gspn_amd", "csrc")

# hipLaunchKernelGGL(name or name<...>, dim3(<grid>), dim3(   and   name<<<<grid>, ...
GGL = re.compile(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*)\s*(?:<[^;()]*?>)?\s*\)?\s*,\s*dim3\((.*?)\),\s*dim3\(", re.S)
CHEVRON = re.compile(r"([A-Za-z_]\w*)\s*(?:<[^;<>()]*>)?\s*<<<\s*(.*?),", re.S)
OWN_GRID = {"multi_copy_kernel": ("grouping.hip", r"multi_copy_kernel, dim3\(\(unsigned\)\(np < (\d+) \? np : \1\)\)"),
            "prefix_rows_kernel": ("sampling.hip", r"prefix_rows_kernel, dim3\(b < (\d+) \? b : \1\)")}


def capped_launches():
    """-> {kernel: [file, ...]} of every launch whose grid expression calls grid_for, and the number of grid_for( calls in the sources"""
    found, calls = {}, 0
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as fh:
            text = fh.read()
        calls += text.count("grid_for(") - text.count("return (long)grid_for(total, block);")      # (gspn_grid_blocks itself launches nothing)
        for rx in (GGL, CHEVRON):
            for m in rx.finditer(text):
                if "grid_for(" in m.group(2):
                    found.setdefault(m.group(1), []).append(os.path.basename(path))
    return found, calls


def test_every_capped_launch_site_has_a_case_or_a_computed_size():
    from tests.test_gpu_grid_cap import COVERED
    found, calls = capped_launches()
    assert sum(len(v) for v in found.values()) == calls, "a grid_for( call in csrc/*.hip is not inside a launch this scan recognises: teach it the new form"
    assert len(found) >= 40
    kernels = set(found)
    for name, (source, pattern) in OWN_GRID.items():
        with open(os.path.join(CSRC, source)) as fh:
            assert re.search(pattern, fh.read()), "%s no longer caps its own grid this way (csrc/%s)" % (name, source)
        kernels.add(name)
    missing, stale = sorted(kernels - set(COVERED)), sorted(set(COVERED) - kernels)
    assert not missing, "launched through a capped grid without a case in tests/test_gpu_grid_cap.py: %s (%s)" % (
        missing, {k: found.get(k) for k in missing})
    assert not stale, "in COVERED but no longer launched through a capped grid: %s" % stale


def test_the_table_names_tests_that_exist():
    import tests.test_gpu_grid_cap as G
    for kernel, where in G.COVERED.items():
        names = re.findall(r"(?:(test_\w+)\.py::)?(test_\w+)", where)
        assert names, (kernel, where)
        for module, test in names:
            if module:
                with open(os.path.join(ROOT, "tests", module + ".py")) as fh:
                    assert re.search(r"^def %s\(" % test, fh.read(), re.M), (kernel, module, test)
            else:
                assert callable(getattr(G, test, None)), (kernel, test)


def test_grid_blocks_is_declared_bound_and_is_the_capped_grid():
    from gspn_amd import _lib
    lib = _lib.lib()
    with open(os.path.join(ROOT, "include", "gspn_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"^long gspn_grid_blocks\(long total, int block\);", header, re.M) and "#define GSPN_ABI_VERSION 21" in header
    assert "gspn_grid_blocks" in _lib.SPECIAL and _lib.ABI_VERSION == 21 == int(lib.gspn_abi_version())
    g = lib.gspn_grid_blocks
    assert g(-1, 256) == -1 and g(10, 0) == -1 and g(10, -4) == -1
    assert g(0, 256) == 1 and g(1, 256) == 1 and g(256, 256) == 1 and g(257, 256) == 2 and g(1000, 64) == 16
    with open(os.path.join(CSRC, "common.h")) as fh:
        cap = re.search(r"const long cap = (\d+)L \* (\d+);\s*\n\s*return \(unsigned\)\(g < 1 \? 1 : \(g > cap \? cap : g\)\);", fh.read())
    assert cap, "grid_for() of csrc/common.h has changed its form: check gspn_grid_blocks against it by hand, then this pattern"
    cap = int(cap.group(1)) * int(cap.group(2))
    for block in (64, 256, 1024):
        assert g(cap * block, block) == cap == g(cap * block + 1, block) == g(1 << 40, block) and g(cap * block - block, block) == cap - 1


def test_every_case_still_runs_one_full_and_one_ragged_trip():
    from gspn_amd import _lib
    from tests.test_gpu_grid_cap import SHAPES
    lib = _lib.lib()
    for case, (total, block) in SHAPES.items():
        grid = int(lib.gspn_grid_blocks(total, block))
        assert grid * block < total < 2 * grid * block and total % block != 0, (case, total, block, grid)
