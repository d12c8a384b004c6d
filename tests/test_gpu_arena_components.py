"""mask_components and component_filter (gspn_amd/components.py, csrc/components.hip) on poisoned, guard-banded allocations
(tests/arena.py; the table's rules are those of tests/test_gpu_arena_geometry.py).  Their workspaces -- the bit table, the size counters,
the marks, the filter's parents and maxima -- and their outputs come from a patched torch.empty, so a counter the call did not reset or a
word it read without writing would show; the sizes are odd, so the rows start at every alignment and an aligned vector that reached past
a row's end, or a walk that left its row, would land in a guard band.  Integer atomics only: every row is held to equal bits, none is
masked."""
import numpy as np
import pytest
import torch

from tests.arena import Case, sweep

pytestmark = pytest.mark.gpu

CASES = []


def case(fn):
    CASES.append(fn)
    return fn


def bytes_of(rng, r, v):
    """set bytes of 1, 2 and 255 at mixed densities, the last row all set, row 0 empty"""
    on = rng.random((r, v)) < rng.choice([0.2, 0.6, 0.9], size=(r, 1))
    m = (np.array([1, 2, 255], np.uint8)[rng.integers(0, 3, size=(r, v))] * on).astype(np.uint8)
    m[-1] = 7
    m[0] = 0
    return torch.from_numpy(m).cuda()


def faces_of(rng, v):
    """a strip over a shuffled order, long-range faces, and ends outside [0, v)"""
    o = rng.permutation(v)
    f = [np.stack((o[:-2], o[1:-1], o[2:]), axis=1)] if v > 2 else []
    f += [rng.integers(0, v, size=(v // 3 + 2, 3)), rng.integers(-5, v + 5, size=(9, 3)), np.array([[-(1 << 31), 0, (1 << 31) - 1]])]
    return torch.from_numpy(np.concatenate(f).astype(np.int32)).cuda()


@case
def mask_components():
    from gspn_amd.components import mask_components
    rng = np.random.default_rng(47)
    small, fs = bytes_of(rng, 3, 257), faces_of(rng, 257)             # one word, ragged vectors at both ends
    wide, fw = bytes_of(rng, 67, 4099), faces_of(rng, 4099)           # two words of the table
    tiny, ft = bytes_of(rng, 33, 1), faces_of(rng, 1)                 # one vertex: every row one byte from the next
    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    return Case("mask_components 3 x 257, 67 x 4099, 33 x 1 and without faces",
                lambda: (mask_components(small, fs), mask_components(wide, fw), mask_components(tiny, ft), mask_components(small, none)))


@case
def component_filter():
    from gspn_amd.components import component_filter
    rng = np.random.default_rng(48)
    small, fs = bytes_of(rng, 3, 257), faces_of(rng, 257)
    wide, fw = bytes_of(rng, 67, 4099), faces_of(rng, 4099)
    tiny, ft = bytes_of(rng, 33, 1), faces_of(rng, 1)
    return Case("component_filter 3 x 257, 67 x 4099 and 33 x 1",
                lambda: (component_filter(small, fs, min_vertices=2), component_filter(wide, fw, min_vertices=3, min_share=0.5),
                         component_filter(tiny, ft, min_vertices=1, min_share=1.0)))


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
MASKED = set()          # names of the rows that carry a mask or a canonical form: none here


@pytest.mark.parametrize("build", CASES, ids=lambda f: f.__name__)
def test_arena(build):
    c = build()
    assert c.masked == (build.__name__ in MASKED)
    sweep(c)


def test_zz_masked_cases():
    print("\ntests/test_gpu_arena_components.py: %d cases, %d masked" % (len(CASES), len(MASKED)))
    assert not MASKED
