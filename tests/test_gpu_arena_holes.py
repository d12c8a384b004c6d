"""hole_fill (gspn_amd/holes.py, csrc/components.hip) on poisoned, guard-banded allocations (tests/arena.py; the table's rules are those of
tests/test_gpu_arena_geometry.py).  Its workspace -- the two bit tables, the size counters with their flags, the marks, the box keys, the
set counts and the parents -- and its outputs come from a patched torch.empty, so a counter the call did not reset or a word it read
without writing would show; the sizes are odd, so the rows start at every alignment and an aligned vector that reached past a row's end,
or a walk that left its row, would land in a guard band.  Integer atomics only: every row is held to equal bits, none is masked."""
import numpy as np
import pytest
import torch

from tests.arena import Case, sweep
from tests.test_gpu_holes import make_rows, make_scene

pytestmark = pytest.mark.gpu

CASES = []


def case(fn):
    CASES.append(fn)
    return fn


def scene_of(rng, r, v):
    """tests/test_gpu_holes.py's lattice with its frames, gaps, U shapes and loose fragments -> masks, faces, xyz on the device"""
    xyz, faces, at = make_scene(rng, v)
    return torch.from_numpy(make_rows(rng, r, v, at)).cuda(), torch.from_numpy(faces).cuda(), torch.from_numpy(xyz).cuda()


@case
def hole_fill():
    from gspn_amd.holes import hole_fill
    rng = np.random.default_rng(49)
    small = scene_of(rng, 3, 257)                                     # one word, ragged vectors at both ends
    wide = scene_of(rng, 67, 4099)                                    # two words of the tables
    tiny = scene_of(rng, 33, 1)                                       # one vertex: every row one byte from the next
    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    return Case("hole_fill 3 x 257, 67 x 4099 with labels, 33 x 1 and without faces",
                lambda: (hole_fill(*small, max_vertices=40), hole_fill(*wide, max_vertices=12, max_share=0.5, label=True),
                         hole_fill(*tiny, max_vertices=1), hole_fill(small[0], none, small[2], max_vertices=40, label=True)))


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
MASKED = set()          # names of the rows that carry a mask or a canonical form: none here


@pytest.mark.parametrize("build", CASES, ids=lambda f: f.__name__)
def test_arena(build):
    c = build()
    assert c.masked == (build.__name__ in MASKED)
    sweep(c)


def test_zz_masked_cases():
    print("\ntests/test_gpu_arena_holes.py: %d cases, %d masked" % (len(CASES), len(MASKED)))
    assert not MASKED
