"""mask_overlaps and mask_nms (gspn_amd/mask_nms.py, csrc/mask_nms.hip) on poisoned, guard-banded allocations (tests/arena.py; the table's
rules are those of tests/test_gpu_arena_geometry.py).  Their workspaces -- the packed words, the sizes, the overlap matrix -- come from a
patched torch.empty, so a counter the call did not reset or a word it read without writing would show; the sizes are odd, so the rows
start at every alignment and an aligned vector that reached past a row's end would land in a guard band.  Integer atomics only: every row
is held to equal bits, none is masked."""
import numpy as np
import pytest
import torch

from tests.arena import Case, sweep

pytestmark = pytest.mark.gpu

CASES = []


def case(fn):
    CASES.append(fn)
    return fn


def bytes_of(rng, *shape):
    """overlapping rows: subsets of two parents, set bytes of 1, 2 and 255, the last row all set, one row empty"""
    parents = rng.random((2, shape[-1])) < 0.6
    pick = parents[rng.integers(0, 2, size=shape[:-1])]
    m = (np.array([1, 2, 255], np.uint8)[rng.integers(0, 3, size=shape)] * (pick & (rng.random(shape) < 0.8))).astype(np.uint8)
    m[..., -1, :] = 7
    m[..., 0, :] = 0
    return torch.from_numpy(m).cuda()


@case
def mask_overlaps():
    from gspn_amd.mask_nms import mask_overlaps
    rng = np.random.default_rng(45)
    small = bytes_of(rng, 3, 257)                                     # one pack block, one tile, ragged vectors at both ends
    wide = bytes_of(rng, 2, 35, 4099)                                 # two scenes, two tiles (three pairs), two pack blocks, two word chunks
    tiny = bytes_of(rng, 33, 1)                                       # one vertex: every row one byte from the next
    return Case("mask_overlaps 3 x 257, 2 x 35 x 4099 and 33 x 1", lambda: (mask_overlaps(small), mask_overlaps(wide), mask_overlaps(tiny)))


@case
def mask_nms():
    from gspn_amd.mask_nms import mask_nms
    rng = np.random.default_rng(46)
    small = bytes_of(rng, 3, 257)
    wide = bytes_of(rng, 2, 35, 4099)
    count = torch.tensor([20, 99], dtype=torch.int32, device="cuda")
    labels = torch.from_numpy(rng.integers(0, 3, size=(2, 35)).astype(np.int32)).cuda()
    tiny = bytes_of(rng, 33, 1)
    return Case("mask_nms 3 x 257, 2 x 35 x 4099 with counts and labels, and 33 x 1",
                lambda: (mask_nms(small, iou_th=0.5), mask_nms(wide, count, labels, iou_th=0.3), mask_nms(tiny, iou_th=0.0)))


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
MASKED = set()          # names of the rows that carry a mask or a canonical form: none here


@pytest.mark.parametrize("build", CASES, ids=lambda f: f.__name__)
def test_arena(build):
    c = build()
    assert c.masked == (build.__name__ in MASKED)
    sweep(c)


def test_zz_masked_cases():
    print("\ntests/test_gpu_arena_mask_nms.py: %d cases, %d masked" % (len(CASES), len(MASKED)))
    assert not MASKED
