"""segment_vote and segment_label_vote (gspn_amd/segments.py, csrc/segments.hip) on poisoned, guard-banded allocations (tests/arena.py; the
table's rules are those of tests/test_gpu_arena_geometry.py).  Their workspaces -- counters, decision words, winners -- come from a patched
torch.empty, so a counter the call did not reset or a decision word it read without writing would show, and every case carries segment
ids outside [0, S): an id that indexed a counter would land in a guard band or change the bits.  Integer atomics only: every row is held
to equal bits, none is masked."""
import numpy as np
import pytest
import torch

from tests.arena import Case, sweep

pytestmark = pytest.mark.gpu

CASES = []


def case(fn):
    CASES.append(fn)
    return fn


def ids(rng, v, s):
    """segment ids with every kind of outsider mixed in"""
    seg = rng.integers(0, s, size=v).astype(np.int64)
    odd = rng.random(v) < 0.15
    seg[odd] = np.array([-1, -5, s, s + 1, 2 ** 31 - 1])[rng.integers(0, 5, size=int(odd.sum()))]
    return torch.from_numpy(seg.astype(np.int32)).cuda()


@case
def segment_vote():
    from gspn_amd.segments import segment_vote
    rng = np.random.default_rng(43)
    bytes_of = lambda r, v: torch.from_numpy((np.array([1, 2, 255], np.uint8)[rng.integers(0, 3, size=(r, v))]                    # noqa: E731
                                              * (rng.random((r, v)) < 0.4)).astype(np.uint8)).cuda()
    small = (bytes_of(3, 257), ids(rng, 257, 7), 7)                                   # one workgroup of every pass, ragged vectors at both ends
    wide = (bytes_of(11, 4099), ids(rng, 4099, 300), 300)                             # five apply tiles, two row groups, five decision words a row
    single = (bytes_of(2, 1500), ids(rng, 1500, 1), 1)                                # every vote on one counter
    return Case("segment_vote 3 x 257 / 7, 11 x 4099 / 300 and 2 x 1500 / 1",
                lambda: (segment_vote(*small), segment_vote(*wide, 0.25), segment_vote(*single, 0.0)))


@case
def segment_label_vote():
    from gspn_amd.segments import segment_label_vote
    rng = np.random.default_rng(44)
    labels = lambda v, c: torch.from_numpy(rng.integers(-1, c + 1, size=v).astype(np.int32)).cuda()                               # noqa: E731
    small = (labels(257, 19), ids(rng, 257, 7), 7, 19)
    wide = (labels(4099, 64), ids(rng, 4099, 300), 300, 64)
    one = (labels(1500, 1), ids(rng, 1500, 2), 2, 1)
    return Case("segment_label_vote 257 / 7 / 19, 4099 / 300 / 64 and 1500 / 2 / 1",
                lambda: (segment_label_vote(*small), segment_label_vote(*wide), segment_label_vote(*one)))


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
MASKED = set()          # names of the rows that carry a mask or a canonical form: none here


@pytest.mark.parametrize("build", CASES, ids=lambda f: f.__name__)
def test_arena(build):
    c = build()
    assert c.masked == (build.__name__ in MASKED)
    sweep(c)


def test_zz_masked_cases():
    print("\ntests/test_gpu_arena_segments.py: %d cases, %d masked" % (len(CASES), len(MASKED)))
    assert not MASKED
