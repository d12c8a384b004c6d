"""nearest_point (gspn_amd/nearest.py, csrc/nearest.hip) on poisoned, guard-banded allocations (tests/arena.py; the table's rules are those
of tests/test_gpu_arena_geometry.py).  Its workspace -- sorted points, plans, counters, starts, ranks -- comes from a patched torch.empty,
so a counter the call did not reset or a start the query read past the scan would show: one build workgroup and several, one scene and
two.  Integer atomics only: every row is held to equal bits, none is masked."""
import numpy as np
import pytest
import torch

from tests.arena import Case, sweep

pytestmark = pytest.mark.gpu

CASES = []


def case(fn):
    CASES.append(fn)
    return fn


@case
def nearest_point():
    from gspn_amd.nearest import nearest_point
    rng = np.random.default_rng(41)
    dev = lambda *shape: torch.from_numpy(rng.random(shape, dtype=np.float32)).cuda()                   # noqa: E731
    small = (dev(1, 1500, 3), dev(1, 1100, 3))                                        # two build workgroups, six query workgroups
    far = (dev(1, 300, 3), dev(1, 9000, 3))                                           # nine build workgroups
    two = (dev(2, 700, 3) * 3 - 1, dev(2, 2500, 3))                                   # two scenes, queries outside the box among them
    return Case("nearest_point 1500 <- 1100, 300 <- 9000 and 2 x 700 <- 2500", lambda: (nearest_point(*small), nearest_point(*far), nearest_point(*two)))


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
MASKED = set()          # names of the rows that carry a mask or a canonical form: none here


@pytest.mark.parametrize("build", CASES, ids=lambda f: f.__name__)
def test_arena(build):
    c = build()
    assert c.masked == (build.__name__ in MASKED)
    sweep(c)


def test_zz_masked_cases():
    print("\ntests/test_gpu_arena_nearest.py: %d cases, %d masked" % (len(CASES), len(MASKED)))
    assert not MASKED
