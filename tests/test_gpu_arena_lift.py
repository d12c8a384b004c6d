"""The lift to a scan's vertices (gspn_amd/lift.py, csrc/lift.hip) on poisoned, guard-banded allocations (tests/arena.py; the table's rules
are those of tests/test_gpu_arena_geometry.py): vertex_tables, gspn_lift_masks through its wrapper -- whose workspace comes from a patched
torch.empty, so every slot an early-leaving tile forgot would show -- and scan_predictions, at the smallest shapes that select each path:
one tile, several tiles with empty ones, dropped rows, both instantiations.  No float atomics: every row is held to equal bits, none is
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


@case
def vertex_tables():
    from gspn_amd.lift import vertex_tables
    rng = np.random.default_rng(31)
    verts, pc = rng.random((1500, 3), dtype=np.float32), rng.random((1100, 3), dtype=np.float32)
    seeds, fb = pc[:64].copy(), rng.random((64, 2), dtype=np.float32)
    big = [torch.from_numpy(a).cuda() for a in (verts, pc, seeds, fb)]                # the cell-grid search and the one-wave search
    far = [torch.from_numpy(a).cuda() for a in (verts[:300], rng.random((9000, 3), dtype=np.float32), seeds[:3], fb[:3])]      # the tiled search
    return Case("vertex_tables 1500 <- 1100 / 64 and 300 <- 9000 / 3", lambda: (vertex_tables(*big), vertex_tables(*far)))


@case
def lift_masks():
    from gspn_amd.lift import lift_masks
    from tests.test_gpu_lift import make_case, on_device, planted_case
    one = on_device(make_case(2, 200, 3, 7, 4, seed=1))                                # one tile, a full and an empty row
    planted = on_device(planted_case())                                              # three tiles, empty ones, rows of class 0 and C
    four = on_device(make_case(512, 1025, 5, 33, 6, seed=2))                          # four vertices per lane, a second tile of one vertex
    return Case("lift_masks (2, 200), the planted (8, 768) and (512, 1025): both instantiations, empty tiles, dropped rows",
                lambda: (lift_masks(**one), lift_masks(**planted), lift_masks(**four)))


@case
def scan_predictions():
    from gspn_amd import synth
    from gspn_amd.lift import scan_predictions
    from tests import predict_ref as PR
    pc, ep = PR.stage_inputs(2, 5, 300, 8, 19, seed=6, ladder=False)
    ep["detections"][1, 4, 6] = 0                                                    # a dropped row for certain
    verts = torch.from_numpy(synth.scan_vertices(pc[1].numpy(), np.zeros(300, np.int32), np.zeros(300, np.int32), 777, 4)[0]).cuda()
    pc, ep = pc.cuda(), {k: v.cuda() for k, v in ep.items()}
    return Case("scan_predictions scene 1 of (2, 5, 300, 8, 19) on 777 vertices", lambda: scan_predictions(ep, 1, verts, pc=pc))


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
MASKED = set()          # names of the rows that carry a mask or a canonical form: none here


@pytest.mark.parametrize("build", CASES, ids=lambda f: f.__name__)
def test_arena(build):
    c = build()
    assert c.masked == (build.__name__ in MASKED)
    sweep(c)


def test_zz_masked_cases():
    print("\ntests/test_gpu_arena_lift.py: %d cases, %d masked" % (len(CASES), len(MASKED)))
    assert not MASKED
