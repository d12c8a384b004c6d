"""CPU checks of the shape_proposal_net trunks (gspn_amd/spn_trunks.py): the spec tables against the reference's literals, the FPS prefix
property that lets one level-1 FPS serve the seed / sem samples, and the level maps that three_nn_nested takes."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import data as D


def test_spec_tables_match_the_reference():
    from gspn_amd import spn_trunks as S
    # model_rpointnet.py:103-106 / :170-173 (SA) and :109-112 / :183-186 (FP), identical in shift_pred_net and sem_net
    assert S.SPN_SA_SPEC == ((2048, 0.2, 32, [32, 32, 64]), (512, 0.4, 32, [64, 64, 128]), (128, 0.8, 32, [128, 128, 256]),
                             (32, 1.6, 32, [256, 256, 512]))
    assert S.SPN_FP_MLP == ([256, 256], [256, 256], [256, 128], [128, 128, 128])


@pytest.mark.parametrize("kind", ["U", "S", "D"])
def test_oracle_fps_prefix_property(kind):
    """FPS picks index 0 first and no later pick depends on npoint: the seed (256) and sem (1024) samples are prefixes of level 1's"""
    x = D.batch(kind, 2, 8192, seed0=3)
    full = O.farthest_point_sample(2048, x)
    for k in (256, 1024, 2048):
        np.testing.assert_array_equal(O.farthest_point_sample(k, x), full[:, :k])


def test_nested_local_maps_invert_the_composed_fps_maps():
    from gspn_amd.tf_interpolate import nested_local_maps, nested_members
    g = torch.Generator().manual_seed(5)
    b, sizes = 3, (2048, 512, 128, 32)
    chain = [torch.stack([torch.randperm(sizes[i], generator=g)[:sizes[i + 1]] for _ in range(b)]).int() for i in range(3)]
    local = nested_local_maps(sizes[0], chain, prefixes=(64, 1))
    assert local.dtype == torch.int32 and tuple(local.shape) == (6, b, sizes[0])
    members = [torch.arange(sizes[0]).expand(b, -1)] + nested_members(chain) + [torch.arange(64).expand(b, -1), torch.arange(1).expand(b, -1)]
    # composition by hand: level k's points as indices of level 1
    l3 = torch.stack([chain[0][s].long()[chain[1][s].long()] for s in range(b)])
    assert torch.equal(members[2], l3)
    assert torch.equal(members[3], torch.stack([l3[s][chain[2][s].long()] for s in range(b)]))
    for l, mem in enumerate(members):
        k = mem.shape[1]
        assert torch.equal(local[l].gather(1, mem.long()), torch.arange(k, dtype=torch.int32).expand(b, -1))    # local inverts members
        assert torch.equal((local[l] >= 0).sum(1), torch.full((b,), k))                                          # and holds nothing else
