"""GPU tests of the three box kernels of csrc/spn_boxes.hip through gspn_amd/spn_boxes.py: box_shrink and points_bbox bit-equal to their
fp32 torch restatements (tests/spn_ref.py, computed on the CPU), spn_target_gen equal to the float64 restatement wherever the largest IoU
is clear of the 0.5 threshold -- and the seeded inputs are asserted to be clear of it everywhere."""
import pytest
import torch

from tests import spn_ref as SR

pytestmark = pytest.mark.gpu

ROOM = torch.tensor([8.0, 6.0, 3.0])
# planted points (far from the room, so the boxes around them hold nothing else) and the boxes that go with them
LONE = torch.tensor([60.0, 60.0, 60.0])
FLAT = torch.tensor([[50.1, 50.2, 50.5], [50.3, 50.1, 50.5], [50.2, 50.4, 50.5]])           # one z
FACE = torch.tensor([[70.5, 70.25, 70.75], [70.25, 70.125, 70.5]])
SPECIAL_BOXES = torch.tensor([
    [100.0, 100.0, 100.0, 1.0, 1.0, 1.0],                   # empty
    [60.0, 60.0, 60.0, 1.0, 1.0, 1.0],                      # holds one point
    [50.2, 50.2, 50.5, 1.0, 1.0, 1.0],                      # holds three points flat on z
    # size 1 (a power of two) and c = FACE[0] - 0.5, both exact in fp32: c + size/2 is FACE[0]'s own coordinate, the point is ON the face
    [70.0, 69.75, 70.25, 1.0, 1.0, 1.0],
])


def shrink_case(b, s, n, seed):
    g = torch.Generator().manual_seed(seed)
    pc = torch.rand(b, n, 3, generator=g) * ROOM
    box = torch.cat((torch.rand(b, s, 3, generator=g) * ROOM, torch.rand(b, s, 3, generator=g) * 1.5 + 0.05), -1)
    planted = torch.cat((LONE.unsqueeze(0), FLAT, FACE))
    k = min(n, planted.shape[0])
    pc[:, :k] = planted[:k]
    ks = min(s, SPECIAL_BOXES.shape[0])
    box[:, :ks] = SPECIAL_BOXES[:ks]
    return box.contiguous(), pc.contiguous()


@pytest.mark.parametrize("b,s,n", [(2, 256, 18000), (2, 2048, 18000), (1, 1, 1), (3, 65, 1000), (1, 7, 63)])
def test_box_shrink_bit_equal(b, s, n):
    from gspn_amd.spn_boxes import box_shrink
    box, pc = shrink_case(b, s, n, 7 * s + n)
    got = box_shrink(box.cuda(), pc.cuda()).cpu()
    want = SR.box_shrink_direct(box, pc)
    assert got.shape == (b, s, 6) and got.dtype == torch.float32
    assert torch.equal(got, want)                          # (-0.0 == 0.0 here, which is wanted)
    if s >= 4 and n >= 6:
        assert not got[:, :3].any()                        # empty, one point, flat: six zeros each
        hi = FACE[0]
        lo = FACE[1]
        assert torch.equal(got[:, 3], torch.cat(((hi + lo) / 2, hi - lo + 1e-3)).expand(b, 6))       # the point on the face is inside
        if n >= 1000:
            assert got[:, 4:].abs().sum() > 0                  # (63 random points leave the few other boxes empty)


def test_box_shrink_rejects_bad_shapes():
    from gspn_amd.spn_boxes import box_shrink
    with pytest.raises(ValueError):
        box_shrink(torch.zeros(2, 4, 5, device="cuda"), torch.zeros(2, 8, 3, device="cuda"))
    with pytest.raises(ValueError):
        box_shrink(torch.zeros(2, 4, 6, device="cuda"), torch.zeros(1, 8, 3, device="cuda"))
    with pytest.raises(ValueError):
        box_shrink(torch.zeros(2, 0, 6, device="cuda"), torch.zeros(2, 8, 3, device="cuda"))


@pytest.mark.parametrize("rows,m", [(512, 512), (200, 512), (1, 1), (5, 1000)])
@pytest.mark.parametrize("with_offset", [False, True])
def test_points_bbox_bit_equal(rows, m, with_offset):
    from gspn_amd.spn_boxes import points_bbox
    g = torch.Generator().manual_seed(rows + m)
    pts = torch.randn(rows, m, 3, generator=g)
    off = torch.rand(rows, 3, generator=g) * ROOM if with_offset else None
    got = points_bbox(pts.cuda().requires_grad_(True), off.cuda() if with_offset else None)
    assert not got.requires_grad
    assert torch.equal(got.cpu(), SR.points_bbox(pts, off))


def test_points_bbox_keeps_leading_dimensions():
    from gspn_amd.spn_boxes import points_bbox
    g = torch.Generator().manual_seed(5)
    pts, off = torch.randn(2, 7, 33, 3, generator=g), torch.randn(2, 7, 3, generator=g)
    got = points_bbox(pts.cuda(), off.cuda())
    assert got.shape == (2, 7, 6) and torch.equal(got.cpu(), SR.points_bbox(pts, off))
    with pytest.raises(ValueError):
        points_bbox(pts.cuda(), off[:, :6].cuda())


def _check_targets(args):
    """equal to float64 on every proposal whose largest IoU is farther than 1e-5 from 0.5 -- and that must be every proposal"""
    from gspn_amd.spn_boxes import spn_target_gen_batch
    got = spn_target_gen_batch(*(a.cuda() for a in args)).cpu()
    want, iou = SR.spn_target_gen_batch(*args)
    clear = (iou - 0.5).abs() > 1e-5
    assert bool(clear.all()), "seeded inputs must stay clear of the threshold: %d do not" % int((~clear).sum())
    assert got.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got[clear], want[clear])
    return got


def test_spn_target_gen_seeded_scenes():
    counts = torch.zeros(3)
    for seed in range(20):
        got = _check_targets(SR.seeded_target_inputs(seed))
        counts += torch.tensor([(got == 1).sum(), (got == -1).sum(), (got == 0).sum()])
    assert float(counts.min()) / float(counts.sum()) > 0.03, counts          # all three classes are exercised


def test_spn_target_gen_large_batch():
    _check_targets(SR.seeded_target_inputs(100, b=8, s=2048))


@pytest.mark.parametrize("name", sorted(SR.hand_made_scenes()))
def test_spn_target_gen_hand_made_scenes(name):
    from gspn_amd.rpointnet import spn_target_gen
    prop, seed_cls, gt_cls, gt, want = SR.hand_made_scenes()[name]
    got = spn_target_gen(prop.cuda(), seed_cls.cuda(), gt_cls.cuda(), gt.cuda())          # the reference's per-scene signature
    assert got.dtype == torch.float32 and got.cpu().tolist() == [float(w) for w in want]


def test_spn_target_gen_scene_without_ground_truth_in_a_batch():
    """one scene of the batch has no valid box: -1 everywhere there, the other scene unaffected"""
    args = list(SR.seeded_target_inputs(3, b=2))
    args[2][0] = 0.0
    got = _check_targets(args)
    assert bool((got[0] == -1).all()) and bool((got[1] == 1).any())
