"""CPU checks of the SPN composition (no GPU needed): the three box entry points of csrc/spn_boxes.hip exist and reject bad sizes, the
float64 / fp32 restatements of tests/spn_ref.py behave as models/model_rpointnet.py's spn_target_gen and box_shrink do on hand-made
inputs, and the public interface refuses what it does not implement."""
import ctypes

import pytest
import torch

from tests import spn_ref as SR


def test_box_entry_points_reject_bad_sizes():
    from gspn_amd import _lib, build
    build.build()
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    for b, s, n in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -2, 4), (4, 4, -3)):
        assert lib.gspn_box_shrink(b, s, n, null, null, null, null) == -1
    for rows, m in ((0, 4), (4, 0), (-1, 4), (4, -1)):
        assert lib.gspn_points_bbox(rows, m, null, null, null, null) == -1
    for b, s, g in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -1, 4), (4, 4, -1)):
        assert lib.gspn_spn_target_gen(b, s, g, null, null, null, null, null, null) == -1


@pytest.mark.parametrize("name", sorted(SR.hand_made_scenes()))
def test_spn_target_gen_restatement_on_hand_made_scenes(name):
    prop, seed_cls, gt_cls, gt, want = SR.hand_made_scenes()[name]
    match, _ = SR.spn_target_gen(prop, seed_cls, gt_cls, gt)
    assert match.tolist() == want
    match32, _ = SR.spn_target_gen(prop, seed_cls, gt_cls, gt, dtype=torch.float32)
    assert match32.tolist() == want


def test_hand_made_scene_ious_are_what_their_names_say():
    prop, seed_cls, gt_cls, gt, _ = SR.hand_made_scenes()["background_seed_at_0.9"]
    _, iou = SR.spn_target_gen(prop, seed_cls, gt_cls, gt)
    assert abs(float(iou[0]) - 0.9) < 1e-6 and abs(float(iou[1]) - 0.2) < 1e-6


def test_seeded_target_inputs_stay_clear_of_the_threshold():
    """the GPU test compares fp32 with float64 only where the largest IoU is farther than 1e-5 from 0.5 and asserts that this leaves
    nothing out; the same condition here, with fp32 and float64 agreeing everywhere and all three classes present"""
    counts = torch.zeros(3)
    for seed in range(20):
        args = SR.seeded_target_inputs(seed)
        m64, iou = SR.spn_target_gen_batch(*args)
        m32, _ = SR.spn_target_gen_batch(*args, dtype=torch.float32)
        assert int(((iou - 0.5).abs() <= 1e-5).sum()) == 0
        assert torch.equal(m64, m32)
        counts += torch.tensor([(m64 == 1).sum(), (m64 == -1).sum(), (m64 == 0).sum()])
    assert float(counts.min()) / float(counts.sum()) > 0.03, counts


def _shrink_inputs(b, s, n, seed):
    g = torch.Generator().manual_seed(seed)
    pc = torch.rand(b, n, 3, generator=g) * torch.tensor([8.0, 6.0, 3.0])
    box = torch.cat((torch.rand(b, s, 3, generator=g) * torch.tensor([8.0, 6.0, 3.0]), torch.rand(b, s, 3, generator=g) * 1.5), -1)
    box[:, 0, :3] = 100.0                                  # empty
    box[:, 1, :3] = pc[:, 0]                               # holds one point: flat on every axis
    box[:, 1, 3:] = 1e-6
    return box, pc


def test_box_shrink_direct_form_equals_gamma_form_bitwise():
    box, pc = _shrink_inputs(2, 64, 18000, 3)
    d, g = SR.box_shrink_direct(box, pc), SR.box_shrink_gamma(box, pc)
    assert d.dtype == torch.float32 and torch.equal(d, g)
    assert not d[:, 0].any() and not d[:, 1].any() and d[:, 2:].abs().sum() > 0


def test_rpointnet_refuses_what_it_does_not_implement():
    from gspn_amd import rpointnet as RP
    cfg = RP.Config()
    assert cfg.TRAIN_MODULE == ['SPN'] and cfg.NUM_SAMPLE == 256 and cfg.NUM_GROUP == 100 and cfg.NUM_POINT_INS == 512
    assert RP.Config(istrain=False).NUM_SAMPLE == 2048
    x = torch.zeros(1, 8, 3)
    args = (x, x, torch.zeros(1, 2, 512, 3), torch.zeros(1, 8, dtype=torch.int64), torch.ones(1, 2), torch.zeros(1, 8, dtype=torch.int64),
            torch.zeros(1, 2, 6))
    with pytest.raises(NotImplementedError, match="inference"):
        RP.rpointnet(*args, cfg, False, mode='inference')
    cfg.TRAIN_MODULE = ['SPN', 'RPOINTNET']
    with pytest.raises(NotImplementedError, match="RPOINTNET"):
        RP.rpointnet(*args, cfg, True)
    with pytest.raises(NotImplementedError):
        RP.get_loss({}, cfg, 1.0, None)


def test_shape_proposal_net_rejects_cpu_tensors():
    from gspn_amd._lib import GspnHipError
    from gspn_amd.shape_proposal import shape_proposal_net
    x = torch.zeros(1, 8, 3)
    with pytest.raises(GspnHipError):
        shape_proposal_net(x, x, torch.zeros(1, 2, 512, 3), torch.zeros(1, 8, dtype=torch.int64), torch.ones(1, 2), 5, 'spn', True)


def test_check_spn_inputs():
    from gspn_amd.shape_proposal import check_spn_inputs
    pc, pc_ins, ind = torch.zeros(2, 8, 3), torch.zeros(2, 4, 512, 3), torch.ones(2, 4)
    label = torch.randint(0, 4, (2, 8))
    check_spn_inputs(pc, pc_ins, label, ind)
    bad = label.clone()
    bad[1, 3] = 4
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        check_spn_inputs(pc, pc_ins, bad, ind)
    bad[1, 3] = -1
    with pytest.raises(ValueError):
        check_spn_inputs(pc, pc_ins, bad, ind)
    with pytest.raises(ValueError):
        check_spn_inputs(pc, pc_ins, label[:, :7], ind)


def test_helpers_without_a_kernel():
    """gather_selection, smooth_l1_loss, get_spn_class_loss and seg_label_per_group are plain tensor code: checked here on the CPU"""
    from gspn_amd import rpointnet as RP
    src = torch.arange(24.0).view(2, 4, 3)
    idx = torch.tensor([[2, -1, 0], [3, 3, -1]], dtype=torch.int32)
    out = RP.gather_selection(src, idx, 3)
    assert torch.equal(out[0, 0], src[0, 2]) and not out[0, 1].any() and torch.equal(out[1, 1], src[1, 3]) and not out[1, 2].any()
    assert torch.equal(RP.smooth_l1_loss(torch.tensor([0.0, 0.0]), torch.tensor([0.5, 3.0])), torch.tensor([0.125, 2.5]))
    logits = torch.randn(2, 5, 2, generator=torch.Generator().manual_seed(0))
    match = torch.tensor([[1, 0, -1, 1, 0], [0, 0, -1, -1, 1]], dtype=torch.int32)
    v = match.reshape(-1) != 0
    want = torch.nn.functional.cross_entropy(logits.reshape(-1, 2)[v], (match.reshape(-1)[v] == 1).long())
    assert abs(float(RP.get_spn_class_loss(logits, match)) - float(want)) < 1e-6
    assert float(RP.get_spn_class_loss(logits, torch.zeros_like(match))) == 0.0
    # group 0: labels 1, 2 -> 1.5 rounds to 2 (half to even); group 1: 2, 3 -> 2.5 rounds to 2; group 2 empty -> 0
    seg = torch.tensor([[1, 2, 2, 3, 7]])
    grp = torch.tensor([[0, 0, 1, 1, 3]])
    assert RP.seg_label_per_group(seg, grp, 3).tolist() == [[2, 2, 0]]
