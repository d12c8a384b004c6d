"""CPU checks of the R-PointNet heads (no GPU needed): the static-shape losses of gspn_amd/heads.py equal the float64 restatements of
tests/heads_ref.py (real indexing, tf.cond as an `if`) within 1e-5, the entry points of csrc/heads.hip exist and reject bad sizes, the new
names are exported from gspn_amd.rpointnet and CPU tensors are refused."""
import ctypes

import pytest
import torch

from tests import heads_ref as HR

K, P = 5, 16


class _Cfg:
    NUM_CATEGORY, NUM_POINT_INS_MASK = K, P


def _ref_terms(ep):
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in ep.items()}
    valid = (d["rois"].abs().sum(-1) != 0).double()
    cl = HR.class_loss(d["rpointnet_class_logits"], d["target_class_ids"], valid)
    bb, diff = HR.bbox_loss(d["target_bbox"], d["target_class_ids"], d["rpointnet_bbox"], valid, K)
    mk = HR.mask_loss(d["target_mask"], d["target_class_ids"], d["rpointnet_mask"], valid, K, P)
    return {"rpointnet_class_loss": cl, "rpointnet_bbox_loss": bb, "rpointnet_mask_loss": mk, "loss": cl + bb + mk}, diff, valid


@pytest.mark.parametrize("kind", ["mixed", "no_positive", "all_padding"])
def test_losses_equal_the_float64_restatements(kind):
    from gspn_amd import rpointnet as RP
    ep = HR.loss_case(kind, p=P, k=K, seed=11)
    want, diff, valid = _ref_terms(ep)
    npos = int(((ep["target_class_ids"] > 0) & (valid > 0)).sum())
    if kind == "mixed":
        assert npos == 7 and int((valid == 0).sum()) > 0 and int(((ep["target_class_ids"] == 0) & (valid > 0)).sum()) > 0
        assert float((diff - 1.0).abs().min()) > 1e-4 and bool((diff > 1).any()) and bool((diff < 1).any())       # off the kink, both branches
    else:
        assert npos == 0 and (kind == "no_positive") == bool(valid.any())
    loss, out = RP.get_rpointnet_loss(dict(ep), _Cfg)
    assert out["rpointnet_class_loss"].dtype == torch.float32 and loss.shape == ()
    got = {k: out[k] for k in ("rpointnet_class_loss", "rpointnet_bbox_loss", "rpointnet_mask_loss")}
    got["loss"] = loss
    for k, w in want.items():
        g = float(got[k])
        print("%s %s: %.9g vs %.9g" % (kind, k, g, float(w)))
        if float(w) == 0.0:
            assert g == 0.0, k                                                      # exactly 0 when no ROI qualifies
        else:
            assert abs(g - float(w)) / abs(float(w)) < 1e-5, k
    if kind == "all_padding":
        assert all(float(v) == 0.0 for v in got.values())
    if kind == "no_positive":
        assert float(got["rpointnet_bbox_loss"]) == 0.0 and float(got["rpointnet_mask_loss"]) == 0.0 and float(got["rpointnet_class_loss"]) > 0
    # the single-term functions, with the reference's signatures
    v32 = valid.float()
    assert torch.equal(RP.get_rpointnet_class_loss(ep["rpointnet_class_logits"], ep["target_class_ids"], v32), out["rpointnet_class_loss"])
    assert torch.equal(RP.get_rpointnet_bbox_loss(ep["target_bbox"], ep["target_class_ids"], ep["rpointnet_bbox"], v32, K), out["rpointnet_bbox_loss"])
    assert torch.equal(RP.get_rpointnet_mask_loss(ep["target_mask"], ep["target_class_ids"], ep["rpointnet_mask"], v32, K, P),
                       out["rpointnet_mask_loss"])


def test_loss_gradients_equal_float64_and_vanish_without_positives():
    from gspn_amd import rpointnet as RP
    keys = ("rpointnet_class_logits", "rpointnet_bbox", "rpointnet_mask")
    for kind in ("mixed", "no_positive"):
        ep = HR.loss_case(kind, p=P, k=K, seed=12)
        ep32 = {k: (v.clone().requires_grad_(True) if k in keys else v) for k, v in ep.items()}
        loss, _ = RP.get_rpointnet_loss(ep32, _Cfg)
        got = torch.autograd.grad(loss, [ep32[k] for k in keys])
        ep64 = {k: (v.double().requires_grad_(True) if k in keys else v) for k, v in ep.items()}
        want_terms, _, _ = _ref_terms(ep64)
        want = torch.autograd.grad(want_terms["loss"], [ep64[k] for k in keys], allow_unused=True)
        for k, g, w in zip(keys, got, want):
            assert bool(torch.isfinite(g).all())
            if w is None or not bool(w.any()):
                assert not bool(g.any()), k
            else:
                assert float((g.double() - w).abs().max() / w.abs().max()) < 1e-5, k


def test_heads_entry_points_exist_and_reject_bad_sizes():
    from gspn_amd import _lib, build
    build.build()
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    _I, _P, _L = ctypes.c_int, ctypes.c_void_p, ctypes.c_long
    assert _lib.SIGNATURES["gspn_crop_linear_fwd"] == [_I] * 5 + [_P, _I] + [_P] * 4 + [_I] + [_P] * 4
    assert _lib.SIGNATURES["gspn_crop_linear_bwd_side"] == [_I] * 5 + [_P] * 5 + [_I] + [_P] * 6
    assert _lib.SPECIAL["gspn_crop_linear_part_floats"] == ([_I] * 4, _L)
    for name in ("gspn_crop_linear_fwd", "gspn_crop_linear_bwd_side", "gspn_crop_linear_part_floats"):
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION >= 15 and lib.gspn_abi_version() == _lib.ABI_VERSION
    fwd = lambda b, n, r, p, c: lib.gspn_crop_linear_fwd(b, n, r, p, c, null, c, null, null, null, null, 1, null, null, null, null)
    bwd = lambda b, n, r, p, c: lib.gspn_crop_linear_bwd_side(b, n, r, p, c, null, null, null, null, null, 1, null, null, null, null, null, null)
    for pos in range(5):
        for bad in (0, -1):
            sizes = [2, 8, 3, 4, 64]
            sizes[pos] = bad
            assert fwd(*sizes) == -1 and bwd(*sizes) == -1
    assert fwd(2, 8, 3, 4, 64) == -1 and bwd(2, 8, 3, 4, 64) == -1                 # null operands
    # valid sizes outside what the kernels take: GSPN_ERR_UNSUPPORTED before anything is launched
    for cout in (6, 63, 260, 1024):
        assert fwd(2, 8, 3, 4, cout) == -2 and bwd(2, 8, 3, 4, cout) == -2
    assert fwd(1 << 15, 8, 1 << 8, 1 << 8, 64) == -2
    part = lib.gspn_crop_linear_part_floats
    assert [part(*s) for s in ((0, 3, 4, 64), (2, 0, 4, 64), (2, 3, 0, 64), (2, 3, 4, 0), (2, 3, 4, 6), (-1, 3, 4, 64))] == [0] * 6
    assert part(1, 1, 1, 4) == 7 * 4 and part(2, 64, 256, 64) == 256 * 7 * 64 and part(2, 384, 1024, 128) == 512 * 7 * 128


def test_heads_names_are_exported_and_cpu_tensors_are_refused():
    from gspn_amd import heads
    from gspn_amd import rpointnet as RP
    from gspn_amd._lib import GspnHipError
    from gspn_amd.mlp import LayerParams
    for name in ("crop_linear", "classification_head", "segmentation_head", "fpn_features", "get_rpointnet_class_loss",
                 "get_rpointnet_bbox_loss", "get_rpointnet_mask_loss", "get_rpointnet_loss"):
        assert name in RP.__all__ and name in heads.__all__ and getattr(RP, name) is getattr(heads, name)
    pc, fea, cen, rois, idx, w, bias = HR.crop_linear_case(1, 7, 8, 2, 5, 4)
    with pytest.raises(GspnHipError):
        RP.crop_linear(pc, fea, cen, rois, idx, LayerParams(w, bias, False))
    with pytest.raises(ValueError):
        RP.crop_linear(pc, fea, cen, rois, idx.long(), LayerParams(w, bias, False))
    with pytest.raises(GspnHipError):
        RP.classification_head(torch.zeros(1, 2, 5, 3), torch.zeros(1, 2, 5, 11), 3, [8], [8], False, None, 'classification_head')
    with pytest.raises(GspnHipError):
        RP.segmentation_head(torch.zeros(1, 2, 5, 3), torch.zeros(1, 2, 5, 11), 3, [8], [8], [8], False, None, 'segmentation_head')
    with pytest.raises(GspnHipError):
        RP.fpn_features({'sem_fea_full_l%d' % i: torch.zeros(1, 4, 7) for i in (1, 2, 3, 4)}, False, None)


def test_crop_rows_restatement_is_points_cropping():
    """tests/heads_ref.crop_rows is the concatenation of what tests/roi_ref.points_cropping returns (the restatement test_gpu_roi.py holds
    roi.points_cropping to), in the heads' column order"""
    from tests import roi_ref as RR
    pc, fea, cen, rois, idx, _, _ = HR.crop_linear_case(2, 50, 8, 4, 9, 4, seed=3)
    for normalize in (True, False):
        f, c, x, _ = RR.points_cropping(pc, fea, cen, rois, idx, normalize)
        assert torch.equal(HR.crop_rows(pc, fea, cen, rois, idx, normalize), torch.cat((f, c, x), -1))
    assert not rois[:, -1].any() and not idx[:, -1].any() and int(idx[0, 1].unique().numel()) < 9
