"""CPU-side tests of gspn_amd/inference.py: the gspn_crop_mean entry point (present, bound, sizes rejected before any launch), the names
rpointnet re-exports, the refusal of CPU tensors, and the restatements of tests/inference_ref.py against loops."""
import ctypes

import pytest
import torch

from tests import inference_ref as IR


def test_crop_mean_entry_point_exists_and_rejects_bad_sizes():
    from gspn_amd import _lib, build
    build.build()
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    _I, _P = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["gspn_crop_mean"] == [_I] * 5 + [_P] * 4
    assert hasattr(lib, "gspn_crop_mean")
    assert _lib.ABI_VERSION >= 16 and lib.gspn_abi_version() == _lib.ABI_VERSION
    one = ctypes.c_void_p(16)                                                   # never dereferenced: every call below returns before a launch
    call = lambda b, n, r, p, c, ptr=one: lib.gspn_crop_mean(b, n, r, p, c, ptr, ptr, ptr, null)
    for pos in range(5):
        for bad in (0, -1):
            sizes = [2, 8, 3, 4, 20]
            sizes[pos] = bad
            assert call(*sizes) == -1
    assert call(2, 8, 3, 4, 20, null) == -1                                     # null operands
    for c in (65, 128, 1044):
        assert call(2, 8, 3, 4, c) == -2                                        # GSPN_ERR_UNSUPPORTED before anything is launched
    assert call(1 << 16, 8, 1 << 15, 4, 20) == -2                               # more (scene, ROI) pairs than a grid holds


def test_inference_names_are_exported_and_cpu_tensors_are_refused():
    from gspn_amd import inference
    from gspn_amd import rpointnet as RP
    from gspn_amd._lib import GspnHipError
    for name in ("rpointnet_inference", "crop_mean"):
        assert name in RP.__all__ and name in inference.__all__ and getattr(RP, name) is getattr(inference, name)
    x = torch.zeros(1, 8, 3)
    args = (x, x, torch.zeros(1, 2, 512, 3), torch.zeros(1, 8, dtype=torch.int64), torch.ones(1, 2), torch.zeros(1, 8, dtype=torch.int64),
            torch.zeros(1, 2, 6))
    with pytest.raises(GspnHipError):
        RP.rpointnet_inference(*args, RP.Config(istrain=False))
    with pytest.raises(GspnHipError):
        RP.rpointnet_inference(*args, RP.Config(istrain=False), fused_crop=True)
    with pytest.raises(GspnHipError):
        RP.crop_mean(torch.zeros(1, 8, 4), torch.zeros(1, 2, 5, dtype=torch.int32))
    with pytest.raises(ValueError):
        RP.crop_mean(torch.zeros(1, 8, 4), torch.zeros(1, 2, 5, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="inference"):                  # the old driver still refuses, and says where to go
        RP.rpointnet(*args, RP.Config(), False, mode='inference')


def test_crop_mean_restatement_equals_a_loop():
    g = torch.Generator().manual_seed(3)
    b, n, r, p, c = 2, 37, 4, 9, 5
    table = torch.rand(b, n, c, generator=g)
    idx = torch.randint(0, n, (b, r, p), generator=g).int()
    idx[0, 0] = 0
    idx[1, 1] = 11
    idx[0, 2, :4] = torch.tensor([-1, n, -7, n + 100]).int()                    # clamped to 0 and n - 1
    want = IR.crop_mean_naive(table, idx)
    got = IR.crop_mean(table, idx)
    assert got.dtype == torch.float64 and got.shape == (b, r, c)
    assert float((got - want).abs().max()) <= 1e-15
    assert torch.equal(got[0, 0], table[0, 0].double()) and float((got[1, 1] - table[1, 11].double()).abs().max()) <= 1e-16
    clamped = idx.clone()
    clamped[0, 2, :4] = torch.tensor([0, n - 1, 0, n - 1]).int()
    assert torch.equal(IR.crop_mean(table, clamped), got)


def test_nearest_seed_and_first_max_pick_restatements():
    pc = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.0, 0.0], [3.0, 1.0, 0.0]]])
    seeds = torch.tensor([[[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]])
    assert IR.nearest_seed(pc, seeds).tolist() == [[1, 0, 0, 0]]                 # equal distances: the first seed
    fb = torch.tensor([[[0.875, 0.125], [0.25, 0.75], [0.5, 0.5]]])
    logits = torch.tensor([[[0.0, 1.0], [2.0, 0.0], [0.0, 0.0], [1.0, 1.0]]])
    table = IR.point_probabilities(pc, seeds, fb, logits)
    assert table.shape == (1, 4, 3) and table[0, :, 0].tolist() == [0.75, 0.125, 0.125, 0.125]
    assert float((table[0, :, 1:].sum(-1) - 1).abs().max()) < 1e-15
    values = torch.tensor([[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]]])
    pick = IR.first_max_pick(values, torch.tensor([[[0.0, 5.0, 5.0], [1.0, 1.0, 1.0], [0.0, 0.0, 2.0]]]))
    assert pick.tolist() == [[2.0, 4.0, 9.0]]
