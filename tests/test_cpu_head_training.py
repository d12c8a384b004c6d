"""CPU tests of the head-training driver's surface: the exported names, the guards (which raise without a device), the messages of the two
pinned signatures and the ABI-17 entry points in the header and the binding."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rpointnet_heads_from_proposals", "rpointnet_head_training", "get_head_training_loss", "tile_linear", "shared_first_layers"]


def test_new_names_are_exported():
    from gspn_amd import heads, rpointnet, training
    for name in NEW:
        assert name in rpointnet.__all__ and callable(getattr(rpointnet, name)), name
    assert training.__all__ == NEW[:3]
    for name in NEW[:3]:
        assert getattr(rpointnet, name) is getattr(training, name)
    for name in NEW[3:]:
        assert name in heads.__all__ and getattr(rpointnet, name) is getattr(heads, name)
    import inspect
    assert inspect.signature(heads.segmentation_head).parameters["split_post"].default is False
    for fn in (training.rpointnet_heads_from_proposals, training.rpointnet_head_training):
        params = inspect.signature(fn).parameters
        for switch in ("fused_crop", "shared_first", "split_post"):
            assert params[switch].default is False and params[switch].kind is inspect.Parameter.KEYWORD_ONLY, switch


def _args():
    x = torch.zeros(1, 8, 3)
    return (x, x, torch.zeros(1, 2, 512, 3), torch.zeros(1, 8, dtype=torch.int64), torch.ones(1, 2), torch.zeros(1, 8, dtype=torch.int64),
            torch.zeros(1, 2, 6))


@pytest.mark.parametrize("modules", [['SPN'], ['SPN', 'RPOINTNET'], []])
def test_guards_raise_without_a_device(modules):
    from gspn_amd import rpointnet as RP
    cfg = RP.Config()
    cfg.TRAIN_MODULE = modules
    args = _args()
    with pytest.raises(NotImplementedError, match="TRAIN_MODULE"):
        RP.rpointnet_head_training(*args, cfg, True)
    with pytest.raises(NotImplementedError, match="TRAIN_MODULE"):
        RP.rpointnet_heads_from_proposals({}, args[0], args[3], args[5], args[6], cfg, True)
    with pytest.raises(NotImplementedError, match="TRAIN_MODULE"):
        RP.get_head_training_loss({}, cfg, 1.0, None)


def test_the_combination_names_its_reason():
    from gspn_amd import rpointnet as RP
    cfg = RP.Config()
    cfg.TRAIN_MODULE = ['SPN', 'RPOINTNET']
    with pytest.raises(NotImplementedError, match="return_fullfea=False"):
        RP.rpointnet_head_training(*_args(), cfg, True)


def test_head_training_rejects_cpu_tensors():
    from gspn_amd import rpointnet as RP
    from gspn_amd._lib import GspnHipError
    cfg = RP.Config()
    cfg.TRAIN_MODULE = ['RPOINTNET']
    with pytest.raises(GspnHipError):
        RP.rpointnet_head_training(*_args(), cfg, True)


def test_pinned_signatures_name_the_new_functions():
    from gspn_amd import rpointnet as RP
    cfg = RP.Config()
    cfg.TRAIN_MODULE = ['RPOINTNET']
    with pytest.raises(NotImplementedError, match="rpointnet_head_training") as e:
        RP.rpointnet(*_args(), cfg, True)
    assert "get_head_training_loss" in str(e.value)
    with pytest.raises(NotImplementedError, match="get_head_training_loss"):
        RP.get_loss({}, cfg, 1.0, None)


def test_abi_17_symbols_in_header_and_binding():
    from gspn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    assert int(re.search(r"#define GSPN_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 17
    lib = _lib.lib()
    assert lib.gspn_abi_version() == _lib.ABI_VERSION
    decl = {"gspn_tile_add": r"int gspn_tile_add\(long groups, int p, int c, const float\* A, const float\* G, float\* Y, void\* stream\);",
            "gspn_tile_sum": r"int gspn_tile_sum\(long groups, int p, int c, const float\* dY, float\* part, float\* dG, void\* stream\);",
            "gspn_tile_sum_part_floats": r"long gspn_tile_sum_part_floats\(long groups, int p, int c\);"}
    for name, pattern in decl.items():
        assert re.search(pattern, hdr), name
        assert hasattr(lib, name), name
    L, I, P = _lib._L, _lib._I, _lib._P
    assert _lib.SIGNATURES["gspn_tile_add"] == [L, I, I, P, P, P, P]
    assert _lib.SIGNATURES["gspn_tile_sum"] == [L, I, I, P, P, P, P]
    assert _lib.SPECIAL["gspn_tile_sum_part_floats"] == ([L, I, I], L)
    # the host side of the launchers: sizes are checked before anything touches a device
    assert lib.gspn_tile_sum_part_floats(3, 256, 256) == 2 * 3 * 4 * 256           # 4 parts of 64 rows, doubles counted in floats
    assert lib.gspn_tile_sum_part_floats(4, 64, 1024) == 0 and lib.gspn_tile_sum_part_floats(3, 256, 6) == 0
    assert lib.gspn_tile_add(2, 3, 6, None, None, None, None) == -2 and lib.gspn_tile_add(0, 3, 8, None, None, None, None) == -1
    assert lib.gspn_tile_sum(2, 3, 1028, None, None, None, None) == -2 and lib.gspn_tile_sum(2, 3, 8, None, None, None, None) == -1
