"""CPU tests of gspn_amd/train.py: ABI 20 and its four symbols against the header's argument lists, the schedules of train.py:87-119 against
closed forms, checkpoints of a CPU VariableStore (round trip, restore under a scope, the two errors), and the int64 restatement of
gspn_batch_perm as a bijection."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("gspn_batch_assemble", "gspn_adam_tf_flat", "gspn_momentum_flat", "gspn_scalars_accumulate")


def _ctype(decl):
    decl = decl.strip()
    if "*" in decl:
        return ctypes.c_void_p
    kind = decl.replace("const ", "").split()[0]
    return {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}[kind]


def test_abi_20_and_the_train_symbols():
    from gspn_amd import _lib, build
    build.build()
    text = open(os.path.join(ROOT, "include", "gspn_hip.h")).read()
    lib = _lib.lib()
    assert int(re.search(r"#define GSPN_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == lib.gspn_abi_version() >= 20
    assert re.search(r"^ \*\s+20: gspn_batch_assemble / gspn_adam_tf_flat / gspn_momentum_flat / gspn_scalars_accumulate", text, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name)
        declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        assert [_ctype(a) for a in declared] == _lib.SIGNATURES[name], name
    # gspn_adam_tf_flat is gspn_adam_flat without weight_decay
    flat = list(_lib.SIGNATURES["gspn_adam_flat"])
    del flat[9]
    assert _lib.SIGNATURES["gspn_adam_tf_flat"] == flat
    assert len(_lib.SIGNATURES["gspn_momentum_flat"]) == 8 and len(_lib.SIGNATURES["gspn_scalars_accumulate"]) == 5
    from gspn_amd import train as T
    for macro, value in (("GSPN_PERM_STREAM", T.PERM_STREAM), ("GSPN_AUGMENT_STREAM", T.AUGMENT_STREAM), ("GSPN_SCALARS_MAX", T.SCALARS_MAX)):
        assert int(re.search(r"#define %s (\w+)" % macro, text).group(1).rstrip("u"), 0) == value
    from gspn_amd.dataset import SCENE_STREAM
    assert len({T.PERM_STREAM, T.AUGMENT_STREAM, SCENE_STREAM, 0xFFFFFFFF}) == 4
    from gspn_amd.build import POLICY_SOURCES
    assert "train.hip" not in POLICY_SOURCES
    # host-side argument rules (no launch)
    null = ctypes.c_void_p(0)
    assert lib.gspn_adam_tf_flat(4, null, null, null, null, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1, null) == -1
    assert lib.gspn_adam_tf_flat(0, null, null, null, null, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0, null) == -1            # step >= 1
    assert lib.gspn_momentum_flat(4, null, null, null, 1e-3, 0.9, 1.0, null) == -1
    assert lib.gspn_scalars_accumulate(17, null, null, null, null) == -1
    assert lib.gspn_batch_assemble(*([1, 1, 8, 1, 1] + [null] * 8 + [1, 1] + [null] * 11)) == -1


def close(got, want):
    return abs(got - want) <= 1e-12 * abs(want) if want != 0 else got == 0


def test_schedules_against_closed_forms():
    from gspn_amd.train import Schedules
    s = Schedules(batch_size=2)
    for step in (0, 27499):
        assert close(s.learning_rate(step), 1e-3) and close(s.bn_decay(step), 0.5) and close(s.loss_weight(step), 0.0)
    assert close(s.learning_rate(27500), 7e-4) and close(s.bn_decay(27500), 0.75) and close(s.loss_weight(27500), 0.3)
    assert close(1.0 - 0.5 * 0.5 ** 6, 0.9921875) and close(s.bn_decay(6 * 27500), 0.99)                           # clipped
    assert close(s.bn_decay(5 * 27500), 0.984375)
    assert close(1e-3 * 0.7 ** 13, 9.688901040699992e-06) and close(s.learning_rate(13 * 27500), 1e-5)            # the floor
    assert close(s.learning_rate(12 * 27500), 1e-3 * 0.7 ** 12)
    half = Schedules(batch_size=2, kl_weight=0.5)
    assert close(half.loss_weight(0), 0.0) and close(half.loss_weight(27500), 0.15) and close(half.loss_weight(2 * 27500), 0.5 * (1 - 0.49))
    other = Schedules(batch_size=8, learning_rate=1e-2, decay_step=40, decay_rate=0.5)
    assert close(other.learning_rate(4), 1e-2) and close(other.learning_rate(5), 5e-3) and close(other.bn_decay(10), 0.875)
    with pytest.raises(ValueError):
        Schedules(batch_size=0)


def make_store(seed, shapes):
    from gspn_amd import tf_util
    store = tf_util.VariableStore(device=torch.device("cpu"), seed=seed)
    old = tf_util.get_variable_store()
    tf_util.set_variable_store(store)
    try:
        for name, (shape, trainable) in shapes.items():
            scope, leaf = name.rsplit("/", 1)
            with tf_util.variable_scope(scope):
                tf_util.get_variable(leaf, shape, tf_util.xavier_initializer() if len(shape) > 1 else tf_util.truncated_normal_initializer(1.0),
                                     trainable=trainable)
    finally:
        tf_util.set_variable_store(old)
    return store


SHAPES = {"a/conv/weights": ((1, 1, 6, 8), True), "a/conv/bn/moving_mean": ((8,), False), "a/conv/bn/moving_variance": ((8,), False),
          "ab/fc/weights": ((8, 5), True), "b/fc/biases": ((5,), True), "b/fc/bn/moving_mean": ((5,), False)}


def test_checkpoint_round_trip_and_scope(tmp_path):
    from gspn_amd.train import restore_variables, save_variables
    src, dst = make_store(1, SHAPES), make_store(2, SHAPES)
    assert all(not torch.equal(src.vars[n], dst.vars[n]) for n in SHAPES)
    path = save_variables(str(tmp_path / "model.ckpt"), src, step=7)
    ptrs = {n: v.data_ptr() for n, v in dst.vars.items()}
    ckpt = restore_variables(path, dst)
    assert ckpt["step"] == 7 and list(ckpt["variables"]) == list(SHAPES)
    for n in SHAPES:                                                       # bit-equal, moving statistics included, written in place
        assert torch.equal(src.vars[n], dst.vars[n]) and dst.vars[n].data_ptr() == ptrs[n], n
    assert dst.vars["a/conv/weights"].requires_grad and not dst.vars["a/conv/bn/moving_mean"].requires_grad

    part = make_store(3, SHAPES)
    before = {n: v.detach().clone() for n, v in part.vars.items()}
    restore_variables(path, part, scope='a')
    for n in SHAPES:                                                       # 'ab/...' is not under 'a'
        if n.startswith("a/"):
            assert torch.equal(part.vars[n], src.vars[n]), n
        else:
            assert torch.equal(part.vars[n], before[n]), n
    with pytest.raises(KeyError):
        restore_variables(path, part, scope='nothing_here')


def test_checkpoint_errors_name_the_variable(tmp_path):
    from gspn_amd.train import restore_variables, save_variables
    src = make_store(1, SHAPES)
    path = save_variables(str(tmp_path / "model.ckpt"), src)
    more = dict(SHAPES)
    more["b/extra/weights"] = ((5, 3), True)
    dst = make_store(2, more)
    before = {n: v.detach().clone() for n, v in dst.vars.items()}
    with pytest.raises(KeyError, match="b/extra/weights"):
        restore_variables(path, dst)
    restore_variables(path, dst, scope='a')                                # the missing name is outside the scope
    wrong = dict(SHAPES)
    wrong["ab/fc/weights"] = ((8, 4), True)
    dst = make_store(2, wrong)
    before = {n: v.detach().clone() for n, v in dst.vars.items()}
    with pytest.raises(ValueError, match="ab/fc/weights"):
        restore_variables(path, dst)
    assert all(torch.equal(dst.vars[n], before[n]) for n in wrong)         # nothing was written before the check failed


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 1000, 4096, 18000])
def test_permutation_restatement_is_a_bijection(n):
    from gspn_amd.train import batch_perm
    perm = batch_perm(torch.tensor([11], dtype=torch.int64), 3, n)
    assert perm.dtype == torch.int64 and tuple(perm.shape) == (3, n)
    want = torch.arange(n)
    for s in range(3):
        assert torch.equal(torch.sort(perm[s]).values, want)
    again = batch_perm(torch.tensor([11], dtype=torch.int64), 3, n)
    assert torch.equal(perm, again)                                        # stateless
    if n >= 64:
        assert not torch.equal(perm[0], perm[1]) and not torch.equal(perm[0], want)
        assert not torch.equal(perm, batch_perm(torch.tensor([12], dtype=torch.int64), 3, n))
