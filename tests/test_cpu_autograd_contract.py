"""The gates behind tests/test_gpu_autograd_contract.py that need no GPU.

Completeness: every torch.autograd.Function subclass in gspn_amd/*.py, found by parsing the sources, has a row in tests/autograd_cases.py,
and every row names a class that exists -- a node added later without a row fails here.  The rows themselves are held to what the table
promises: indices with duplicates and an unreferenced target, a float64 restatement that runs, a named value test that exists.

Argument rules: mlp_stack, mlp_linear and the stand-alone batch norm reject a layer tensor of the wrong dtype, rank or size with ValueError
wherever it lives -- before the device rule, the order of gspn_amd/_args.py -- and a layer tensor on another device than x with GspnHipError.
Everything here is a CPU tensor: with or without those checks no call can reach a launch (x itself fails the device rule)."""
import ast
import glob
import os
import re

import pytest
import torch

from tests import autograd_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def function_classes():
    """-> {class name: file} of every class in gspn_amd/*.py one of whose bases is [torch.autograd.]Function"""
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "gspn_amd", "*.py"))):
        with open(path) as fh:
            tree = ast.parse(fh.read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.ClassDef):
                for base in node.bases:
                    name = base.attr if isinstance(base, ast.Attribute) else getattr(base, "id", None)
                    if name == "Function":
                        assert node.name not in found, "two autograd nodes named %s" % node.name
                        found[node.name] = os.path.basename(path)
    return found


def test_every_autograd_node_has_a_row():
    found = function_classes()
    assert len(found) >= 17, found
    rows = {c.node for c in AC.CASES}
    missing, stale = sorted(set(found) - rows), sorted(rows - set(found))
    assert not missing, "autograd nodes without a row in tests/autograd_cases.py: %s" % {k: found[k] for k in missing}
    assert not stale, "rows of tests/autograd_cases.py that name no class of gspn_amd/: %s" % stale
    forms = [c.name for c in AC.CASES if c.node == "_MlpStack"]
    assert sorted(forms) == ["mlp_stack", "mlp_stack_gathered", "mlp_stack_pooled", "mlp_stack_preagg"]     # each form saves different state
    assert len({c.name for c in AC.CASES}) == len(AC.CASES)


def kept_arguments():
    """-> {class name: sorted names} of the forward arguments a node keeps for backward, by inspection of its forward: the arguments of
    ctx.save_for_backward(...) and the right-hand sides of `ctx.<attr> = <argument>` (a tensor, or an object that holds one)"""
    kept = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "gspn_amd", "*.py"))):
        with open(path) as fh:
            tree = ast.parse(fh.read(), path)
        for cls in (n for n in ast.walk(tree) if isinstance(n, ast.ClassDef)):
            fwd = [f for f in cls.body if isinstance(f, ast.FunctionDef) and f.name == "forward"]
            if not fwd or not any((b.attr if isinstance(b, ast.Attribute) else getattr(b, "id", None)) == "Function" for b in cls.bases):
                continue
            args = {a.arg for a in fwd[0].args.args[1:]}
            names = set()
            for node in ast.walk(fwd[0]):
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "save_for_backward":
                    names |= {a.id for a in node.args if isinstance(a, ast.Name) and a.id in args}
                if isinstance(node, ast.Assign) and isinstance(node.value, ast.Name) and node.value.id in args and \
                        any(isinstance(t, ast.Attribute) and getattr(t.value, "id", None) == "ctx" for t in node.targets):
                    names.add(node.value.id)
            kept[cls.name] = sorted(names)
    return kept


SCALARS = {"_TileAdd": {"p"}, "_MlpStack": {"spec"}}       # kept arguments that are no tensor (a count) or are covered by name (the layer list)


def test_a_node_that_keeps_an_argument_has_a_row_that_rereads():
    """scenario 6 covers the rows that declare `reread`: a node whose forward keeps one of its tensor arguments -- by save_for_backward or
    as a plain attribute, directly or inside an object (roi._Lists) -- must not sit behind rows that declare none"""
    kept = kept_arguments()
    assert kept["_CropGather"] == ["idx", "lists"] and kept["_GroupPoint"] == ["idx"] and kept["_PadCols"] == [] and kept["_GroupMaxpool"] == []
    for node, names in kept.items():
        names = set(names) - SCALARS.get(node, set())
        rows = [c for c in AC.CASES if c.node == node]
        assert rows, node
        if names:
            assert all(c.reread for c in rows), "%s keeps %s for backward, but a row of it declares no re-read tensor" % (node, sorted(names))


def test_the_scan_finds_a_node_that_is_added(tmp_path, monkeypatch):
    """the parser sees both spellings of the base class, so a new node cannot hide behind an import style"""
    (tmp_path / "gspn_amd").mkdir()
    (tmp_path / "gspn_amd" / "new.py").write_text("import torch\nfrom torch.autograd import Function\n\n\nclass _A(torch.autograd.Function):\n    pass\n\n\n"
                                                  "class _B(Function):\n    pass\n\n\nclass _C(object):\n    pass\n")
    monkeypatch.setattr("tests.test_cpu_autograd_contract.ROOT", str(tmp_path))
    assert function_classes() == {"_A": "new.py", "_B": "new.py"}


@pytest.mark.parametrize("case", AC.CASES, ids=repr)
def test_a_row_is_what_the_table_promises(case):
    module, test = re.fullmatch(r"tests/(test_\w+)\.py::(test_\w+)", case.tol_from).groups()
    with open(os.path.join(ROOT, "tests", module + ".py")) as fh:
        assert re.search(r"^def %s\(" % test, fh.read(), re.M), case.tol_from
    assert case.tol_out[0] in ("rel", "allclose", "exact") and case.tol_grad[0] in ("rel", "allclose", "exact")
    assert all(t[0] == "exact" or t[1] <= 1e-4 for t in (case.tol_out, case.tol_grad))
    t = case.build()
    names = case.grads + case.params + case.consts + case.ints + case.state
    assert sorted(names) == sorted(t), (sorted(names), sorted(t))
    assert set(case.reread) <= set(names) and set(case.expand) <= set(names) and set(case.zero_scale) <= set(case.params)
    for k in case.grads + case.params + case.consts + case.state:
        assert t[k].dtype == torch.float64 and t[k].numel() > 0, k
        assert t[k].dim() == 1 or max(t[k].shape) <= 1500 and t[k].shape[-1] <= 64, (k, tuple(t[k].shape))
    for k in case.ints:
        idx = t[k]
        assert not idx.dtype.is_floating_point
        flat = idx.reshape(idx.shape[0], -1)
        assert all(int(row.unique().numel()) < row.numel() for row in flat), "%s: no duplicates" % k
        # an unreferenced target: no index names the last one, so a gradient row that receives nothing exists
        assert int(flat.min()) >= 0 and int(flat.max()) + 1 < case.targets[k], k


@pytest.mark.parametrize("case", [c for c in AC.CASES if not c.name.startswith("mlp_stack_")] + [AC.BY_NAME["mlp_stack_pooled"]], ids=repr)
def test_the_float64_restatement_runs_and_differentiates(case):
    """(the two SA rows take their geometry from the C oracle: the GPU file runs their restatement)"""
    t = {k: (v.float().double() if v.dtype.is_floating_point else v) for k, v in case.build().items()}
    for k in case.grads + case.params:
        t[k].requires_grad_(True)
    outs = case.ref(t)
    assert isinstance(outs, tuple) and all(o.dtype == torch.float64 for o in outs)
    sum(o.sum() for o in outs).backward()
    for k in case.grads + case.params:
        assert t[k].grad is not None and t[k].grad.shape == t[k].shape, k
    if case.decisions is not None:
        from tests.test_gpu_mlp import fragile_entries
        zs, ns = case.decisions(t)
        fragile, rows = fragile_entries(zs, ns)
        assert not bool(fragile.any()) and not bool(rows.any()), "%s: a ReLU or pool decision within float32 rounding: pick another seed" % case.name


# ---- D. the argument rules ----------------------------------------------------------------------------------------------------------

def _layer(cin=6, cout=8, bn=True, **over):
    from gspn_amd.mlp import LayerParams
    t = dict(weights=torch.zeros(cin, cout), biases=torch.zeros(cout), beta=torch.zeros(cout), gamma=torch.ones(cout),
             moving_mean=torch.zeros(cout), moving_variance=torch.ones(cout))
    t.update(over)
    return LayerParams(t["weights"], t["biases"], bn, *([t["beta"], t["gamma"], t["moving_mean"], t["moving_variance"]] if bn else []))


BN_NAMES = ("beta", "gamma", "moving_mean", "moving_variance")
BAD = [("dtype", lambda t: t.double()), ("rank", lambda t: t.unsqueeze(0)), ("size", lambda t: torch.cat([t, t[:1]]))]


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
@pytest.mark.parametrize("name", ("weights", "biases") + BN_NAMES)
def test_mlp_stack_rejects_a_layer_tensor_that_does_not_fit_wherever_it_lives(name, what, spoil):
    from gspn_amd.mlp import mlp_stack
    x = torch.zeros(16, 6)
    good = getattr(_layer(), name)
    for layers in ([_layer(**{name: spoil(good)})], [_layer(), _layer(cin=8, **{name: spoil(getattr(_layer(cin=8), name))})]):
        with pytest.raises(ValueError, match=name):
            mlp_stack(x, 6, layers, True, 0.5)


def test_mlp_stack_holds_the_widths_together():
    from gspn_amd.mlp import mlp_stack
    x = torch.zeros(16, 6)
    with pytest.raises(ValueError, match="weights"):
        mlp_stack(x, 5, [_layer()], True, 0.5)                        # cin does not match the first layer
    with pytest.raises(ValueError, match="layer 1: weights"):
        mlp_stack(x, 6, [_layer(), _layer(cin=7)], True, 0.5)         # the second layer does not take what the first gives
    with pytest.raises(ValueError, match="x must be"):
        mlp_stack(x.double(), 6, [_layer()], True, 0.5)
    for name in ("moving_mean", "moving_variance"):
        with pytest.raises(ValueError, match="%s is updated in place" % name):
            mlp_stack(x, 6, [_layer(**{name: torch.zeros(16)[::2]})], True, 0.5)


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
@pytest.mark.parametrize("name", ("weights", "biases"))
def test_mlp_linear_rejects_a_layer_tensor_that_does_not_fit_wherever_it_lives(name, what, spoil):
    from gspn_amd.mlp import mlp_linear
    with pytest.raises(ValueError, match=name):
        mlp_linear(torch.zeros(16, 6), 6, _layer(bn=False, **{name: spoil(getattr(_layer(), name))}))
    with pytest.raises(ValueError, match="weights"):
        mlp_linear(torch.zeros(16, 6), 5, _layer(bn=False))


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
@pytest.mark.parametrize("name", BN_NAMES)
def test_batch_norm_rejects_a_tensor_that_does_not_fit_wherever_it_lives(name, what, spoil):
    from gspn_amd.tf_util import _BatchNormRows
    lp = _layer()
    t = {k: getattr(lp, k) for k in BN_NAMES}
    t[name] = spoil(t[name])
    with pytest.raises(ValueError, match=name):
        _BatchNormRows.apply(torch.zeros(16, 8), t["gamma"], t["beta"], t["moving_mean"], t["moving_variance"], True, 0.5)
    for moving in ("moving_mean", "moving_variance"):
        t = {k: getattr(lp, k) for k in BN_NAMES}
        t[moving] = torch.zeros(16)[::2]
        with pytest.raises(ValueError, match="%s is updated in place" % moving):
            _BatchNormRows.apply(torch.zeros(16, 8), t["gamma"], t["beta"], t["moving_mean"], t["moving_variance"], True, 0.5)


def test_the_device_rule_comes_last_and_covers_every_layer_tensor():
    from gspn_amd import _lib as L
    from gspn_amd import mlp as M
    from gspn_amd.tf_util import _BatchNormRows, _apply_wide_input_layer
    x = torch.zeros(16, 6)
    lp = _layer()
    # tensors that fit, on the CPU: the device rule of x, for every entry point
    with pytest.raises(L.GspnHipError):
        M.mlp_stack(x, 6, [lp], True, 0.5)
    with pytest.raises(L.GspnHipError):
        M.mlp_linear(x, 6, _layer(bn=False))
    with pytest.raises(L.GspnHipError):
        _BatchNormRows.apply(torch.zeros(16, 8), lp.gamma, lp.beta, lp.moving_mean, lp.moving_variance, True, 0.5)
    with pytest.raises(ValueError, match="biases"):                    # the wide-input layer goes through the same helper
        _apply_wide_input_layer(x, 6, _layer(biases=torch.zeros(9)), True, True, 0.5)
    # a layer tensor that is not where x is: the helper's second half, asked directly (no tensor here is on a device)
    elsewhere = torch.device("meta")
    for name in ("weights", "biases") + BN_NAMES:
        moved = _layer(**{name: getattr(lp, name).to(elsewhere)})
        M.layer_typed(moved, 6, "probe")                              # shapes and dtypes fit wherever it lives
        with pytest.raises(L.GspnHipError, match=name):
            M.layer_on_device(moved, x.device, "probe")
    assert M.layer_on_device(lp, x.device, "probe") is lp             # contiguous tensors on the device: nothing is copied


def test_a_view_is_copied_under_autograd_and_never_takes_a_sink():
    """the helper's copies, on the CPU: values and shape of the view, a gradient that reaches the caller's tensor, a new allocation"""
    from gspn_amd import mlp as M
    store = torch.randn(8, 6, requires_grad=True)                      # (cout, cin) storage
    gamma_wide = torch.rand(16, requires_grad=True)
    lp = _layer(weights=store.t(), gamma=gamma_wide[::2])
    got = M.layer_on_device(lp, store.device, "probe")
    assert got is not lp and got.weights.is_contiguous() and got.gamma.is_contiguous()
    assert torch.equal(got.weights, store.t()) and torch.equal(got.gamma, gamma_wide[::2])
    assert got.weights.data_ptr() != store.data_ptr() and got.moving_mean is lp.moving_mean and got.biases is lp.biases
    (got.weights * 2).sum().backward()
    assert store.grad.shape == store.shape and float(store.grad.min()) == 2.0
