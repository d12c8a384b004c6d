"""The shared MLP on operands that are only 4-byte aligned, and on launches the library declines.

Almost every launcher of csrc/mlp.hip chooses between a kernel that moves 16 bytes per access and a general one, on `vec_ok(pointer, pitch)`
or on a launcher that answers GSPN_ERR_UNSUPPORTED (-2), which gspn_amd/mlp.py catches at seven places and answers with other launches.
A fresh torch allocation is always aligned far beyond 16 bytes, so neither kind of choice is ever taken the other way by the tests that hand
the stack fresh tensors.  A parameter inside parallel.FlatAdam's flat buffer, or a gradient slice of parallel.FlatGradBucket, IS 4-byte
aligned only as soon as a tensor of odd length precedes it (rpointnet's 19 class biases).  Here:

  * the stack, mlp_linear and the two module front ends against float64 with one kind of operand at a time placed 4, 8 or 12 bytes past a
    16-byte boundary (tests.test_gpu_mlp.misaligned) -- tolerances: forward 1e-5, routed gradients 1e-5, check_stack gradients 1e-4;
  * every `except NotImplementedError` of mlp.py really taken: by an input the library declines on its own where one exists, and by a stand-in
    for the entry point that counts its calls and answers -2 without launching anything;
  * all of it again with gradient sinks into a bucket whose every slice is 4-byte aligned only, over two steps, against the bucket filled by `cat`.

Every test prints a data-pointer residue of what it misplaced and which launches ran (mlp.PROFILE kinds, call counts of the entry points)."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import mlp_ref as R
from oracle import oracle as O
from tests import data as D
from tests.test_gpu_mlp import PLACES, check_stack, check_stack_routed, make_params, misaligned, place_grad, place_x, to_layers
from tests.test_gpu_modules import fresh_store, ref_params, rel_err

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2            # GSPN_ERR_UNSUPPORTED (include/gspn_hip.h): _lib.check turns it into NotImplementedError


# ---------------------------------------------------------------------------------------------------------------------- tools
@contextlib.contextmanager
def profiled(kinds):
    """collects "kind:cin->cout" of every GEMM launch group the stack times (mlp.PROFILE) into `kinds`"""
    from gspn_amd import mlp as M
    M.PROFILE = []
    try:
        yield
        torch.cuda.synchronize()
        kinds.extend("%s:%d->%d" % (e[0], e[2], e[3]) for e in M.PROFILE)
    finally:
        M.PROFILE = None


class Entry:
    """stands in for one entry point of the library: records the return code of every call, and either passes the call on or declines it
    (GSPN_ERR_UNSUPPORTED) without launching anything"""

    def __init__(self, monkeypatch, name, decline=False):
        from gspn_amd import _lib as L
        lib = L.lib()
        self.name, self.real, self.decline, self.rcs = name, getattr(lib, name), decline, []
        monkeypatch.setattr(lib, name, self)

    def __call__(self, *args):
        rc = UNSUPPORTED if self.decline else self.real(*args)
        self.rcs.append(rc)
        return rc


def diffs(res, ref):
    """largest difference of every tensor two runs of one case left, relative to the tensor's largest element in `ref`"""
    names = ["out", "dX"] + ["g%d" % i for i in range(len(ref["grads"]))]
    pairs = [(res["out"], ref["out"]), (res["dX"], ref["dX"])] + list(zip(res["grads"], ref["grads"]))
    return {n: float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-9) for n, (a, b) in zip(names, pairs)}


def residues(res):
    return sorted({t.data_ptr() % 16 for lp in res["layers"] for t in lp.tensors()})


_aligned_runs = {}          # case -> results of the run on fresh allocations (each case is run under four placements)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_runs():
    yield
    _aligned_runs.clear()


def aligned_run(key, fn):
    if key not in _aligned_runs:
        res, kinds = {}, []
        with profiled(kinds):
            fn(results=res)
        res.pop("layers")
        _aligned_runs[key] = (res, kinds)
    return _aligned_runs[key]


def report(what, case, place, res, ref, kinds, ref_kinds):
    d = diffs(res, ref)
    worst = max(d.items(), key=lambda kv: kv[1])
    print("%s %s place=%s: parameter residues %s; largest difference from the aligned run %s = %.3g; kinds %s%s"
          % (what, case, place, residues(res), worst[0], worst[1], sorted(set(kinds)), "" if sorted(kinds) == sorted(ref_kinds) else " (aligned: %s)" % sorted(set(ref_kinds))))


# ------------------------------------------------------------------------------------ 2. one misplaced kind of operand at a time
ROUTED_CASES = [
    (4096, 6, 6, [32, 32, 64], 32), (1000, 67, 67, [64, 64, 64], None), (130, 3, 3, [7, 33], 2),                             # small and ragged
    (524288, 8, 6, [32, 32, 64], 32), (131072, 68, 67, [64, 64, 128], 32), (262144, 68, 67, [64, 64, 64], None),             # the long benchmark stacks
    (32768, 132, 131, [128, 128, 256], 32), (4096, 384, 384, [256, 128], None), (16384, 192, 192, [128, 64], None),          # the short layers
]


# the three long benchmark stacks run under the "all" placement only: with all four this module took 16.8 s beside 8.7 s for tests/test_gpu_mlp.py
# (MI355X), and the sink matrix below runs them again
LONG_ROWS = 131072


@pytest.mark.parametrize("rows,ld,cin,chans,ns,place", [c + (pl,) for c in ROUTED_CASES for pl in PLACES if c[0] < LONG_ROWS or pl == "all"])
def test_stack_gradients_at_1e5_with_misplaced_operands(rows, ld, cin, chans, ns, place):
    """check_stack_routed (training, every gradient, nothing silenced) with the input, the parameters, the upstream gradient, or all of them
    4-byte aligned only.  The difference from the run on fresh allocations is printed, not asserted: a forward that runs on another kernel
    rounds differently and may flip a ReLU at the kink, which the routed reference absorbs and a run-to-run comparison would not."""
    case = (rows, ld, cin, tuple(chans), ns)
    ref, ref_kinds = aligned_run(("routed",) + case, lambda results: check_stack_routed(rows, ld, cin, chans, ns, results=results))
    res, kinds = {}, []
    with profiled(kinds):
        check_stack_routed(rows, ld, cin, chans, ns, place=place, results=res)
    report("check_stack_routed", case, place, res, ref, kinds, ref_kinds)


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("training", [True, False])
def test_wide_stack_forward_backward_with_misplaced_operands(training, place):
    """fa_layer1 of the 4-level networks (768 input channels: row-blocked K) through check_stack, both modes"""
    case = (1024, 768, 768, (256, 256), None)
    ref, ref_kinds = aligned_run(("stack", training) + case, lambda results: check_stack(1024, 768, 768, [256, 256], None, training, results=results))
    res, kinds = {}, []
    with profiled(kinds):
        check_stack(1024, 768, 768, [256, 256], None, training, place=place, results=res)
    report("check_stack training=%s" % training, case, place, res, ref, kinds, ref_kinds)


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("rows,cin,cout", [(18000 * 2, 128, 19), (640, 19, 5)])
def test_linear_layer_with_misplaced_operands(rows, cin, cout, place):
    """mlp_linear (no batch-norm, no activation: rpointnet's class scores, 128 -> 19 at 2 x 18000 points) against float64 -- forward and
    gradients at 1e-5 of the largest element, like the routed stack (no ReLU, so nothing to route; measured on MI355X: at most 5.3e-7)"""
    from gspn_amd.mlp import mlp_linear
    g = torch.Generator().manual_seed(rows + cout)
    x64 = torch.randn(rows, cin, generator=g, dtype=torch.float64)
    ps = make_params([cout], cin, seed=cout, bn=False)
    go64 = torch.randn(rows, cout, generator=g, dtype=torch.float64)
    outs = {}
    for pl in (None, place):
        lp = to_layers(ps, pl)[0]
        x = place_x(x64.float().cuda(), pl)
        out = mlp_linear(x, cin, lp)
        go = place_grad(go64.float().cuda(), pl)
        out.backward(go)
        outs[pl] = (out.detach(), x.grad, lp.weights.grad, lp.biases.grad)
        if pl is not None:
            print("mlp_linear %d x %d -> %d place=%s: residues x %d, w %d, b %d, d_out %d" % (rows, cin, cout, pl, x.data_ptr() % 16, lp.weights.data_ptr() % 16,
                                                                                            lp.biases.data_ptr() % 16, go.data_ptr() % 16))
    w64, b64 = ps[0]["w"], ps[0]["b"]
    refs = (x64 @ w64 + b64, go64 @ w64.t(), x64.t() @ go64, go64.sum(0))
    for name, got, al, ref, tol in zip(("out", "dX", "dW", "dbias"), outs[place], outs[None], refs, (1e-5, 1e-5, 1e-5, 1e-5)):
        print("  %s: error against float64 %.3g, difference from the aligned run %.3g" % (name, rel_err(got, ref), rel_err(got, al)))
        assert rel_err(got, ref) < tol, name


# ------------------------------------------------------------------------------------------------------ the module front ends
def _misplace_new_variables(monkeypatch, counter):
    """every variable the store creates from here on lives 4, 8 or 12 bytes past a 16-byte boundary (same values)"""
    from gspn_amd import tf_util

    real = tf_util.get_variable

    def get_variable(name, shape, initializer, trainable=True):
        store = tf_util.get_variable_store()
        before = len(store.vars)
        v = real(name, shape, initializer, trainable)
        if len(store.vars) > before:                       # just created
            counter[0] = counter[0] % 3 + 1
            if trainable:
                v.data = misaligned(v.data, counter[0])
            else:
                full = [k for k, t in store.vars.items() if t is v][0]
                v = store.vars[full] = misaligned(v, counter[0])
            assert v.data_ptr() % 16 == 4 * counter[0]
        return v
    monkeypatch.setattr(tf_util, "get_variable", get_variable)


@pytest.mark.parametrize("place", ["params", "all"])
def test_sa_module_with_misplaced_features_and_parameters(place, monkeypatch):
    """pointnet_sa_module with a feature matrix (the fused front end reads it 16 bytes at a time) and / or parameters that are 4-byte aligned
    only, against the float64 composition of test_sa_module_matches_oracle at its tolerances.  The pre-aggregation and gathering launchers
    reject such operands (GSPN_ERR_ARG), so the module has to route around them: parameters alone leave the gathering first layer (its
    weights are read element-wise), a misplaced feature matrix takes the materialised grouped rows."""
    from gspn_amd.pointnet_util import pointnet_sa_module
    kind, b, n, c, npoint, radius, ns, mlp = "D", 2, 2048, 64, 256, 0.4, 32, [64, 64, 128]
    xyz = D.batch(kind, b, n)
    rng = np.random.default_rng(7)
    pts = rng.random((b, n, c)).astype(np.float32)
    ridx_fps = O.farthest_point_sample(npoint, xyz)
    rnew = O.gather_point(xyz, ridx_fps)
    ridx, _ = O.query_ball_point(radius, ns, xyz, rnew)
    gx = O.group_point(xyz, ridx) - rnew[:, :, None, :]
    g = torch.from_numpy(rng.standard_normal((b, npoint, mlp[-1]))).double()
    ran = {}
    for pl in (None, place):
        entries = {nm: Entry(monkeypatch, nm) for nm in ("gspn_preagg_fwd", "gspn_mlp_fwd_gather", "gspn_mlp_fwd_pool32")}
        store = fresh_store()
        if pl is not None:
            _misplace_new_variables(monkeypatch, [0])
        txyz = torch.from_numpy(xyz).cuda()
        tpts = torch.from_numpy(pts).cuda()
        if pl == "all":
            tpts = misaligned(tpts)
            assert tpts.data_ptr() % 16 == 4
        tpts.requires_grad_(True)
        new_xyz, new_points, idx = pointnet_sa_module(txyz, tpts, npoint, radius, ns, mlp, None, False, True, 0.5, 'layer1')
        ran[pl] = {nm: list(e.rcs) for nm, e in entries.items()}
        if pl is not None:
            assert all(v.data_ptr() % 16 != 0 for v in store.vars.values())
        np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
        ps = ref_params(store, 'layer1', ['conv%d' % i for i in range(len(mlp))])
        for p in ps:                                       # the reference starts from the initial moving statistics
            p["moving_mean"] = torch.zeros_like(p["moving_mean"])
            p["moving_var"] = torch.ones_like(p["moving_var"])
        pts64 = torch.from_numpy(pts).double().requires_grad_(True)
        gidx = torch.from_numpy(ridx.astype(np.int64))
        bi = torch.arange(b)[:, None, None].expand_as(gidx)
        x64 = torch.cat([torch.from_numpy(gx).double(), pts64[bi, gidx]], -1).reshape(-1, 3 + c)
        ref, moving = R.stack(x64, ps, True, 0.5, ns)
        ref = ref.view(b, npoint, mlp[-1])
        assert rel_err(new_points, ref) < 1e-5
        ref.backward(g)
        new_points.backward(g.float().cuda())
        for i, p in enumerate(ps):
            assert rel_err(store.vars['layer1/conv%d/weights' % i].grad.view(p["w"].shape), p["w"].grad) < 1e-4
            assert rel_err(store.vars['layer1/conv%d/bn/gamma' % i].grad, p["gamma"].grad) < 1e-4
            assert rel_err(store.vars['layer1/conv%d/bn/moving_mean' % i], moving[i][0]) < 1e-5
        assert rel_err(tpts.grad, pts64.grad) < 1e-4
        monkeypatch.undo()
    print("pointnet_sa_module place=%s: entry points called (return codes) aligned %s, misplaced %s" % (place, ran[None], ran[place]))
    assert ran[None]["gspn_preagg_fwd"] == [0] or ran[None]["gspn_mlp_fwd_gather"] == [0]      # fresh allocations take a fused front end
    assert not ran[place]["gspn_preagg_fwd"]               # the pre-aggregation rejects misplaced weights / source rows: never offered them
    if place == "all":
        assert not ran[place]["gspn_mlp_fwd_gather"]       # ... and the gathering first layer a misplaced feature matrix


@pytest.mark.parametrize("place", ["params", "all"])
def test_fp_module_with_misplaced_features_and_parameters(place, monkeypatch):
    """pointnet_fp_module at the shape of test_fp_module_preaggregated_first_layer (skip link of 3 columns without a gradient) with the
    parameters, or the sparse features and the parameters, 4-byte aligned only: against that test's float64 composition at its tolerances
    (output 1e-5, d(points2) 1e-4).  Fresh allocations take the pre-aggregated first layer; the misplaced ones must not be offered to it."""
    from gspn_amd import pointnet_util as PU
    b, n1, n2, c1, c2, mlp = 2, 4096, 512, 3, 64, [64, 64, 64]
    xyz1 = D.batch("D", b, n1, 3)
    xyz2 = O.gather_point(xyz1, O.farthest_point_sample(n2, xyz1))
    rng = np.random.default_rng(23)
    p1 = rng.standard_normal((b, n1, c1)).astype(np.float32)
    p2 = rng.standard_normal((b, n2, c2)).astype(np.float32)
    g = rng.standard_normal((b, n1, mlp[-1])).astype(np.float32)
    rd, ri = O.three_nn(xyz1, xyz2)
    w64 = R.fp_weights(torch.from_numpy(rd).double())
    gi = torch.from_numpy(ri.astype(np.int64))
    bi = torch.arange(b)[:, None, None].expand_as(gi)
    ran, grads = {}, {}
    for pl in (None, place):
        pre = Entry(monkeypatch, "gspn_preagg_fwd")
        store = fresh_store(99)
        if pl is not None:
            _misplace_new_variables(monkeypatch, [0])
        t1 = torch.from_numpy(p1).cuda()
        t2 = torch.from_numpy(p2).cuda()
        if pl == "all":
            t2 = misaligned(t2)
            assert t2.data_ptr() % 16 == 4
        t2.requires_grad_(True)
        out = PU.pointnet_fp_module(torch.from_numpy(xyz1).cuda(), torch.from_numpy(xyz2).cuda(), t1, t2, mlp, True, 0.5, 'fa')
        ran[pl] = list(pre.rcs)
        if pl is not None:
            assert all(v.data_ptr() % 16 != 0 for v in store.vars.values())
        out.backward(torch.from_numpy(g).cuda())
        grads[pl] = {k: v.grad.clone() for k, v in store.named_parameters()}
        p2r = torch.from_numpy(p2).double().requires_grad_(True)
        interp = (p2r[bi, gi] * w64[..., None]).sum(2)
        cat = torch.cat([interp, torch.from_numpy(p1).double()], 2)
        ps = ref_params(store, 'fa', ['conv_%d' % i for i in range(len(mlp))])
        for p in ps:
            p["moving_mean"] = torch.zeros_like(p["moving_mean"])
            p["moving_var"] = torch.ones_like(p["moving_var"])
        ref, _ = R.stack(cat.reshape(b * n1, -1), ps, True, 0.5, None)
        assert rel_err(out, ref.view(b, n1, mlp[-1])) < 1e-5
        ref.view(b, n1, mlp[-1]).backward(torch.from_numpy(g).double())
        assert rel_err(t2.grad, p2r.grad) < 1e-4
        monkeypatch.undo()
    worst = max((rel_err(grads[place][k], grads[None][k]), k) for k in grads[None])
    print("pointnet_fp_module place=%s: gspn_preagg_fwd return codes aligned %s, misplaced %s; largest parameter-gradient difference from the aligned run %.3g (%s)"
          % (place, ran[None], ran[place], worst[0], worst[1]))
    assert ran[None] == [0] and not ran[place]


# ------------------------------------------------------------------------------------------------ 3. every decline site, declined
POOL32 = (4096, 8, 6, [32, 32, 64], 32)
# (name, entry point, case, the placement that makes the library decline it by itself or None, forward site?)
DECLINES = [
    ("fwd_pool32", "gspn_mlp_fwd_pool32", POOL32, None, True),                                             # mlp.py: plain forward + the stand-alone pool
    ("pool32_select", "gspn_pool32_select", POOL32, None, True),                                           # ... the stand-alone pool over (rows, c)
    ("pool32_select_groups", "gspn_pool32_select_groups", (8192, 8, 6, [64, 128], 256), None, True),
    ("dense_rsum", "gspn_dense_rsum", (65536, 20, 20, [64, 64, 64], None), "grad", False),                 # d_out is read as quads
    ("fused_coef", "gspn_mlp_bwd_fused_coef", (131072, 8, 6, [32, 32, 64], 32), "grad", False),            # the pooled top layer reads dPool as quads
    ("fused_coef_128", "gspn_mlp_bwd_fused_coef", (131072, 68, 67, [64, 64, 128], 32), "grad", False),     # ... and so does the lean pass A behind it
    ("wgrad_known", "gspn_mlp_bwd_wgrad_known", POOL32, "x", False),                                       # the one-GEMM pass A streams X through the LDS DMA
    ("pooltop", "gspn_mlp_bwd_data_pooltop", (4096, 32, 32, [32, 64], 32), None, False),
]


def _run_case(case, place=None):
    rows, ld, cin, chans, ns = case
    res, kinds = {}, []
    with profiled(kinds):
        check_stack_routed(rows, ld, cin, chans, ns, place=place, results=res)
    return res, kinds


def _compare_declined(name, dec, ctl, forward_site):
    """a declined and an undeclined run of one case (same operands, so the same forward unless the decline is IN the forward)"""
    assert torch.equal(dec["out"], ctl["out"])             # forward sites: the two pool forms return the same bits (test_pool_in_the_forward_epilogue_...)
    if forward_site:                                       # ... and gradients that differ only where two rows of a group tie exactly
        assert rel_err(dec["dX"], ctl["dX"]) < 1e-6
        for a, b in zip(dec["grads"], ctl["grads"]):
            assert rel_err(a, b) < 1e-6
    else:                                                  # test_both_backward_passes_in_one_launch_equal_the_two_pass_form's bound
        for a, b in zip([dec["dX"]] + dec["grads"], [ctl["dX"]] + ctl["grads"]):
            scale = float(b.abs().max())
            assert float((a - b).abs().max()) <= 2e-5 * max(scale, 1e-9), (name, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("name,entry,case,natural,forward_site", DECLINES, ids=[d[0] for d in DECLINES])
def test_declined_launch_by_injection(name, entry, case, natural, forward_site, monkeypatch):
    """the fast entry point answers GSPN_ERR_UNSUPPORTED without launching: the launches mlp.py answers with are held to the float64 reference
    (check_stack_routed) and to the undeclined run of the same case, in which the fast entry point really ran"""
    e = Entry(monkeypatch, entry)
    ctl, ctl_kinds = _run_case(case)
    assert 0 in e.rcs, (entry, e.rcs)                      # the control took the fast launch
    n_ctl = len(e.rcs)
    e.decline = True
    dec, dec_kinds = _run_case(case)
    attempts = len(e.rcs) - n_ctl
    print("%s declined by injection at %s: %d attempt(s); kinds %s (undeclined: %s)" % (entry, case, attempts, sorted(dec_kinds), sorted(ctl_kinds)))
    assert attempts >= 1
    if name.startswith("fused"):
        assert any(k.startswith("fused") for k in ctl_kinds)
        assert len([k for k in dec_kinds if k.startswith("fused")]) < len([k for k in ctl_kinds if k.startswith("fused")])
        assert any(k.startswith("wgrad") for k in dec_kinds)
    _compare_declined(name, dec, ctl, forward_site)


def test_declined_fused_launch_without_the_merged_coefficient_kernel(monkeypatch):
    """the same `except` reached through gspn_mlp_bwd_fused (mlp.FUSED_COEF off)"""
    from gspn_amd import mlp as M
    monkeypatch.setattr(M, "FUSED_COEF", False)
    case = (131072, 8, 6, [32, 32, 64], 32)
    e = Entry(monkeypatch, "gspn_mlp_bwd_fused")
    ctl, ctl_kinds = _run_case(case)
    assert e.rcs and all(rc == 0 for rc in e.rcs) and any(k.startswith("fused") for k in ctl_kinds)
    n_ctl = len(e.rcs)
    e.decline = True
    dec, dec_kinds = _run_case(case)
    print("gspn_mlp_bwd_fused declined by injection at %s: %d attempt(s); kinds %s (undeclined: %s)" % (case, len(e.rcs) - n_ctl, sorted(dec_kinds), sorted(ctl_kinds)))
    assert len(e.rcs) > n_ctl and not any(k.startswith("fused") for k in dec_kinds)
    _compare_declined("fused", dec, ctl, False)


@pytest.mark.parametrize("name,entry,case,natural,forward_site", [d for d in DECLINES if d[3]], ids=[d[0] for d in DECLINES if d[3]])
def test_declined_launch_by_a_misplaced_operand(name, entry, case, natural, forward_site, monkeypatch):
    """the library itself declines: the Python guard in front of the launch says yes, the launcher finds an operand it reads 16 bytes at a
    time on a 4-byte boundary.  Held to float64; and, where only the upstream gradient moved (the forward is then the same launch sequence),
    to the undeclined run on fresh allocations at 2e-5 of each tensor's largest element."""
    e = Entry(monkeypatch, entry)
    ctl, ctl_kinds = _run_case(case)
    assert 0 in e.rcs, (entry, e.rcs)
    n_ctl, ctl_declined = len(e.rcs), e.rcs.count(UNSUPPORTED)
    dec, dec_kinds = _run_case(case, place=natural)
    rcs = e.rcs[n_ctl:]
    print("%s at %s with place=%s: return codes %s; kinds %s (on fresh allocations: %s)" % (entry, case, natural, rcs, sorted(dec_kinds), sorted(ctl_kinds)))
    assert rcs.count(UNSUPPORTED) > ctl_declined, "the launcher took an operand this test meant it to decline"
    if name.startswith("fused"):
        assert any(k.startswith("fused") for k in ctl_kinds)
        assert len([k for k in dec_kinds if k.startswith("fused")]) < len([k for k in ctl_kinds if k.startswith("fused")])
    if natural == "grad":
        _compare_declined(name, dec, ctl, False)
    else:
        print("  (the input moved, so the first layer's forward ran on another kernel: differences reported only) %s" % diffs(dec, ctl))


def test_pooled_top_layer_outside_the_streaming_kernels_lds_budget_is_declined(monkeypatch):
    """gspn_mlp_bwd_data_pooltop declines 64 -> 128 by itself (W diag(cB) W^T, W^T and two row tiles do not fit its LDS budget) behind a Python
    guard that admits it (cin <= 64, cout <= 128): the register-staged pass B answers.  No undeclined run of this shape exists."""
    e = Entry(monkeypatch, "gspn_mlp_bwd_data_pooltop")
    res, kinds = _run_case((2048, 64, 64, [64, 128], 32))
    print("gspn_mlp_bwd_data_pooltop at 2048 x 64 -> 128: return codes %s; kinds %s" % (e.rcs, sorted(kinds)))
    assert e.rcs == [UNSUPPORTED]


# -------------------------------------------------------------------------- 4. the same with gradient sinks, over two steps
def _two_steps(case, place, sinks, fill):
    """two forward / backward / flatten() steps of one stack whose parameters lie behind a 1-element dummy in a FlatGradBucket (every slice
    starts 4 bytes past a multiple of 16 when the sizes before it are multiples of 4).  The bucket is filled with `fill` before the first step and
    not touched between the steps.  Returns the bucket after each step."""
    from gspn_amd import mlp as M
    from gspn_amd import parallel
    rows, ld, cin, chans, ns = case
    g = torch.Generator().manual_seed(rows + cin + 11)
    x0 = torch.randn(rows, ld, generator=g)
    x0[:, cin:] = 0
    gos = [torch.randn(rows // ns if ns else rows, chans[-1], generator=g).cuda() for _ in range(2)]
    layers = to_layers(make_params(chans, cin, seed=cin + 1), place)
    dummy = torch.nn.Parameter(torch.zeros(1, device="cuda"))
    params = [dummy] + [t for lp in layers for t in lp.tensors()]
    bucket = parallel.FlatGradBucket(params)
    res4 = sorted({v.data_ptr() % 16 for v in bucket._views[1:]})
    assert any(r != 0 for r in res4)
    if all(p.numel() % 4 == 0 for p in params[1:]):
        assert res4 == [4], res4
    if sinks:
        bucket.attach_sinks()
    bucket.flat.fill_(fill)
    flats = []
    try:
        for step in range(2):
            for p in params:
                p.grad = None
            x = place_x(x0.cuda(), place)
            out = M.mlp_stack(x, cin, layers, True, 0.7, pool_ns=ns)
            go = place_grad(gos[step], place)
            out.backward(go)
            bucket.flatten()
            torch.cuda.synchronize()
            assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(params, bucket._views))
            flats.append(bucket.flat.clone())
    finally:
        for k in [k for k, e in M.GRAD_SINKS.items() if e.bucket is bucket]:
            del M.GRAD_SINKS[k]
    return flats, res4, params


def _check_sinks(what, case, place, fill):
    kinds = []
    with profiled(kinds):
        plain, _, _ = _two_steps(case, place, False, fill)
    sunk, res4, params = _two_steps(case, place, True, fill)
    print("%s %s place=%s bucket filled with %s: slice residues %s; kinds %s" % (what, case, place, fill, res4, sorted(set(kinds))))
    names = ["dummy"] + ["%s%d" % (n, li) for li in range((len(params) - 1) // 4) for n in ("dW", "dbias", "dbeta", "dgamma")]
    for step in range(2):
        assert torch.isfinite(sunk[step]).all() and torch.isfinite(plain[step]).all(), "step %d: a slice kept the bucket's old content" % step
        if not torch.equal(sunk[step], plain[step]):
            off, bad = 0, []
            for nm, p in zip(names, params):
                if not torch.equal(sunk[step][off:off + p.numel()], plain[step][off:off + p.numel()]):
                    bad.append(nm)
                off += p.numel()
            raise AssertionError("step %d: the bucket written through the sinks differs from the gathered one in %s" % (step, bad))


@pytest.mark.parametrize("fill", [float("nan"), 0.0], ids=["nan", "zero"])
@pytest.mark.parametrize("name,entry,case,natural,forward_site", DECLINES, ids=[d[0] for d in DECLINES])
def test_gradient_sinks_after_a_declined_launch_over_two_steps(name, entry, case, natural, forward_site, fill, monkeypatch):
    """a launch that declines must leave no sink claimed that it did not fill: the bucket written through the sinks is bit-identical to the one
    gathered by `cat`, after each of two steps, on a bucket that still holds the step before (NaN before the first).  A sink left claimed
    shows as NaN after the first step (the late gradient is ADDED onto the unwritten slice) or, from a zero bucket, as last step's gradient
    plus this step's after the second."""
    e = Entry(monkeypatch, entry, decline=True)
    _check_sinks("%s declined by injection" % entry, case, None, fill)
    assert len(e.rcs) >= 4 and all(rc == UNSUPPORTED for rc in e.rcs)      # attempted in every step of both runs
    if natural:
        e.decline = False
        del e.rcs[:]
        _check_sinks("%s declined by the library" % entry, case, natural, fill)
        print("  return codes %s" % e.rcs)
        assert UNSUPPORTED in e.rcs


def test_gradient_sinks_when_the_coefficient_kernel_behind_dense_rsum_declines(monkeypatch):
    """the dense_rsum block of mlp.py claims the top layer's sinks inside _coef_from_parts, under the same `except`: a declining
    gspn_mlp_bwd_coef (its first call of a backward pass is that block's) must hand them back to the two-product pass A"""
    from gspn_amd import _lib as L
    lib = L.lib()
    real = lib.gspn_mlp_bwd_coef
    calls = []

    class FirstOfEachBackwardDeclines:
        def __call__(self, *a):
            first = not calls or calls[-1] == "end"
            calls.append(UNSUPPORTED if first else "ran")
            return UNSUPPORTED if first else real(*a)
    monkeypatch.setattr(lib, "gspn_mlp_bwd_coef", FirstOfEachBackwardDeclines())
    from gspn_amd import parallel
    realf = parallel.FlatGradBucket.flatten
    monkeypatch.setattr(parallel.FlatGradBucket, "flatten", lambda self: (calls.append("end"), realf(self))[1])
    for fill in (float("nan"), 0.0):
        del calls[:]
        _check_sinks("gspn_mlp_bwd_coef declined behind gspn_dense_rsum", (65536, 20, 20, [64, 64, 64], None), None, fill)
        assert calls.count(UNSUPPORTED) == 4 and "ran" in calls


@pytest.mark.parametrize("fill", [float("nan"), 0.0], ids=["nan", "zero"])
def test_gradient_sinks_after_a_declined_fused_launch_without_the_merged_coefficient_kernel(fill, monkeypatch):
    """the gspn_mlp_bwd_fused branch (mlp.FUSED_COEF off) of the same `except`"""
    from gspn_amd import mlp as M
    monkeypatch.setattr(M, "FUSED_COEF", False)
    e = Entry(monkeypatch, "gspn_mlp_bwd_fused", decline=True)
    _check_sinks("gspn_mlp_bwd_fused declined by injection", (131072, 8, 6, [32, 32, 64], 32), None, fill)
    assert len(e.rcs) >= 4 and all(rc == UNSUPPORTED for rc in e.rcs)


@pytest.mark.parametrize("fill", [float("nan"), 0.0], ids=["nan", "zero"])
def test_gradient_sinks_after_the_pooled_top_layer_outside_the_lds_budget_is_declined(fill, monkeypatch):
    e = Entry(monkeypatch, "gspn_mlp_bwd_data_pooltop")
    _check_sinks("gspn_mlp_bwd_data_pooltop declined by the library", (2048, 64, 64, [64, 128], 32), None, fill)
    assert e.rcs == [UNSUPPORTED] * 4


@pytest.mark.parametrize("rows,ld,cin,chans,ns", ROUTED_CASES + [(1024, 768, 768, [256, 256], None)])
def test_gradient_sinks_with_every_operand_misplaced_over_two_steps(rows, ld, cin, chans, ns):
    """the "all" placement of every case above with its gradients written straight into 4-byte-aligned bucket slices"""
    _check_sinks("sinks", (rows, ld, cin, chans, ns), "all", float("nan"))

