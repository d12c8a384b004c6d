"""The shared MLP on stacks whose layers do not all have batch norm.

LayerParams.bn is one flag per layer, and `bn=` is a public argument of both modules and both heads.  A stack that mixes the two kinds of layer
takes host branches of gspn_amd/mlp.py that nothing else reaches (want_rsum = tr_all and prev.bn; bn_dw = 0 if ran_known else int(lp.bn);
gspn_mlp_bwd_fused with part == NULL; the two-product pass A with use_bn = 0 next to a layer whose coefficients arrive early; gradient sinks with
no gamma to claim), and a stack without any batch norm at >= 65536 rows takes the long-layer plans with use_bn = 0.  All of it against float64
(oracle/mlp_ref.py) through the two checkers of tests/test_gpu_mlp.py at their own tolerances: forward 1e-5, routed gradients 1e-5, check_stack
gradients 1e-4, fragile cap 2 %.  Notation: T = batch norm, F = none; a case is (rows, ld, cin, chans, pool)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import mlp_ref as R
from oracle import oracle as O
from tests import data as D
from tests.test_gpu_mlp import check_stack, check_stack_routed, make_params, place_grad, place_x, to_layers
from tests.test_gpu_mlp_unaligned import UNSUPPORTED, Entry, diffs, profiled
from tests.test_gpu_modules import fresh_store, rel_err
from tests.test_gpu_sa_variants import ref_sa

pytestmark = pytest.mark.gpu

T, F = True, False


class FusedEntry(Entry):
    """gspn_mlp_bwd_fused, passed on; keeps the `part` pointer of every call (argument 16 of the entry point: None when it is NULL)"""

    def __init__(self, monkeypatch):
        self.parts = []
        Entry.__init__(self, monkeypatch, "gspn_mlp_bwd_fused")

    def __call__(self, *args):
        assert len(args) == 19
        self.parts.append(args[16].value)
        return Entry.__call__(self, *args)


# --------------------------------------------------------------------- a. the fused backward with no reductions to carry
@pytest.mark.parametrize("ns", [None, 32])
@pytest.mark.parametrize("c1", [32, 64, 128])
@pytest.mark.parametrize("c0", [32, 64])
def test_fused_backward_over_a_layer_without_batch_norm(c0, c1, ns, monkeypatch):
    """[F, T] at 65536 rows: layer 1 gets its coefficients early (gspn_dense_rsum, resp. gspn_pool_rsum for the pooled top) and goes through
    gspn_mlp_bwd_fused with part = NULL, because the layer below has no reductions to take -- bwd_fused_kernel<c0 / 32, c1 / 32, false, ns == 32>.
    Layer 0 then runs the two-product pass A with use_bn = 0.  Every gradient at 1e-5, nothing silenced; the fused entry point must have been
    called exactly once, with a NULL part, and must have taken the launch."""
    e = FusedEntry(monkeypatch)
    kinds = []
    with profiled(kinds):
        check_stack_routed(65536, 8, 6, [c0, c1], ns, bn=[F, T])
    print("gspn_mlp_bwd_fused at [%d, %d] pool %s: return codes %s, part pointers %s; kinds %s" % (c0, c1, ns, e.rcs, e.parts, sorted(kinds)))
    assert e.rcs == [0]
    assert e.parts == [None]
    assert "fused:%d->%d" % (c0, c1) in kinds and "wgrad:6->%d" % c0 in kinds


# ------------------------------------------------------------------------------- c. mixed stacks on the short-layer plans
SHORT = [(4096, 8, 6, [32, 32, 64], 32), (1000, 67, 67, [64, 64, 64], None)]
PATTERNS = [[T, F, T], [F, T, F], [T, T, F], [F, F, T]]


def _pid(bn):
    return "".join("T" if v else "F" for v in bn)


@pytest.mark.parametrize("bn", PATTERNS, ids=_pid)
@pytest.mark.parametrize("rows,ld,cin,chans,ns", SHORT)
def test_mixed_stack_training_gradients_with_the_gpu_forward_s_own_routing(rows, ld, cin, chans, ns, bn):
    check_stack_routed(rows, ld, cin, chans, ns, bn=bn)


@pytest.mark.parametrize("bn", PATTERNS, ids=_pid)
@pytest.mark.parametrize("rows,ld,cin,chans,ns", SHORT)
def test_mixed_stack_in_evaluation_mode(rows, ld, cin, chans, ns, bn):
    check_stack(rows, ld, cin, chans, ns, False, bn=bn)


# ---------------------------------------------------------------------------- d. no batch norm at all on the long-layer plans
LONG = [(65536, 68, 67, [64, 64, 128], 32), (65536, 8, 6, [64, 64, 64], None), (131072, 8, 6, [32, 64], None)]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("rows,ld,cin,chans,ns", LONG)
def test_long_stack_without_batch_norm(rows, ld, cin, chans, ns, training):
    """the >= 65536-row forward kernels, the lean pass B and the streaming pass A with use_bn = 0; a stack without batch norm has no batch
    statistics, so both modes compute the same values -- through different host branches (is_training reaches every backward launch)"""
    check_stack(rows, ld, cin, chans, ns, training, ref_device="cuda", bn=False)


# ------------------------------------------------------------------------------------------ e. operand placement and sinks
MIXED = (65536, 8, 6, [64, 64], None)


def test_mixed_stack_with_every_operand_misplaced(monkeypatch):
    """the dense 64 -> 64 case of (a) with every operand 4-byte aligned only.  The fused launch reads the upstream gradient as quads, and so does
    gspn_dense_rsum in front of it, which hands it its coefficients: with d_out misplaced the pre-pass declines first, mlp.py then never offers the
    layer to gspn_mlp_bwd_fused (no known coefficients), and both layers run pass A + pass B -- layer 1 the two-product pass with use_bn = 1,
    layer 0 with use_bn = 0.  Held to float64 at 1e-5 like the aligned run; the difference between the two runs is printed (the first layer's
    forward runs on another kernel, so a ReLU at the kink may route differently, which the routed reference absorbs)."""
    rows, ld, cin, chans, ns = MIXED
    fused, rsum = FusedEntry(monkeypatch), Entry(monkeypatch, "gspn_dense_rsum")
    ctl, ctl_kinds = {}, []
    with profiled(ctl_kinds):
        check_stack_routed(rows, ld, cin, chans, ns, bn=[F, T], results=ctl)
    assert fused.rcs == [0] and fused.parts == [None] and rsum.rcs == [0]
    del fused.rcs[:], rsum.rcs[:]
    res, kinds = {}, []
    with profiled(kinds):
        check_stack_routed(rows, ld, cin, chans, ns, bn=[F, T], place="all", results=res)
    print("place=all: gspn_dense_rsum %s, gspn_mlp_bwd_fused %s; kinds %s (aligned: %s); differences from the aligned run %s"
          % (rsum.rcs, fused.rcs, sorted(kinds), sorted(ctl_kinds), diffs(res, ctl)))
    assert UNSUPPORTED in rsum.rcs + fused.rcs                     # the library declined by itself
    assert 0 not in fused.rcs and not any(k.startswith("fused") for k in kinds)
    assert "wgrad:64->64" in kinds and "bwd:64->64" in kinds       # the two-pass form answered


def _two_steps(sinks):
    """two forward / backward / flatten() steps of the [F, T] stack with its six parameters in a FlatGradBucket that holds NaN before each
    step; returns the bucket after each step.  Input, parameters and the first step's upstream gradient are check_stack_routed's own (same
    generators, same draw order), so the first step repeats the run that checker holds to float64."""
    from gspn_amd import mlp as M
    from gspn_amd import parallel
    rows, ld, cin, chans, ns = MIXED
    g = torch.Generator().manual_seed(rows + cin + 1)
    x0 = torch.randn(rows, ld, generator=g, dtype=torch.float64)
    x0[:, cin:] = 0
    x0 = x0.float()
    gos = [torch.randn(rows, chans[-1], generator=g, dtype=torch.float64).float().cuda() for _ in range(2)]
    layers = to_layers(make_params(chans, cin, seed=cin + 1, bn=[F, T]))
    params = [t for lp in layers for t in lp.tensors()]
    assert len(params) == 6                                        # w, b | w, b, beta, gamma: no slot for a gamma that does not exist
    bucket = parallel.FlatGradBucket(params)
    if sinks:
        bucket.attach_sinks()
    flats = []
    try:
        for step in range(2):
            bucket.flat.fill_(float("nan"))
            for p in params:
                p.grad = None
            x = place_x(x0.cuda(), None)
            out = M.mlp_stack(x, cin, layers, True, 0.7, pool_ns=ns)
            out.backward(place_grad(gos[step], None))
            if sinks:                                              # every gradient went straight into its slice: autograd got none of them, .grad IS the slice
                assert len(bucket._written) == len(params)
                assert all(p.grad is not None and p.grad.data_ptr() == v.data_ptr() for p, v in zip(params, bucket._views))
            bucket.flatten()
            torch.cuda.synchronize()
            assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(params, bucket._views))
            flats.append(bucket.flat.clone())
    finally:
        for k in [k for k, e in M.GRAD_SINKS.items() if e.bucket is bucket]:
            del M.GRAD_SINKS[k]
    return flats, params


def test_gradient_sinks_of_a_mixed_stack_over_two_steps(monkeypatch):
    """FlatGradBucket.attach_sinks() on the [F, T] stack: the bucket written through the sinks is bit-identical to the one gathered by `cat`,
    after each of two steps, from a bucket that holds NaN before each.  A slot claimed for the gamma / beta the first layer does not have, or a
    slot left unwritten (the no-BN layer's bias comes out of the two-product pass A, the other layer's out of the coefficient kernel), shows as
    NaN or as a difference.  The first step is the run check_stack_routed holds to float64 (its results= hook): both buckets equal its gradients."""
    e = FusedEntry(monkeypatch)
    ctl = {}
    check_stack_routed(*MIXED, bn=[F, T], results=ctl)
    plain, params = _two_steps(False)
    sunk, _ = _two_steps(True)
    assert e.rcs == [0] * 5 and e.parts == [None] * 5              # the fused launch with no reductions, in every step of every run
    assert torch.equal(plain[0], torch.cat([t.reshape(-1) for t in ctl["grads"]]))
    names = ["dW0", "dbias0", "dW1", "dbias1", "dbeta1", "dgamma1"]
    for step in range(2):
        assert torch.isfinite(plain[step]).all() and torch.isfinite(sunk[step]).all(), "step %d: a slice kept the NaN it was filled with" % step
        off, bad = 0, []
        for nm, p in zip(names, params):
            if not torch.equal(sunk[step][off:off + p.numel()], plain[step][off:off + p.numel()]):
                bad.append(nm)
            off += p.numel()
        assert not bad, "step %d: the bucket written through the sinks differs from the gathered one in %s" % (step, bad)
    assert not torch.equal(plain[0], plain[1])                     # (two different upstream gradients: the second step really rewrote it)


# --------------------------------------------------------------------------------------------------------------- f. modules
def _random_biases(store, seed):
    """the store initialises biases to 0: give the ones created so far values, so that the forward's bias add is compared too"""
    g = torch.Generator().manual_seed(seed)
    n = 0
    for k, v in store.vars.items():
        if k.endswith("/biases"):
            v.data.copy_(((torch.rand(v.shape, generator=g) - 0.5) * 0.2).to(v.device))
            n += 1
    return n


@pytest.mark.parametrize("training", [True, False])
def test_sa_module_without_batch_norm_through_the_gathering_front_end(training):
    """pointnet_sa_module(bn=False) at SA2's shape, 16384 grouped rows: mlp_stack(gather=) takes layers without batch norm, the pre-aggregated
    first layer does not (preagg_ok), so the first layer gathers its rows and its backward is gspn_mlp_bwd_wgrad_gather with use_bn = 0.
    Against the float64 composition on oracle geometry: output 1e-5; weights, BIASES (the one parameter gradient that differs in kind from the
    batch-normalised case) and the feature gradient 1e-4."""
    from gspn_amd import mlp as M
    from gspn_amd import pointnet_util as PU
    from gspn_amd import tf_util
    from gspn_amd.geometry import sa_geometry
    kind, b, n, c, npoint, radius, ns, mlp = "U", 2, 2048, 64, 256, 0.4, 32, [64, 64, 128]
    xyz = D.batch(kind, b, n, 6)
    pts = np.random.default_rng(12).standard_normal((b, n, c)).astype(np.float32)
    tx = torch.from_numpy(xyz).cuda()
    tp = torch.from_numpy(pts).cuda().requires_grad_(True)
    store = fresh_store(55)
    with tf_util.variable_scope('sa'):
        layers = PU._mlp_layers(mlp, 3 + c, 'conv', False)         # the module's own variables, created ahead of its call
    assert _random_biases(store, 8) == len(mlp)
    assert not M.preagg_ok(layers, training, c)
    geo = sa_geometry(tx, npoint, radius, ns)
    assert PU._sa_stack_gathered(tp.detach(), geo, True, 3 + c, layers, training, 0.5, ns) is not None
    nvars = len(store.vars)
    new_xyz, new_points, idx = PU.pointnet_sa_module(tx, tp, npoint, radius, ns, mlp, None, False, training, 0.5, 'sa', bn=False)
    assert len(store.vars) == nvars                                # the module found the variables above
    rnew, ref, ridx, leaves = ref_sa(store, 'sa', xyz, pts, npoint, radius, ns, mlp, None, False, 'max', False, True, 0.5, bn=False)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    assert rel_err(new_points, ref) < 1e-5
    g = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(ref.shape)))
    ref.backward(g)
    new_points.backward(g.float().cuda())
    for i, p in enumerate(leaves["ps"]):
        assert rel_err(store.vars['sa/conv%d/weights' % i].grad.view(p["w"].shape), p["w"].grad) < 1e-4, i
        assert rel_err(store.vars['sa/conv%d/biases' % i].grad, p["b"].grad) < 1e-4, i
    assert rel_err(tp.grad, leaves["pts"].grad) < 1e-4


@pytest.mark.parametrize("training", [True, False])
def test_fp_module_without_batch_norm(training):
    """pointnet_fp_module(bn=False) at the first shape of test_fp_module_matches_oracle (4096 dense rows of 192 columns, 192 -> 128 -> 64),
    against that test's float64 composition: output 1e-5; weights, biases and both feature gradients 1e-4"""
    from gspn_amd import pointnet_util as PU
    from gspn_amd import tf_util
    b, n1, n2, c1, c2, mlp = 2, 2048, 512, 64, 128, [128, 64]
    store = fresh_store(99)
    with tf_util.variable_scope('fa'):
        PU._mlp_layers(mlp, c1 + c2, 'conv_', False)
    assert _random_biases(store, 9) == len(mlp)
    xyz1 = D.batch("D", b, n1, 3)
    xyz2 = O.gather_point(xyz1, O.farthest_point_sample(n2, xyz1))
    rng = np.random.default_rng(17)
    p1 = rng.standard_normal((b, n1, c1)).astype(np.float32)
    p2 = rng.standard_normal((b, n2, c2)).astype(np.float32)
    t1 = torch.from_numpy(p1).cuda().requires_grad_(True)
    t2 = torch.from_numpy(p2).cuda().requires_grad_(True)
    nvars = len(store.vars)
    out = PU.pointnet_fp_module(torch.from_numpy(xyz1).cuda(), torch.from_numpy(xyz2).cuda(), t1, t2, mlp, training, 0.5, 'fa', bn=False)
    assert len(store.vars) == nvars
    rd, ri = O.three_nn(xyz1, xyz2)
    w64 = R.fp_weights(torch.from_numpy(rd).double())
    p2r = torch.from_numpy(p2).double().requires_grad_(True)
    p1r = torch.from_numpy(p1).double().requires_grad_(True)
    gi = torch.from_numpy(ri.astype(np.int64))
    bi = torch.arange(b)[:, None, None].expand_as(gi)
    cat = torch.cat([(p2r[bi, gi] * w64[..., None]).sum(2), p1r], 2)
    ps = []
    for i in range(len(mlp)):
        w = store.vars['fa/conv_%d/weights' % i].detach().double().cpu()
        ps.append({"w": w.view(w.shape[-2], w.shape[-1]).clone().requires_grad_(True),
                   "b": store.vars['fa/conv_%d/biases' % i].detach().double().cpu().clone().requires_grad_(True), "bn": False})
    ref, _ = R.stack(cat.reshape(b * n1, -1), ps, training, 0.5, None)
    ref = ref.view(b, n1, mlp[-1])
    assert rel_err(out, ref) < 1e-5
    g = torch.from_numpy(rng.standard_normal(ref.shape)).double()
    ref.backward(g)
    out.backward(g.float().cuda())
    for i, p in enumerate(ps):
        assert rel_err(store.vars['fa/conv_%d/weights' % i].grad.view(p["w"].shape), p["w"].grad) < 1e-4, i
        assert rel_err(store.vars['fa/conv_%d/biases' % i].grad, p["b"].grad) < 1e-4, i
    assert rel_err(t2.grad, p2r.grad) < 1e-4
    assert rel_err(t1.grad, p1r.grad) < 1e-4


# --------------------------------------------------------------------------------------- g. gspn_mlp_bwd_data alone, on a column range
# Which kernel a plain call of gspn_mlp_bwd_data (no dW job, no BN reductions) gets, read off bwd_data_launch, bwd_lean_try and pick_bn (csrc/mlp.hip):
#   * bwd_lean_kernel takes the launch unless rows % 128, cout % 32, ncols % 32 or col0 % 4 is non-zero (or an operand is not 16-byte aligned);
#     every case below has cout % 32 != 0 and ncols % 32 != 0, so mlp_bwd_data_kernel<BN, V, P, false> runs (false: no dW job rides along);
#   * BN = pick_bn(rows, ncols): 32 up to 32 columns; 64 up to 64 columns and 128 beyond, each only while the grid still has 2 * GSPN_PLAN_CUS = 448
#     workgroups of 128 rows (65536 rows: 512) and the narrower tile does not pad markedly fewer columns (100 columns: 128 against 2 x 64, equal);
#   * V (16-byte accesses) needs Y's and dZ's pitch and cout (W's pitch) to be multiples of 4 and the pointers aligned: cout = 20 is the vector
#     form, cout = 18 the scalar one;   * P: the upstream gradient is that of a max-pool (dPool, pool_arg, ns) instead of a dense dZ.
DATA_COLS = [  # (BN, rows, ncols, cout, pooled)
    (128, 65536, 100, 20, False), (128, 65536, 100, 18, False), (128, 65536, 100, 20, True), (128, 65536, 100, 18, True),
    (64, 65536, 48, 20, True), (64, 65536, 48, 18, True),
    (32, 2080, 24, 18, True),                                      # 16 full 128-row tiles and one of 32 rows
]


@pytest.mark.parametrize("bn_tile,rows,ncols,cout,pooled", DATA_COLS)
def test_bwd_data_cols_entry_point_against_float64(bn_tile, rows, ncols, cout, pooled):
    """gspn_mlp_bwd_data (plain form, a column range) through the C ABI with a hand-built gspn_dy_args and padded pitches: columns [col0, col0 + ncols) of
    dX = dY . W^T, dY = cA*[relu open]*dz + cB*y + cC, against float64 on the device at 2e-5 of the largest element; every other column of dX
    keeps what it held.  The seven mlp_bwd_data_kernel<BN, V, P, false> instantiations no stack or module selects (see DATA_COLS)."""
    from gspn_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(rows + 7 * ncols + cout + int(pooled))
    vec = cout % 4 == 0
    col0, ns = 4, 32
    cin = col0 + ncols + 2                                         # two columns past the range, and a pitch wider still
    ldx = cin + 4
    ldy, ldz = (cout + 4, cout + 8) if vec else (cout + 3, cout + 5)
    Yb = torch.randn(rows, ldy, device=dev, generator=g); Y = Yb[:, :cout]
    W = torch.randn(cin, cout, device=dev, generator=g) * 0.1
    rnd = lambda lo, hi: torch.rand(cout, device=dev, generator=g) * (hi - lo) + lo
    scale, shift = rnd(0.5, 1.5), rnd(-0.3, 0.3)
    cA, cB, cC = rnd(0.5, 1.5), rnd(-0.01, 0.01), rnd(-0.01, 0.01)
    a = L.DyArgs()
    a.Y, a.ldy = Yb.data_ptr(), ldy
    a.scale, a.shift, a.cA, a.cB, a.cC = scale.data_ptr(), shift.data_ptr(), cA.data_ptr(), cB.data_ptr(), cC.data_ptr()
    if pooled:
        assert rows % ns == 0
        dP = torch.randn(rows // ns, cout, device=dev, generator=g)
        arg = torch.randint(0, ns, (rows // ns, cout), device=dev, dtype=torch.int32, generator=g)
        a.dZ, a.ldz, a.dPool, a.pool_arg, a.ns = None, 0, dP.data_ptr(), arg.data_ptr(), ns
        dz = torch.zeros(rows // ns, ns, cout, device=dev, dtype=torch.float64)
        dz.scatter_(1, arg.long().unsqueeze(1), dP.double().unsqueeze(1))
        dz = dz.view(rows, cout)
    else:
        Zb = torch.randn(rows, ldz, device=dev, generator=g)
        a.dZ, a.ldz, a.dPool, a.pool_arg, a.ns = Zb.data_ptr(), ldz, None, None, 0
        dz = Zb[:, :cout].double()
    assert (Yb.data_ptr() | W.data_ptr()) % 16 == 0
    dXb = torch.full((rows, ldx), 7.0, device=dev)
    L.check(lib.gspn_mlp_bwd_data(rows, cin, cout, ctypes.byref(a), L.ptr(W), col0, ncols, L.ptr(dXb), ldx, None, None, L.stream()), "bwd_data")
    torch.cuda.synchronize()
    # the mask with the float32 expression the kernel uses, so that no element sits on the other side of the kink
    dyh = torch.where((Y * scale + shift) > 0, dz, torch.zeros_like(dz))
    dY = cA.double() * dyh + cB.double() * Y.double() + cC.double()
    rdX = dY @ W[col0:col0 + ncols].double().t()
    err = rel_err(dXb[:, col0:col0 + ncols], rdX)
    print("gspn_mlp_bwd_data %d x [%d, %d) <- %d, tile %d, %s, %s: %.3g" % (rows, col0, col0 + ncols, cout, bn_tile, "vector" if vec else "scalar",
                                                                                "pooled" if pooled else "dense", err))
    assert err < 2e-5
    assert bool((dXb[:, :col0] == 7.0).all()) and bool((dXb[:, col0 + ncols:] == 7.0).all())


# ------------------------------------------------------------------------- h. the four forms of gspn_mlp_bwd_data on one layer
@pytest.mark.parametrize("pooled", [False, True], ids=["dense", "pooled"])
def test_bwd_data_four_forms_agree_and_carry_their_jobs(pooled):
    """One layer 24 -> 20 at 2080 rows (16 full 128-row tiles and one of 32 rows), whole row, padded pitches, after gspn_mlp_bwd_wgrad(dW = NULL)
    has filled `work`: gspn_mlp_bwd_data plain, with the dW job, with the previous layer's BN reductions, with both.  dX is the same bits in all
    four (include/gspn_hip.h) and within test g's 2e-5 of float64; dW of the riding job within 2e-5 of float64's largest element (test g's bound,
    the same GEMM family); the rows of `part`, summed in float64, equal sum(dyh) and sum(dyh * xhat) of the layer below at 1e-5 of the largest
    element (check_stack_routed's bound on dbeta / dgamma, which these sums are up to gamma * rstd)."""
    from gspn_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2080 + int(pooled))
    rows, cin, cout, ns, eps = 2080, 24, 20, 32, 1e-3
    ldx, ldxin, ldy, ldz = cin + 4, cin + 8, cout + 4, cout + 8
    Xb = torch.randn(rows, ldxin, device=dev, generator=g); X = Xb[:, :cin]            # the layer's input = the pre-BN output of the layer below
    Yb = torch.randn(rows, ldy, device=dev, generator=g); Y = Yb[:, :cout]
    W = torch.randn(cin, cout, device=dev, generator=g) * 0.1
    rnd = lambda n, lo, hi: torch.rand(n, device=dev, generator=g) * (hi - lo) + lo
    in_scale, in_shift = rnd(cin, 0.5, 1.5), rnd(cin, -0.3, 0.3)
    mean_p, var_p = X.mean(0).contiguous(), X.var(0, unbiased=False).contiguous()
    gamma, beta = rnd(cout, 0.5, 1.5), rnd(cout, -0.3, 0.3)
    mean, var = Y.mean(0).contiguous(), Y.var(0, unbiased=False).contiguous()
    rstd = 1.0 / torch.sqrt(var.double() + eps)
    scale = (gamma.double() * rstd).float()
    shift = (beta.double() - mean.double() * gamma.double() * rstd).float()
    cA, cB, cC = (torch.empty(cout, device=dev) for _ in range(3))
    a = L.DyArgs()
    a.Y, a.ldy = Yb.data_ptr(), ldy
    a.scale, a.shift, a.cA, a.cB, a.cC = scale.data_ptr(), shift.data_ptr(), cA.data_ptr(), cB.data_ptr(), cC.data_ptr()
    if pooled:
        dP = torch.randn(rows // ns, cout, device=dev, generator=g)
        arg = torch.randint(0, ns, (rows // ns, cout), device=dev, dtype=torch.int32, generator=g)
        a.dZ, a.ldz, a.dPool, a.pool_arg, a.ns = None, 0, dP.data_ptr(), arg.data_ptr(), ns
        dz = torch.zeros(rows // ns, ns, cout, device=dev, dtype=torch.float64)
        dz.scatter_(1, arg.long().unsqueeze(1), dP.double().unsqueeze(1))
        dz = dz.view(rows, cout)
    else:
        Zb = torch.randn(rows, ldz, device=dev, generator=g)
        a.dZ, a.ldz, a.dPool, a.pool_arg, a.ns = Zb.data_ptr(), ldz, None, None, 0
        dz = Zb[:, :cout].double()
    st = L.stream()
    work = torch.empty(int(lib.gspn_mlp_bwd_work_bytes(rows, cin, cout)) // 4, device=dev)
    L.check(lib.gspn_mlp_bwd_wgrad(rows, cin, cout, ctypes.byref(a), L.ptr(Xb), ldxin, L.ptr(in_scale), L.ptr(in_shift), L.ptr(mean), L.ptr(var), L.ptr(gamma),
                                   eps, 1, 1, L.ptr(work), L.ptr(cA), L.ptr(cB), L.ptr(cC), None, None, None, None, st), "bwd_wgrad")
    dX, dW, part, npart = {}, {}, {}, {}
    for form in ("plain", "dw", "rs", "both"):
        dX[form] = torch.full((rows, ldx), 7.0, device=dev)
        dw = rs = None
        if form in ("dw", "both"):
            dW[form] = torch.full((cin, cout), 7.0, device=dev)
            dw = L.DwArgs(L.ptr(Xb), ldxin, L.ptr(var), L.ptr(gamma), eps, 1, 1, L.ptr(work), L.ptr(dW[form]))
        if form in ("rs", "both"):
            part[form] = torch.zeros(int(lib.gspn_rsum_part_floats(rows, cin)), device=dev)
            npart[form] = ctypes.c_int(0)
            rs = L.RsumArgs(L.ptr(Xb), ldxin, L.ptr(in_scale), L.ptr(in_shift), L.ptr(mean_p), L.ptr(var_p), eps, L.ptr(part[form]), ctypes.pointer(npart[form]))
        L.check(lib.gspn_mlp_bwd_data(rows, cin, cout, ctypes.byref(a), L.ptr(W), 0, cin, L.ptr(dX[form]), ldx, ctypes.byref(dw) if dw is not None else None,
                                      ctypes.byref(rs) if rs is not None else None, st), "bwd_data(%s)" % form)
    torch.cuda.synchronize()
    for form in ("dw", "rs", "both"):
        assert torch.equal(dX[form], dX["plain"]), form
    assert bool((dX["plain"][:, cin:] == 7.0).all())
    # float64, the masks with the float32 expressions the kernels use (no element on the other side of a kink)
    dyh = torch.where((Y * scale + shift) > 0, dz, torch.zeros_like(dz))
    rdX = (cA.double() * dyh + cB.double() * Y.double() + cC.double()) @ W.double().t()
    err = rel_err(dX["plain"][:, :cin], rdX)
    open_p = (X * in_scale + in_shift) > 0
    act = torch.where(open_p, X.double() * in_scale.double() + in_shift.double(), torch.zeros_like(rdX))
    xhat = (Y.double() - mean.double()) * rstd
    r0, r1 = dyh.sum(0), (dyh * xhat).sum(0)
    rdW = (gamma.double() * rstd) * (act.t() @ dyh - act.sum(0)[:, None] * (r0 / rows) - (act.t() @ xhat) * (r1 / rows))
    dyh_p = torch.where(open_p, rdX, torch.zeros_like(rdX))
    xhat_p = (X.double() - mean_p.double()) / torch.sqrt(var_p.double() + eps)
    rsum = torch.stack([dyh_p.sum(0), (dyh_p * xhat_p).sum(0)])
    errs_w = {f: rel_err(dW[f], rdW) for f in dW}
    errs_p = {}
    for f in part:
        n = npart[f].value
        assert 0 < n and n * 2 * cin <= part[f].numel()
        got = part[f][:n * 2 * cin].view(n, 2, cin).double().sum(0)
        errs_p[f] = (rel_err(got[0], rsum[0]), rel_err(got[1], rsum[1]))
    print("gspn_mlp_bwd_data four forms, %s: dX %.3g; dW %s; part %s (%s rows)" % ("pooled" if pooled else "dense", err, errs_w, errs_p,
                                                                                   {f: npart[f].value for f in npart}))
    assert err < 2e-5
    assert all(e < 2e-5 for e in errs_w.values())
    assert all(e0 < 1e-5 and e1 < 1e-5 for e0, e1 in errs_p.values())
