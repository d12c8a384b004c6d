"""Every shared-MLP kernel instantiation the launchers of csrc/mlp.hip and csrc/mlp_short.hip can select, at the smallest shape that selects
it, against float64 (profiles/kernel_coverage_mlp.txt records which instantiation each group of cases reaches; tools/kernel_coverage.py
measures it from a kernel trace of this suite).

Forward: gspn_mlp_fwd / gspn_mlp_fwd_pool32 called directly, checked by check_forward -- the body of
tests/test_gpu_mlp_short.py::test_short_forward_against_fp64 with its shape, alignment and pitches as parameters, at that test's tolerances
(BASELINE.json north_star: 1e-5).  The tile shapes and kernels a tuning switch alone selects run the same checker in a child process (the
switches are read once per process).
Backward: stacks through check_stack_routed / check_stack of tests/test_gpu_mlp.py, one row per instantiation the default environment
selects."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_forward(rows, cin, cout, act, pool, aligned=True, padx=4, pady=4, tile_rows=None):
    """Y = act(X) . W + bias of one layer against a float64 product of the two-rounding fp32 activation relu(x*scale + shift):
    Y within 1e-5 of max |ref|, Y's pad columns untouched, every partial statistics row written and finite, their sums within 1e-5 of
    sum y and sum y^2; with `pool` the 32-row groups' maxima of the kernel's own Y bit for bit, and the FIRST row that reaches each
    (include/gspn_hip.h: the pool's arg is the row offset of the first maximum, and gspn_pool32_select hands amax on as that arg).
    aligned=False: X starts 4 bytes past a 16-byte boundary (the vector-load kernels must decline it).
    tile_rows: the launch has more partial statistics rows than tiles of this many rows (workgroup i takes tile i): the surplus rows are zero."""
    from gspn_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(rows + cin)
    ldx, ldy = cin + padx, cout + pady
    X = torch.randn(rows, ldx, device=dev, generator=gen)                     # padded pitch: ldx > cin
    W = torch.randn(cin, cout, device=dev, generator=gen) / cin ** 0.5
    bias = torch.randn(cout, device=dev, generator=gen) * 0.1
    sc = (torch.rand(cin, device=dev, generator=gen) + 0.5) if act else None
    sh = (torch.randn(cin, device=dev, generator=gen) * 0.3) if act else None
    if act:
        sc[::7] = -sc[::7]                                                    # negative scales are legal (gamma < 0)
    Y = torch.full((rows, ldy), float("nan"), device=dev)                    # ldy > cout: the pad columns must stay untouched
    nst = int(lib.gspn_mlp_fwd_stats_bytes(rows, cout)) // 4
    assert nst > 0 and nst % (2 * cout) == 0
    stats = torch.full((nst,), float("nan"), device=dev)
    if pool:
        X = (torch.round(X * 2) / 2).contiguous()                             # quantised inputs and weights: tied maxima inside a pool group occur
        W = (torch.round(W * 8) / 8).contiguous()
    if not aligned:
        buf = torch.empty(X.numel() + 4, device=dev)
        Xm = buf[1:1 + X.numel()].view_as(X)
        Xm.copy_(X)
        X = Xm
        assert X.data_ptr() % 16 == 4 and X.is_contiguous()
    vmax = torch.full((rows // 32, cout), float("nan"), device=dev) if pool else None
    amax = torch.full((rows // 32, cout), -1, dtype=torch.int32, device=dev) if pool else None
    st = L.stream()
    if pool:
        L.check(lib.gspn_mlp_fwd_pool32(rows, cin, cout, L.ptr(X), ldx, L.ptr(sc), L.ptr(sh), L.ptr(W), L.ptr(bias), L.ptr(Y), ldy, L.ptr(stats),
                                        L.ptr(vmax), L.ptr(amax), st), "fwd")
    else:
        L.check(lib.gspn_mlp_fwd(rows, cin, cout, L.ptr(X), ldx, L.ptr(sc), L.ptr(sh), L.ptr(W), L.ptr(bias), L.ptr(Y), ldy, L.ptr(stats), st), "fwd")
    torch.cuda.synchronize()
    A = X[:, :cin]
    A = torch.relu((A * sc + sh).double()) if act else A.double()            # two fp32 roundings, as tf.nn.batch_normalization's x*scale + shift
    ref = A @ W.double() + bias.double()
    got = Y[:, :cout]
    assert bool(torch.isnan(Y[:, cout:]).all())
    err = float((got.double() - ref).abs().max()) / float(ref.abs().max())
    parts = stats.view(-1, 2, cout).double()
    assert bool(torch.isfinite(parts).all())
    if tile_rows:
        ntiles = (rows + tile_rows - 1) // tile_rows
        assert parts.shape[0] > ntiles and bool((parts[ntiles:] == 0).all())     # a workgroup without a tile writes a zero row, exactly
    tot = parts.sum(0)
    e1 = float((tot[0] - ref.sum(0)).abs().max()) / float(ref.abs().sum(0).max())
    e2 = float((tot[1] - (ref * ref).sum(0)).abs().max()) / float((ref * ref).sum(0).max())
    print("check_forward %d x %d -> %d act=%d pool=%d aligned=%d: Y %.2e  sum y %.2e  sum y^2 %.2e (of 1e-5)" % (rows, cin, cout, act, pool, aligned, err, e1, e2))
    assert err <= 1e-5 and e1 <= 1e-5 and e2 <= 1e-5
    if pool:
        g = got.reshape(rows // 32, 32, cout)
        mx = g.max(1).values
        assert torch.equal(vmax, mx)
        assert int(amax.min()) >= 0 and int(amax.max()) < 32
        assert torch.equal(g.gather(1, amax.long().unsqueeze(1)).squeeze(1), mx)          # amax names a row that holds the maximum ...
        first = (g == mx.unsqueeze(1)).float().argmax(1).int()                # ... the FIRST one (the reference's strict '>')
        assert torch.equal(amax, first)


AP = [(False, False), (True, False), (False, True), (True, True)]


def _ap(shapes):
    return [s + ap for s in shapes for ap in AP]


# (rows / 32) * (cout / 32) > 2048 32 x 32 tiles: gspn_fwd_short_go widens the workgroup's tile (MT, NT) -- mlp_short.hip
SHORT_12 = [(8192, c, 320) for c in (64, 128, 192, 256, 384)] + [(4096, 128, 576)]                       # fwd_short_kernel<KW, 1, 2>
SHORT_21 = [(8192, c, 288) for c in (64, 128, 192)]                                                      # <KW, 2, 1>: cout no multiple of 64
SHORT_22 = [(8192, c, 576) for c in (64, 128, 192)] + [(8192, 64, 1024)]                                 # <KW, 2, 2>
# MT = 2 needs cin <= 192 (the staged A tile): wider inputs stay at (1, 1) / (1, 2) whatever the tile count
SHORT_WIDE = [(8192, 256, 288), (8192, 384, 576)]
# <KW, 1, 1>: one tile, and the largest short layer
SHORT_11 = [(64, c, 96) for c in (64, 128, 192, 256, 384)] + [(8192, c, 64) for c in (64, 128, 192, 256, 384)]


@pytest.mark.parametrize("rows,cin,cout,act,pool", _ap(SHORT_12 + SHORT_WIDE + SHORT_11))
def test_short_forward_tile_shapes(rows, cin, cout, act, pool):
    check_forward(rows, cin, cout, act, pool)


@pytest.mark.parametrize("rows,cin,cout,act,pool", _ap(SHORT_21 + SHORT_22))
def test_short_forward_two_row_tiles(rows, cin, cout, act, pool):
    """MT = 2: rows / 32 workgroups for rows / 64 tiles -- the second half of the workgroups has no tile and writes a zero statistics row"""
    check_forward(rows, cin, cout, act, pool, tile_rows=64)


def pitch4(cin):
    """the pad that makes ldx = cin + pad a multiple of 4 floats (16-byte rows: what the vector-load kernels need of the pitch)"""
    return (-cin) % 4 or 4


# mlp_fwd_stream_kernel<BN, TRG, false, false>: stream_plan by (cin, cout).  16-byte rows (pitch4), cin with and without a K tail (cin % 4), rows no
# multiple of the 32 TRG-row tile (pooled: of 32 only)
STREAM = [(1000, 20, 100), (4096 + 32, 6, 128),           # <128, 4>: cin <= 32, cout > 64
          (1000, 67, 128), (1056, 76, 100),               # <128, 2>: 33 <= cin <= 76
          (1000, 20, 32), (1056, 43, 20),                 # <32, 4>:  cin <= 44, cout <= 32
          (1000, 6, 64), (1056, 40, 33),                  # <64, 4>:  cin <= 40, 33 <= cout <= 64
          (1000, 67, 64), (1056, 104, 64)]                # <64, 2>:  41 <= cin <= 104
# mlp_fwd_kernel<BN, true> takes what the streaming kernel's LDS plan does not hold; BN = pick_bn(rows, cout): 64 / 128-column tiles only once they
# make >= 448 workgroups
GENERIC = [(1000, 50, 20), (1000, 131, 64), (1000, 384, 256),       # <32, true>
           (4096 + 32, 100, 1024),                                  # <64, true>
           (8192, 100, 1024)]                                       # <128, true>
# routing edges of the row count at 128 -> 128: short <32, 1, 1>, short's last, mlp_fwd_kernel<32, true> (no multiple of 128), lean <1>
EDGES = [(64, 128, 128), (8192, 128, 128), (8192 + 64, 128, 128), (8192 + 128, 128, 128)]


@pytest.mark.parametrize("rows,cin,cout,act,pool", _ap(STREAM + GENERIC + EDGES))
def test_forward_kernels_by_plan(rows, cin, cout, act, pool):
    check_forward(rows - rows % 32 if pool else rows, cin, cout, act, pool, padx=pitch4(cin))      # (pooled: 1000 -> 992 rows, still a ragged last tile)


# layers of <= 8192 rows (a multiple of 64) that the short kernel declines get rows / 32 partial statistics rows all the same
# (gspn_mlp_fwd_stats_bytes knows rows and cout only): the kernels of 128-row tiles are launched with four times as many workgroups as tiles
DECLINED = [(4096, 96, 64),            # fwd_lean_kernel<1>: cin not one of the short kernel's widths
            (4096, 40, 20),            # mlp_fwd_stream_kernel<32, 4>
            (4096, 128, 20),           # mlp_fwd_kernel<32, true>: cout no multiple of 32
            (8192, 100, 1024)]         # mlp_fwd_kernel<128, true>


@pytest.mark.parametrize("rows,cin,cout,act,pool", _ap(DECLINED))
def test_short_layers_the_short_kernel_declines_leave_zero_surplus_statistics_rows(rows, cin, cout, act, pool):
    check_forward(rows, cin, cout, act, pool, tile_rows=128)


# the two halves of vec_ok(X, ldx), one at a time: a pitch that is no multiple of 4 floats under an aligned pointer ...
@pytest.mark.parametrize("rows,cin,cout,act,pool", _ap([(1000, 67, 128), (1000, 6, 64), (1000, 50, 20), (4096, 128, 128), (4096, 96, 64)]))
def test_forward_kernels_on_a_pitch_of_odd_floats(rows, cin, cout, act, pool):
    """ldx % 4 != 0: the short, lean and streaming kernels decline, mlp_fwd_kernel<BN, false> takes every shape"""
    check_forward(rows - rows % 32 if pool else rows, cin, cout, act, pool, padx=pitch4(cin) + 1)


# ... and a pointer 4 bytes past a 16-byte boundary under a pitch of whole quads
@pytest.mark.parametrize("rows,cin,cout,act,pool", _ap(GENERIC + [(1000, 20, 100), (1000, 67, 64), (4096, 128, 128), (4096, 96, 64)]))
def test_forward_kernels_on_a_4_byte_aligned_input(rows, cin, cout, act, pool):
    """X 4 bytes past a 16-byte boundary, ldx % 4 == 0: the pointer alone makes the short, lean and streaming kernels decline;
    mlp_fwd_kernel<BN, false> at 32, 64 and 128 columns"""
    check_forward(rows - rows % 32 if pool else rows, cin, cout, act, pool, aligned=False, padx=pitch4(cin))


# ---- instances a tuning switch alone selects: one child process per setting ---------------------------------------------------------
SWITCHED = {
    # fwd_short_kernel<16 / 32, 1, 4>: cout a multiple of 128, cin <= 128
    "nt4": ({"GSPN_FWD_SHORT_NT": "4"}, [(64, 64, 128), (2048, 128, 128), (8192, 64, 256), (4032, 128, 384)]),
    # <KW, 2, 1> at small shapes: one tile for two workgroups (the second writes a zero statistics row), an odd tile count
    "mt2": ({"GSPN_FWD_SHORT_MT": "2"}, [(64, 64, 32), (64, 128, 96), (1984, 192, 32), (1984, 64, 96), (4032, 128, 32)]),
    # <KW, 2, 2>
    "mt2nt2": ({"GSPN_FWD_SHORT_MT": "2", "GSPN_FWD_SHORT_NT": "2"}, [(64, 64, 64), (64, 192, 192), (1984, 128, 64), (4032, 192, 128), (1984, 64, 192)]),
    # fwd_lean_kernel<2, ., .>: 64-column blocks
    "lean64": ({"GSPN_FWD_LEAN_BN": "64"}, [(4096, 96, 64), (4096, 32, 128), (8192 + 128, 128, 128), (2048, 160, 192)]),
}


def run_switched(name):
    """(the child's entry point)"""
    for shape in SWITCHED[name][1]:
        for act, pool in AP:
            check_forward(*shape, act, pool, tile_rows=64 if "GSPN_FWD_SHORT_MT" in SWITCHED[name][0] else None)     # MT = 2: rows / 32 workgroups, rows / 64 tiles
    print("SWITCHED_OK %s" % name)


@pytest.mark.parametrize("name", sorted(SWITCHED))
def test_forward_instances_behind_a_tuning_switch(name):
    env = dict(os.environ, **SWITCHED[name][0])
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_mlp_instances import run_switched; run_switched(%r)" % name],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "SWITCHED_OK %s" % name in r.stdout


# ---- backward: one stack per instantiation that the default environment selects and no other test launched ---------------------------
# (found by a sweep of mlp_stack over rows 96 .. 131072, 3 .. 1024 channels, dense / pooled, training / eval, aligned / 4-byte aligned operands
#  under a kernel trace; the smallest reaching shape of the sweep's grid each -- profiles/kernel_coverage_mlp.txt)
@pytest.mark.parametrize("rows,ld,cin,chans,ns", [
    (32768, 64, 64, [32, 32], None),           # bwd_lean_kernel<2, 0, false, true>: 64-column blocks need > 16384 rows
    (65536, 68, 67, [20], 32),                 # mlp_bwd_data_kernel<128, true, true, true>
    (4096, 1024, 1024, [20], 16),              # mlp_bwd_data_kernel<64, true, true, true>
    (4096, 8, 6, [36, 20], 32),                # mlp_fwd_stream_kernel<64, 4, false, true>: the pooled top layer's pass B, 33 .. 64 input channels
    (131072, 8, 6, [64], None),                # wgrad_stream_kernel<1, 2, 32, true, false, false, false>: a one-layer stack has no early coefficients
    (4096, 64, 64, [128], 32),                 # wgrad_lean_kernel<2, 2, 1, false>: a pooled layer without an input activation
    (4096, 128, 128, [128], 32),               # wgrad_lean_kernel<4, 2, 1, false>
])
def test_backward_instances_training(rows, ld, cin, chans, ns):
    from tests.test_gpu_mlp import check_stack_routed
    check_stack_routed(rows, ld, cin, chans, ns)


# fragile (silenced) gradient entries of these shapes, from the float64 reference alone: 0, 0.22, 0.24, 0.30 % (cap: 2 %)
@pytest.mark.parametrize("rows,ld,cin,chans,ns", [
    (4096, 4, 3, [32, 32], 256),               # bwd_lean_kernel<1, 2, false, true>: pool groups of >= 128 rows
    (131072, 4, 3, [64, 64], 32),              # bwd_lean_kernel<2, 1, false, true>
    (131072, 4, 3, [64, 64], 256),             # bwd_lean_kernel<2, 2, false, true>
    (131072, 4, 3, [32, 64], None),            # wgrad_stream_kernel<1, 2, 32, false, false, false, false>: two column tiles from 131072 rows on
])
def test_backward_instances_eval(rows, ld, cin, chans, ns):
    from tests.test_gpu_mlp import check_stack
    check_stack(rows, ld, cin, chans, ns, False, ref_device="cuda")


# ---- backward instantiations only an SA module in eval mode selects (the gathered first layer without batch statistics) --------------------
def sa_eval_reference(store, xyz, pts, npoint, radius, ns, mlp):
    """float64 composition of an eval-mode SA module on oracle geometry, from the variables of `store` under scope 'sa': returns the group
    indices, the pooled output (b, npoint, mlp[-1]), check_stack's fragile (group, channel) entries of it, and the float64 leaves"""
    import numpy as np
    from oracle import mlp_ref as R
    from oracle import oracle as O
    from tests.test_gpu_mlp import fragile_entries
    from tests.test_gpu_modules import ref_params
    b = xyz.shape[0]
    rnew = O.gather_point(xyz, O.farthest_point_sample(npoint, xyz))
    ridx, _ = O.query_ball_point(radius, ns, xyz, rnew)
    gi = torch.from_numpy(ridx.astype(np.int64))
    bi = torch.arange(b)[:, None, None].expand_as(gi)
    gx = torch.from_numpy(O.group_point(xyz, ridx) - rnew[:, :, None, :]).double()
    p64 = torch.from_numpy(pts).double().requires_grad_(True)
    h = torch.cat([gx, p64[bi, gi]], -1).reshape(-1, 3 + pts.shape[2])
    ps = ref_params(store, 'sa', ['conv%d' % i for i in range(len(mlp))])
    zs = []
    for p in ps:
        z, _, _ = R.layer(h, p["w"], p["b"], p["gamma"], p["beta"], p["moving_mean"], p["moving_var"], False, 0.5, True, relu=False)
        zs.append(z.detach())
        h = torch.relu(z)
    fragile, _ = fragile_entries(zs, ns)
    ref = h.view(b * npoint, ns, -1).max(dim=1).values.view(b, npoint, -1)
    return ridx, ref, fragile.view(b, npoint, -1), dict(pts=p64, ps=ps)


def sa_eval_variables(npoint, c, mlp, seed):
    """a fresh variable store with the module's layers under 'sa', their BN variables away from the initial (gamma 1, beta 0, mean 0, variance 1)"""
    from gspn_amd import pointnet_util as PU
    from gspn_amd import tf_util
    from tests.test_gpu_modules import fresh_store
    store = fresh_store(seed)
    with tf_util.variable_scope('sa'):
        layers = PU._mlp_layers(mlp, 3 + c, 'conv', True)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for lp in layers:
            n = lp.gamma.numel()
            lp.gamma.copy_(torch.rand(n, generator=g) + 0.5)
            lp.beta.copy_(torch.rand(n, generator=g) - 0.5)
            lp.moving_mean.copy_(torch.randn(n, generator=g) * 0.1)
            lp.moving_variance.copy_(torch.rand(n, generator=g) + 0.5)
    return store


# fragile (silenced) entries of the pooled output's gradient, from the float64 reference alone: 0.30 and 0.43 % (cap: check_stack's 2 %).  The radius
# fills every group with distinct points: a ball query pads a short group with copies of its first point, whose rows tie exactly (2.3 - 2.5 % at 0.2)
@pytest.mark.parametrize("b,n,c,npoint,radius,ns,mlp", [
    (2, 1024, 64, 1024, 0.5, 32, [64, 64, 128]),       # mlp_bwd_data_kernel<64, true, false, false>: 64 gathered feature columns, >= 57344 rows
    (2, 1024, 3, 1024, 0.5, 64, [64, 64, 128]),        # wgrad_stream_kernel<1, 2, 32, false, false, true, false>: two column tiles from 131072 rows on
])
def test_backward_instances_of_an_eval_mode_sa_module(b, n, c, npoint, radius, ns, mlp):
    """pointnet_sa_module(is_training=False) with the gathered first layer, forward at 1e-5 and every gradient at check_stack's 1e-4 against the
    float64 composition on oracle geometry, the upstream gradient silenced on check_stack's fragile entries."""
    import numpy as np
    from gspn_amd.pointnet_util import pointnet_sa_module
    from tests import data as D
    store = sa_eval_variables(npoint, c, mlp, 31)
    xyz = D.batch("U", b, n, 9)
    pts = np.random.default_rng(4).standard_normal((b, n, c)).astype(np.float32)
    tp = torch.from_numpy(pts).cuda().requires_grad_(True)
    new_xyz, out, idx = pointnet_sa_module(torch.from_numpy(xyz).cuda(), tp, npoint, radius, ns, mlp, None, False, False, 0.5, 'sa')
    ridx, ref, fragile, leaves = sa_eval_reference(store, xyz, pts, npoint, radius, ns, mlp)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    frac = float(fragile.float().mean())
    print("eval-mode SA module %s: fragile (silenced) gradient entries %.3f %% of %d" % ((b, n, c, npoint, ns, mlp), 100 * frac, fragile.numel()))
    assert frac <= 0.02
    assert out.shape == ref.shape
    err = lambda a, r: float((a.double().cpu() - r).abs().max() / (r.abs().max() + 1e-30))
    assert err(out, ref) < 1e-5
    go = torch.randn(ref.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    go[fragile] = 0
    ref.backward(go)
    out.backward(go.float().cuda())
    for i, p in enumerate(leaves["ps"]):
        assert err(store.vars['sa/conv%d/weights' % i].grad.view(p["w"].shape), p["w"].grad) < 1e-4, i
        assert err(store.vars['sa/conv%d/bn/gamma' % i].grad, p["gamma"].grad) < 1e-4, i
        assert err(store.vars['sa/conv%d/bn/beta' % i].grad, p["beta"].grad) < 1e-4, i
    assert err(tp.grad, leaves["pts"].grad) < 1e-4
