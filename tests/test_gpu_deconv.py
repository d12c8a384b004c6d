"""GPU parity of the transposed convolution (csrc/deconv.hip), tf_util.conv2d_transpose and the decoder / instance encoder of
shape_proposal_net against float64 restatements (tests/deconv_ref.py, oracle/mlp_ref.py)."""
import pytest
import torch

from tests import deconv_ref as DR
from tests.test_gpu_modules import fresh_store, rel_err

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _op(x, k, b, stride):
    from gspn_amd.deconv import conv2d_transpose_valid
    return conv2d_transpose_valid(x, k, b, stride)


def test_known_answer_orientation():
    """one-hot input pixel (iy, ix) times a ramp kernel: the output holds K[ky, kx, :, 0] at (iy*s + ky, ix*s + kx), nothing else"""
    kh, kw, cout, sh, sw, iy, ix = 3, 2, 4, 2, 3, 1, 2
    x = torch.zeros(1, 3, 4, 1, device=DEV)
    x[0, iy, ix, 0] = 1.0
    k = torch.tensor([[[[1.0 + 100 * ky + 10 * kx + co] for co in range(cout)] for kx in range(kw)] for ky in range(kh)], device=DEV)
    y = _op(x, k, None, (sh, sw)).cpu()
    want = torch.zeros(1, 3 * sh + max(kh - sh, 0), 4 * sw + max(kw - sw, 0), cout)
    for ky in range(kh):
        for kx in range(kw):
            want[0, iy * sh + ky, ix * sw + kx] = k[ky, kx, :, 0].cpu()
    assert torch.equal(y, want)


# every up-convolution of decoding_net's three branches at 512 decodes (model_rpointnet.py:284-301), then odd shapes:
# 3 / 5 / 33 channels, k < s, n = 1, non-square maps and kernels.   (n, hi, wi, cin, cout, kh, kw, sh, sw)
DECODER = [(512, 1, 1, 512, 512, 3, 3, 1, 1), (512, 3, 3, 512, 256, 3, 3, 2, 2), (512, 7, 7, 256, 128, 4, 4, 2, 2), (512, 16, 16, 128, 3, 1, 1, 1, 1),
           (512, 1, 1, 512, 512, 2, 2, 1, 1), (512, 2, 2, 512, 256, 3, 3, 1, 1), (512, 4, 4, 256, 256, 4, 4, 2, 2), (512, 10, 10, 256, 128, 5, 5, 3, 3),
           (512, 32, 32, 128, 3, 1, 1, 1, 1), (512, 2, 2, 512, 256, 2, 2, 1, 1), (512, 3, 3, 256, 256, 3, 3, 2, 2), (512, 7, 7, 256, 128, 4, 4, 3, 3),
           (512, 22, 22, 128, 3, 1, 1, 1, 1)]
ODD = [(3, 5, 5, 3, 5, 2, 2, 3, 3), (1, 4, 4, 33, 3, 3, 3, 2, 2), (2, 3, 3, 5, 33, 1, 1, 2, 2), (1, 1, 1, 3, 3, 1, 1, 1, 1), (1, 2, 2, 5, 5, 4, 4, 1, 1),
       (2, 3, 5, 5, 3, 3, 2, 2, 1), (1, 6, 3, 33, 33, 2, 5, 3, 2), (4, 1, 3, 64, 200, 3, 3, 3, 1)]


def _run(shape, seed):
    n, hi, wi, cin, cout, kh, kw, sh, sw = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, hi, wi, cin, generator=g).to(DEV).requires_grad_(True)
    k = (torch.randn(kh, kw, cout, cin, generator=g) * 0.1).to(DEV).requires_grad_(True)
    b = torch.randn(cout, generator=g).to(DEV).requires_grad_(True)
    y = _op(x, k, b, (sh, sw))
    dy = torch.randn(y.shape, generator=g).to(DEV)
    dx, dk, db = torch.autograd.grad(y, (x, k, b), dy)
    return (x, k, b, dy), (y, dx, dk, db)


@pytest.mark.parametrize("shape", DECODER + ODD)
def test_against_float64(shape):
    n, hi, wi, cin, cout, kh, kw, sh, sw = shape
    (x, k, b, dy), got = _run(shape, sum(shape))
    x64, k64, b64 = (t.detach().double().requires_grad_(True) for t in (x, k, b))
    y64 = DR.deconv(x64, k64, b64, (sh, sw))
    ref = (y64,) + torch.autograd.grad(y64, (x64, k64, b64), dy.double())
    assert got[0].shape == y64.shape
    for name, a, r in zip(("y", "dx", "dk", "dbias"), got, ref):
        e = rel_err(a, r)
        assert e <= 1e-5, "%s %s rel_err %.3g" % (shape, name, e)


@pytest.mark.parametrize("shape", [(512, 7, 7, 256, 128, 4, 4, 2, 2), (512, 16, 16, 128, 3, 1, 1, 1, 1), (3, 5, 5, 3, 5, 2, 2, 3, 3)])
def test_bit_identical(shape):
    _, a = _run(shape, 7)
    _, b = _run(shape, 7)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_bad_arguments_return_codes():
    from gspn_amd import _lib as L
    lib = L.lib()
    buf = torch.zeros(64, device=DEV)
    p = L.ptr(buf)
    st = L.stream()
    assert lib.gspn_deconv_fwd(0, 1, 1, 1, 1, 1, 1, 1, 1, p, p, None, p, st) == -1
    assert lib.gspn_deconv_fwd(1, 1, 1, 1, 1, 0, 1, 1, 1, p, p, None, p, st) == -1
    assert lib.gspn_deconv_fwd(1, 1, 1, 1, 1, 1, 1, 1, 0, p, p, None, p, st) == -1
    assert lib.gspn_deconv_fwd(1, 1, 1, 1, 1, 1, 1, 1, 1, None, p, None, p, st) == -1
    assert lib.gspn_deconv_bwd_input(1, 1, 1, 1, -3, 1, 1, 1, 1, p, p, p, st) == -1
    assert lib.gspn_deconv_bwd_kernel(1, 1, 1, 1, 1, 1, 1, 1, 1, p, p, p, p, None, st) == -1
    assert lib.gspn_deconv_bwd_kernel(1, 1, 1, 1, 1, 1, 1, 1, 1, p, p, None, None, p, st) == -1
    assert lib.gspn_deconv_fwd(1, 1 << 16, 1 << 16, 1, 1, 1, 1, 1, 1, p, p, None, p, st) == -2
    assert lib.gspn_deconv_bwd_kernel_work_bytes(0, 1, 1, 1, 1, 1, 1, 1, 1) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        _op(torch.zeros(1, 2, 2, 4, device=DEV), torch.zeros(2, 2, 3, 5, device=DEV), None, (1, 1))


# ---------------------------------------------------------------------------------------------------- tf_util.conv2d_transpose
def _check_grad(got, ref, name, tol=1e-4, zero_scale=1.0):
    """rel_err <= tol.  A bias in front of a batch norm has an exactly-zero gradient, which fp32 leaves as round-off of the size of the
    same layer's dbeta: then |got| <= tol * zero_scale (the float64 dbeta's largest entry, where the caller has it)"""
    if ref.abs().max() < 1e-10:
        assert float(got.abs().max()) <= tol * zero_scale, name
    else:
        e = rel_err(got, ref)
        assert e <= tol, "%s rel_err %.3g" % (name, e)


def test_conv2d_transpose_layer_bn_train_eval():
    from gspn_amd import tf_util
    store = fresh_store(3)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 3, 3, 8, generator=g).to(DEV).requires_grad_(True)
    y = tf_util.conv2d_transpose(x, 16, [3, 3], "up", stride=[2, 2], padding='VALID', bn=True, is_training=True, bn_decay=0.8,
                                 weight_decay=0.5)
    names = [(nm, tuple(v.shape)) for nm, v in store.vars.items()]
    assert names == [("up/weights", (3, 3, 16, 8)), ("up/conv2d_transpose/kernel", (3, 3, 16, 8)), ("up/conv2d_transpose/bias", (16,)),
                     ("up/bn/beta", (16,)), ("up/bn/gamma", (16,)), ("up/bn/moving_mean", (16,)), ("up/bn/moving_variance", (16,))]
    assert list(store.losses) == ["up/weights"]
    v = {nm: t.detach().double().cpu() for nm, t in store.vars.items()}
    lim = (6.0 / (9 * 16 + 9 * 8)) ** 0.5
    assert float(v["up/conv2d_transpose/kernel"].abs().max()) <= lim and float(v["up/conv2d_transpose/bias"].abs().max()) == 0.0
    p64 = {nm: v[nm].clone().requires_grad_(True) for nm in ("up/conv2d_transpose/kernel", "up/conv2d_transpose/bias", "up/bn/gamma", "up/bn/beta")}
    x64 = x.detach().double().cpu().requires_grad_(True)
    z = DR.deconv(x64, p64["up/conv2d_transpose/kernel"], p64["up/conv2d_transpose/bias"], (2, 2))
    # (the store's moving statistics were already updated by the call: start the float64 update from their initial values)
    r, mm, mv = DR.bn_relu(z, p64["up/bn/gamma"], p64["up/bn/beta"], torch.zeros(16, dtype=torch.float64), torch.ones(16, dtype=torch.float64),
                           True, 0.8)
    assert y.shape == r.shape == (6, 7, 7, 16)
    assert rel_err(y, r) <= 3e-5
    assert rel_err(store.vars["up/bn/moving_mean"], mm) <= 1e-5 and rel_err(store.vars["up/bn/moving_variance"], mv) <= 1e-5
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.to(DEV))
    r.backward(dy.double())
    assert store.vars["up/weights"].grad is None
    assert rel_err(x.grad, x64.grad) <= 1e-4
    for nm, t in p64.items():
        _check_grad(store.vars[nm].grad, t.grad, nm)
    # eval: the moving statistics normalise, and stay as they are
    mm0, mv0 = store.vars["up/bn/moving_mean"].clone(), store.vars["up/bn/moving_variance"].clone()
    ye = tf_util.conv2d_transpose(x.detach(), 16, [3, 3], "up", stride=[2, 2], padding='VALID', bn=True, is_training=False, bn_decay=0.8)
    re_, _, _ = DR.bn_relu(z.detach(), p64["up/bn/gamma"].detach(), p64["up/bn/beta"].detach(), mm0.double().cpu(), mv0.double().cpu(), False)
    assert rel_err(ye, re_) <= 3e-5
    assert torch.equal(mm0, store.vars["up/bn/moving_mean"]) and torch.equal(mv0, store.vars["up/bn/moving_variance"])
    # the dead variable has no gradient, so an optimizer step leaves it bit-identical
    dead = store.vars["up/weights"].detach().clone()
    opt = torch.optim.Adam(store.parameters(), lr=1e-2)
    opt.step()
    assert torch.equal(dead, store.vars["up/weights"])
    assert not torch.equal(p64["up/conv2d_transpose/kernel"].detach().float(), store.vars["up/conv2d_transpose/kernel"].detach().cpu())


def test_conv2d_transpose_linear_no_bn():
    from gspn_amd import tf_util
    store = fresh_store(4)
    x = torch.randn(3, 16, 16, 128, device=DEV)
    y = tf_util.conv2d_transpose(x, 3, [1, 1], "last", stride=[1, 1], padding='VALID', activation_fn=None)
    k = store.vars["last/conv2d_transpose/kernel"].detach().double().cpu()
    b = torch.linspace(-1, 1, 3, dtype=torch.float64)
    with torch.no_grad():
        store.vars["last/conv2d_transpose/bias"].copy_(b.float())
    y = tf_util.conv2d_transpose(x, 3, [1, 1], "last", stride=[1, 1], padding='VALID', activation_fn=None)
    assert rel_err(y, DR.deconv(x.double().cpu(), k, b)) <= 1e-5
    assert [nm for nm in store.vars] == ["last/weights", "last/conv2d_transpose/kernel", "last/conv2d_transpose/bias"]


# ---------------------------------------------------------------------------------------------------- decoder / instance encoder
def _decoder_ref(store, scope, feat64, num_point, is_training):
    from gspn_amd.shape_proposal import decoder_layers
    layers, npc = decoder_layers(num_point)
    P = {}

    def par(nm):
        if nm not in P:
            P[nm] = store.vars[nm].detach().double().cpu().clone().requires_grad_(True)
        return P[nm]
    net = feat64.reshape(-1, 1, 1, feat64.shape[-1])
    for name, cout, k, s, bn in layers:
        pre = "%s/%s/" % (scope, name)
        net = DR.deconv(net, par(pre + "conv2d_transpose/kernel"), par(pre + "conv2d_transpose/bias"), (s, s))
        if bn:
            net, _, _ = DR.bn_relu(net, par(pre + "bn/gamma"), par(pre + "bn/beta"), store.vars[pre + "bn/moving_mean"].double().cpu(),
                                   store.vars[pre + "bn/moving_variance"].double().cpu(), is_training)
    pc_up = net.reshape(-1, npc, 3)
    h = feat64.reshape(-1, feat64.shape[-1])
    for nm in ("de_fc2", "de_fc3"):
        pre = "%s/%s/" % (scope, nm)
        h = h @ par(pre + "weights") + par(pre + "biases")
        h, _, _ = DR.bn_relu(h, par(pre + "bn/gamma"), par(pre + "bn/beta"), store.vars[pre + "bn/moving_mean"].double().cpu(),
                             store.vars[pre + "bn/moving_variance"].double().cpu(), is_training)
    h = h @ par(scope + "/de_fc4/weights") + par(scope + "/de_fc4/biases")
    pc = torch.cat([pc_up, h.reshape(-1, num_point - npc, 3)], dim=1)
    return pc.reshape(feat64.shape[0], feat64.shape[1], num_point, 3), P


@pytest.mark.parametrize("num_point", [512, 1024, 2048])
def test_decoding_net_against_float64(num_point):
    from gspn_amd.shape_proposal import decoding_net
    store = fresh_store(11)
    g = torch.Generator().manual_seed(num_point)
    feat = torch.randn(2, 4, 256, generator=g).to(DEV).requires_grad_(True)
    pc = decoding_net(feat, num_point, "decoder", True, None)
    assert pc.shape == (2, 4, num_point, 3)
    feat64 = feat.detach().double().cpu().requires_grad_(True)
    ref, P = _decoder_ref(store, "decoder", feat64, num_point, True)
    assert rel_err(pc, ref) <= 3e-5
    dpc = torch.randn(pc.shape, generator=g)
    pc.backward(dpc.to(DEV))
    ref.backward(dpc.double())
    assert rel_err(feat.grad, feat64.grad) <= 1e-4
    for nm, t in P.items():
        _check_grad(store.vars[nm].grad, t.grad, nm)
    names = [nm for nm in store.vars]
    layers = [l[0] for l in __import__("gspn_amd.shape_proposal", fromlist=["x"]).decoder_layers(num_point)[0]]
    want = []
    for i, name in enumerate(layers):
        want += ["decoder/%s/weights" % name, "decoder/%s/conv2d_transpose/kernel" % name, "decoder/%s/conv2d_transpose/bias" % name]
        if i < len(layers) - 1:
            want += ["decoder/%s/bn/%s" % (name, s) for s in ("beta", "gamma", "moving_mean", "moving_variance")]
    for nm in ("de_fc2", "de_fc3"):
        want += ["decoder/%s/%s" % (nm, s) for s in ("weights", "biases", "bn/beta", "bn/gamma", "bn/moving_mean", "bn/moving_variance")]
    want += ["decoder/de_fc4/weights", "decoder/de_fc4/biases"]
    assert names == want
    for name in layers:
        assert store.vars["decoder/%s/weights" % name].grad is None


def test_single_encoding_net_against_float64():
    from gspn_amd.shape_proposal import single_encoding_net
    from oracle import mlp_ref as R
    store = fresh_store(12)
    g = torch.Generator().manual_seed(2)
    pc = (torch.rand(64, 512, 3, generator=g) - 0.5).to(DEV)           # 64 instances of 512 points, centred like normalised instances
    out = single_encoding_net(pc, [64, 256, 512], [256], "pc_ins_encoder", True, None)
    assert out.shape == (64, 256)

    def par(nm):
        return store.vars[nm].detach().double().cpu().clone().requires_grad_(True)
    ps = []
    for i in range(3):
        pre = "pc_ins_encoder/conv%d/" % i
        w = par(pre + "weights")
        ps.append({"w": w.view(w.shape[-2], w.shape[-1]), "wleaf": w, "b": par(pre + "biases"), "gamma": par(pre + "bn/gamma"),
                   "beta": par(pre + "bn/beta"), "moving_mean": torch.zeros(w.shape[-1], dtype=torch.float64),
                   "moving_var": torch.ones(w.shape[-1], dtype=torch.float64), "bn": True})
    z, _ = R.stack(pc.double().cpu().reshape(-1, 3), ps, True)                 # (64*512, 512) before the pool
    # the float64 backward follows the GPU forward's own decisions: the pool winner of every (instance, channel) is the row whose float64
    # value is nearest the GPU's pooled value (the same conv stack again, deterministic), and fc0's ReLU mask is the GPU output's
    from gspn_amd.mlp import mlp_stack
    from gspn_amd.pointnet_util import _mlp_layers
    from gspn_amd import tf_util
    with tf_util.variable_scope("pc_ins_encoder"):
        rows = torch.nn.functional.pad(pc.reshape(-1, 3), (0, 1))
        pooled = mlp_stack(rows, 3, _mlp_layers([64, 256, 512], 3, 'conv', True), True, None, pool_ns=512).detach().double().cpu()
    zg = z.view(64, 512, 512)
    win = (zg.detach() - pooled.unsqueeze(1)).abs().argmin(dim=1, keepdim=True)
    h = zg.gather(1, win).squeeze(1)
    assert rel_err(h, pooled) <= 3e-5
    fc = {k: par("pc_ins_encoder/fc0/" + k) for k in ("weights", "biases", "bn/gamma", "bn/beta")}
    ref, _, _ = R.layer(h, fc["weights"], fc["biases"], fc["bn/gamma"], fc["bn/beta"], torch.zeros(256, dtype=torch.float64),
                        torch.ones(256, dtype=torch.float64), True, relu=False)
    ref = ref * (out.detach().cpu() > 0).double()
    assert rel_err(out, ref) <= 3e-5
    d = torch.randn(out.shape, generator=g)
    out.backward(d.to(DEV))
    ref.backward(d.double())
    for i, p in enumerate(ps):
        pre = "pc_ins_encoder/conv%d/" % i
        _check_grad(store.vars[pre + "weights"].grad, p["wleaf"].grad, pre + "weights")
        _check_grad(store.vars[pre + "bn/gamma"].grad, p["gamma"].grad, pre + "bn/gamma")
        _check_grad(store.vars[pre + "bn/beta"].grad, p["beta"].grad, pre + "bn/beta")
    for k, t in fc.items():
        _check_grad(store.vars["pc_ins_encoder/fc0/" + k].grad, t.grad, k, zero_scale=float(fc["bn/beta"].grad.abs().max()))
    names = [nm for nm in store.vars]
    want = ["pc_ins_encoder/conv%d/%s" % (i, s) for i in range(3)
            for s in ("weights", "biases", "bn/beta", "bn/gamma", "bn/moving_mean", "bn/moving_variance")]
    assert names == want + ["pc_ins_encoder/fc0/%s" % s for s in ("weights", "biases", "bn/beta", "bn/gamma", "bn/moving_mean", "bn/moving_variance")]


def test_sample_fixed_noise():
    from gspn_amd.shape_proposal import sample
    g = torch.Generator().manual_seed(9)
    mean, log_var, eps = (torch.randn(2, 64, 256, generator=g) for _ in range(3))
    log_var = log_var.clamp(-10, 1)
    z = sample(mean.to(DEV), log_var.to(DEV), eps.to(DEV))
    ref = mean.double() + torch.exp(log_var.double() / 2.0) * eps.double()
    assert rel_err(z, ref) <= 1e-6
    zr = sample(mean.to(DEV), log_var.to(DEV))
    assert zr.shape == mean.shape and zr.device == DEV and not torch.equal(zr, z)
