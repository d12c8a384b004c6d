"""One row per torch.autograd.Function of gspn_amd/ (tests/test_cpu_autograd_contract.py holds the table to the sources): the node's smallest
meaningful inputs as float64 / int32 masters on the CPU, the public call that reaches it, a float64 restatement in plain torch, and the
tolerance its own value test already holds it to.  tests/test_gpu_autograd_contract.py drives every row the ways autograd can drive a node.

A row's inputs are named.  `grads`: float inputs that take a gradient; `params`: layer tensors that take one; `consts`: float inputs that take
none (coordinates, interpolation weights); `ints`: index tensors -- every one holds duplicates and leaves one target unreferenced; `state`:
moving statistics, updated in place by the forward pass.  `call(t, hold)` takes the tensors on the device under those names and returns the
tuple of differentiable outputs; what the node keeps beside its arguments (an SA module's geometry) it leaves in hold["internals"].
`ref(t)` is the same on float64 CPU tensors.  `reread`: the inputs backward reads again (an in-place change between the two passes must
raise).  `expand`: inputs for which a stride-0 broadcast has a meaning.  `declines`: weights whose public call documents that it
refuses them, before anything runs, unless they are contiguous (it slices them in place) -- a view of one must raise NotImplementedError.
`int_grads`: the node's backward still adds with atomics, so its
upstream gradients are integers in [-8, 8] (and its inputs dyadic where a product enters the sum): every order of the sum is then exact.
`zero_scale`: gradients whose true value is zero up to rounding (a bias in front of a batch norm), held to the scale of the named one.
`decisions(t)`: the float64 pre-activations of a batch-normalised ReLU stack -- the builders' seeds are chosen so that none lies within
float32 rounding of the kink and no pool group ties (tests.test_gpu_mlp.fragile_entries), and the GPU test asserts that they still do."""
import numpy as np
import torch

from oracle import mlp_ref as R

DECAY = 0.7
# how a row's figures are compared with float64.  ("rel", t): max |got - ref| <= t * max |ref|, the rel_err of tests/test_gpu_mlp.py;
# ("allclose", t): |got - ref| <= t + t * |ref| elementwise, numpy's assert_allclose(rtol=t, atol=t) of tests/test_gpu_geometry.py
# ("exact",): equal to the float64 figure bit for bit (a copy, or a sum of integers: the masters are rounded to float32 before either side sees them)
REL5, REL4, REL6, CLOSE5, EXACT = ("rel", 1e-5), ("rel", 1e-4), ("rel", 1e-6), ("allclose", 1e-5), ("exact",)


class Case:
    def __init__(self, name, node, build, call, ref, tol_out, tol_grad, tol_from, grads=(), params=(), consts=(), ints=(), state=(),
                 reread=(), expand=(), int_grads=False, zero_scale=None, decisions=None, second=None,
                 targets=None, declines=()):
        self.name, self.node, self.build, self.call, self.ref = name, node, build, call, ref
        self.tol_out, self.tol_grad, self.tol_from = tol_out, tol_grad, tol_from
        self.grads, self.params, self.consts, self.ints, self.state = tuple(grads), tuple(params), tuple(consts), tuple(ints), tuple(state)
        self.reread, self.expand, self.int_grads = tuple(reread), tuple(expand), int_grads
        self.zero_scale = dict(zero_scale or {})
        self.decisions = decisions
        self.targets = dict(targets or {})     # index input -> how many targets it indexes (the last one is never named)
        self.declines = tuple(declines)        # layer tensors the public call refuses (NotImplementedError, before anything runs) unless contiguous and aligned
        self.second = second             # name of a row of another kind whose first output has this row's output shape (scenario 3)

    def __repr__(self):
        return self.name


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _index(g, n, *shape):
    """int32 indices into n targets: the last target is never named, target 0 is named by a whole row, every row repeats an entry"""
    idx = torch.randint(0, n - 1, shape, generator=g, dtype=torch.int32)
    idx[..., -1] = idx[..., 0]
    idx[0, 0] = 0
    return idx


def take(points, idx):
    """points (b, n, c), idx (b, ...) -> (b, ..., c): plain indexing, scene by scene"""
    b = points.shape[0]
    bi = torch.arange(b).view(b, *([1] * (idx.dim() - 1))).expand_as(idx)
    return points[bi, idx.long()]


# ---- the shared MLP ----------------------------------------------------------------------------------------------------------------------

def _layer_masters(g, chans, cin, bn=True):
    t = {}
    for i, c in enumerate(chans):
        lim = (6.0 / (cin + c)) ** 0.5
        t["w%d" % i] = (torch.rand(cin, c, generator=g, dtype=torch.float64) * 2 - 1) * lim
        t["b%d" % i] = (torch.rand(c, generator=g, dtype=torch.float64) - 0.5) * 0.2
        if bn:
            t["gamma%d" % i] = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
            t["beta%d" % i] = torch.rand(c, generator=g, dtype=torch.float64) - 0.5
            t["mm%d" % i] = torch.zeros(c, dtype=torch.float64)
            t["mv%d" % i] = torch.ones(c, dtype=torch.float64)
        cin = c
    return t


def _layer_names(nl, bn=True):
    params = sum([["w%d" % i, "b%d" % i] + (["gamma%d" % i, "beta%d" % i] if bn else []) for i in range(nl)], [])
    state = sum([["mm%d" % i, "mv%d" % i] for i in range(nl)], []) if bn else []
    return params, state


def layer_params(t, nl, bn=True):
    from gspn_amd.mlp import LayerParams
    return [LayerParams(t["w%d" % i], t["b%d" % i], True, t["beta%d" % i], t["gamma%d" % i], t["mm%d" % i], t["mv%d" % i]) if bn
            else LayerParams(t["w%d" % i], t["b%d" % i], False) for i in range(nl)]


def _ref_layers(h, t, nl, pool_ns=None, zs=None):
    for i in range(nl):
        z, _, _ = R.layer(h, t["w%d" % i], t["b%d" % i], t["gamma%d" % i], t["beta%d" % i], t["mm%d" % i], t["mv%d" % i], True, DECAY, True,
                          relu=False)
        if zs is not None:
            zs.append(z.detach())
        h = torch.relu(z)
    if pool_ns:
        h = h.view(-1, pool_ns, h.shape[1]).max(dim=1).values
    return h


STACK_ROWS, STACK_CIN, STACK_CHANS = 320, 19, [32, 48]          # 2 scenes x 5 groups x 32 samples; 19 columns: a pitch that is no multiple of 4


def _build_stack(seed):
    def build():
        g = _gen(seed)
        t = {"x": _randn(g, STACK_ROWS, STACK_CIN)}
        t.update(_layer_masters(g, STACK_CHANS, STACK_CIN))
        return t
    return build


def _call_stack(pool_ns):
    def call(t, hold=None):
        from gspn_amd.mlp import mlp_stack
        return (mlp_stack(t["x"], STACK_CIN, layer_params(t, 2), True, DECAY, pool_ns=pool_ns),)
    return call


def _ref_stack(pool_ns):
    return lambda t: (_ref_layers(t["x"], t, 2, pool_ns),)


def _decisions_stack(pool_ns):
    def decisions(t):
        zs = []
        _ref_layers(t["x"], t, 2, pool_ns, zs)
        return zs, pool_ns
    return decisions


SA_SHAPES = {
    # the smallest shapes at which tests/test_gpu_sa_variants.py shows the form being selected (b, n, c, npoint, radius, nsample, mlp)
    "gathered": (3, 1500, 8, 100, 0.3, 16, [32, 48]),       # test_fused_sa_front_end_equals_the_materialised_path: c < 16 -> mlp_stack(gather=)
    "preagg": (2, 1024, 20, 64, 0.3, 32, [64, 32]),         # the same test's c >= 16 row: preagg_ok, as test_preaggregated_first_layer_random_shapes needs
}


def _build_sa(form, seed):
    def build():
        from tests import data as D
        b, n, c, npoint, radius, ns, mlp = SA_SHAPES[form]
        g = _gen(seed)
        t = {"xyz": torch.from_numpy(D.batch("U", b, n, 6)).double(), "points": _randn(g, b, n, c)}
        t.update(_layer_masters(g, mlp, 3 + c))
        return t
    return build


def _call_sa(form):
    def call(t, hold=None):
        from gspn_amd import pointnet_util as PU
        from gspn_amd import tf_util
        from gspn_amd.geometry import sa_geometry
        b, n, c, npoint, radius, ns, mlp = SA_SHAPES[form]
        store = tf_util.set_variable_store(tf_util.VariableStore(seed=1))
        for i in range(len(mlp)):
            for name, key in (("weights", "w"), ("biases", "b"), ("bn/beta", "beta"), ("bn/gamma", "gamma"), ("bn/moving_mean", "mm"),
                              ("bn/moving_variance", "mv")):
                v = t["%s%d" % (key, i)]
                store.vars["sa/conv%d/%s" % (i, name)] = v[None, None] if key == "w" else v          # the stored kernel is (1, 1, cin, cout)
        geo = sa_geometry(t["xyz"], npoint, radius, ns, inverse=True)
        _, out, _ = PU.pointnet_sa_module(t["xyz"], t["points"], npoint, radius, ns, mlp, None, False, True, DECAY, "sa", geometry=geo)
        if hold is not None:
            keys = ("gidx", "rel", "idx", "order", "offsets") if form == "gathered" else ("gidx", "rel", "order", "offsets")
            hold["internals"] = {k: getattr(geo, k) for k in keys}
            hold["form"] = _stack_form(out)
        return (out,)
    return call


def _stack_form(out):
    """which form of _MlpStack produced `out`: 'gathered', 'preagg' or 'plain' (read off the node's ctx)"""
    node, seen = out.grad_fn, 0
    while node is not None and not hasattr(node, "spec") and seen < 8:
        node, seen = (node.next_functions[0][0] if node.next_functions else None), seen + 1
    if node is None or not hasattr(node, "spec"):
        return None
    return "gathered" if node.spec.get("gather") is not None else ("preagg" if node.spec.get("preagg") is not None else "plain")


def _sa_rows(form, t):
    from oracle import oracle as O
    b, n, c, npoint, radius, ns, mlp = SA_SHAPES[form]
    xyz = t["xyz"].detach().float().numpy()
    new = O.gather_point(xyz, O.farthest_point_sample(npoint, xyz))
    idx = torch.from_numpy(O.query_ball_point(radius, ns, xyz, new)[0].astype(np.int64))
    gx = take(t["xyz"], idx) - torch.from_numpy(new).double()[:, :, None, :]
    return torch.cat([gx, take(t["points"], idx)], -1).reshape(-1, 3 + c), b, npoint, ns, len(mlp), idx


def _ref_sa(form):
    def ref(t):
        rows, b, npoint, ns, nl, _ = _sa_rows(form, t)
        return (_ref_layers(rows, t, nl, ns).view(b, npoint, -1),)
    return ref


def _decisions_sa(form):
    def decisions(t):
        rows, b, npoint, ns, nl, idx = _sa_rows(form, t)
        zs = []
        _ref_layers(rows, t, nl, ns, zs)
        # a ball with fewer than nsample points repeats its first hit: rows of one group that name the same point are equal, and which of
        # them wins the pool changes no gradient.  Only the first of them stands for the tie rule.
        first = torch.ones_like(idx, dtype=torch.bool)
        for j in range(1, ns):
            first[:, :, j] = (idx[:, :, :j] != idx[:, :, j:j + 1]).all(-1)
        zs[-1] = torch.where(first.reshape(-1, 1), zs[-1], torch.full_like(zs[-1], -1e30))
        return zs, ns
    return decisions


def _build_linear():
    g = _gen(21)
    return {"x": _randn(g, 300, 19), "w0": _randn(g, 19, 20) / 19 ** 0.5, "b0": _randn(g, 20)}     # (300, 20) out: pad_cols' and tile_linear's shape


def _call_linear(t, hold=None):
    from gspn_amd.mlp import LayerParams, mlp_linear
    return (mlp_linear(t["x"], 19, LayerParams(t["w0"], t["b0"], False)),)


def _build_bn():
    g = _gen(22)
    return {"x": _randn(g, 300, 19) * 2 + 1, "gamma": torch.rand(19, generator=g, dtype=torch.float64) + 0.5, "beta": _randn(g, 19),
            "mm": _randn(g, 19) * 0.1, "mv": torch.rand(19, generator=g, dtype=torch.float64) + 0.5}


def _call_bn(t, hold=None):
    from gspn_amd import tf_util
    store = tf_util.set_variable_store(tf_util.VariableStore(seed=1))
    for name, key in (("beta", "beta"), ("gamma", "gamma"), ("moving_mean", "mm"), ("moving_variance", "mv")):
        store.vars["bn/" + name] = t[key]
    return (tf_util.batch_norm_template(t["x"], True, "bn", [0], DECAY),)


def _ref_bn(t):
    x = t["x"].reshape(-1, 19)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)                     # tf.nn.moments: the biased variance
    inv = torch.rsqrt(var + R.EPS) * t["gamma"]
    return ((x * inv + (t["beta"] - mean * inv)).view(t["x"].shape),)


def _build_sync_bn():
    g = _gen(23)
    return {"x": _randn(g, 300, 19) * 2 + 1, "gamma": torch.rand(19, generator=g, dtype=torch.float64) + 0.5, "beta": _randn(g, 19),
            "mm": _randn(g, 19) * 0.1, "mv": torch.rand(19, generator=g, dtype=torch.float64) + 0.5}


def _call_sync_bn(t, hold=None):
    from gspn_amd.parallel import sync_bn_relu
    return (sync_bn_relu(t["x"], t["gamma"], t["beta"], t["mm"], t["mv"], DECAY, R.EPS, relu=False),)


def _ref_sync_bn(t):
    x = t["x"]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    inv = torch.rsqrt(var + R.EPS) * t["gamma"]
    return (x * inv + (t["beta"] - mean * inv),)


def _build_deconv():
    g = _gen(24)
    return {"x": _randn(g, 2, 3, 5, 6), "kernel": _randn(g, 3, 3, 7, 6) / 6 ** 0.5, "bias": _randn(g, 7)}


def _call_deconv(t, hold=None):
    from gspn_amd.deconv import conv2d_transpose_valid
    return (conv2d_transpose_valid(t["x"], t["kernel"], t["bias"], (2, 2)),)


def _ref_deconv(t):
    from tests import deconv_ref as DR
    return (DR.deconv(t["x"], t["kernel"], t["bias"], (2, 2)),)


# ---- gathers and their transposes --------------------------------------------------------------------------------------------------------

B, N, M, NS, C = 2, 200, 40, 8, 19


def _build_group():
    g = _gen(31)
    return {"points": _randn(g, B, N, C), "idx": _index(g, N, B, M, NS)}


def _call_group_point(t, hold=None):
    from gspn_amd.tf_grouping import group_point
    return (group_point(t["points"], t["idx"]),)


def _call_group_maxpool(t, hold=None):
    from gspn_amd.tf_grouping import group_maxpool
    return (group_maxpool(t["points"], t["idx"])[0],)


def _build_gather_point():
    g = _gen(32)
    return {"inp": _randn(g, B, N, 3), "idx": _index(g, N, B, 64)}


def _call_gather_point(t, hold=None):
    from gspn_amd.tf_sampling import gather_point
    return (gather_point(t["inp"], t["idx"]),)


def _weights(g, *shape):
    w = torch.rand(*shape, generator=g, dtype=torch.float64) + 0.05
    return w / w.sum(-1, keepdim=True)


def _build_interpolate():
    g = _gen(33)
    return {"points": _randn(g, B, 50, C), "idx": _index(g, 50, B, N, 3), "weight": _weights(g, B, N, 3)}


def _call_interpolate(t, hold=None):
    from gspn_amd.tf_interpolate import three_interpolate
    return (three_interpolate(t["points"], t["idx"], t["weight"]),)


def _ref_interpolate(t):
    return ((take(t["points"], t["idx"]) * t["weight"].unsqueeze(-1)).sum(2),)


def _build_nn_distance():
    """coordinates on a grid of 2^-10 in [-1, 1): every squared distance (< 2^24 units of 2^-20), every term 2 g (a - b) of the gradient,
    with g an integer in [-8, 8], and every sum of a few hundred of them (< 2^22 units of 2^-9) is exact in float32, whatever order the
    LDS atomics take -- so outputs and gradients are held to the float64 figures bit for bit, as the node's value test holds its outputs
    to the oracle's"""
    g = _gen(34)
    grid = lambda *s: torch.randint(-1024, 1024, s, generator=g).double() / 1024
    return {"xyz1": grid(B, N, 3), "xyz2": grid(B, 150, 3)}


def _call_nn_distance(t, hold=None):
    from gspn_amd.tf_nndistance import nn_distance
    d1, _, d2, _ = nn_distance(t["xyz1"], t["xyz2"])
    return d1, d2


def _ref_nn_distance(t):
    d = ((t["xyz1"][:, :, None, :] - t["xyz2"][:, None, :, :]) ** 2).sum(-1)
    two = d.detach().topk(2, dim=2, largest=False).values, d.detach().topk(2, dim=1, largest=False).values
    assert float((two[0][:, :, 1] - two[0][:, :, 0]).min()) > 0 and float((two[1][:, 1] - two[1][:, 0]).min()) > 0, "a tie between two nearest points"
    return d.min(2).values, d.min(1).values


def _build_group_concat():
    g = _gen(35)
    xyz = torch.rand(B, N, 3, generator=g, dtype=torch.float64)
    return {"xyz": xyz, "new_xyz": xyz[:, :M].clone(), "points": _randn(g, B, N, 5), "idx": _index(g, N, B, M, NS)}


def _call_group_concat(t, hold=None):
    from gspn_amd.invlists import inverse_lists
    from gspn_amd.pointnet_util import group_concat
    order, offsets = inverse_lists(t["idx"].reshape(B, -1), N)
    if hold is not None:
        hold["internals"] = {"order": order, "offsets": offsets}
    return (group_concat(t["xyz"], t["new_xyz"], t["points"], t["idx"], True, order, offsets),)


def _ref_group_concat(t):
    rows = torch.cat([take(t["xyz"], t["idx"]) - t["new_xyz"][:, :, None, :], take(t["points"], t["idx"])], -1).reshape(-1, 8)
    return (rows,)                                       # 3 + 5 columns: the pitch of 8 has no pad column


def _build_fp_concat():
    g = _gen(36)
    return {"points2": _randn(g, B, 50, C), "points1": _randn(g, B, N, 5), "idx": _index(g, 50, B, N, 3), "weight": _weights(g, B, N, 3)}


def _call_fp_concat(t, hold=None):
    from gspn_amd.invlists import inverse_lists
    from gspn_amd.pointnet_util import fp_concat
    order, offsets = inverse_lists(t["idx"].reshape(B, -1), 50)
    if hold is not None:
        hold["internals"] = {"order": order, "offsets": offsets}
    return (fp_concat(t["points2"], t["idx"], t["weight"], t["points1"], order, offsets),)


def _ref_fp_concat(t):
    rows = torch.cat([(take(t["points2"], t["idx"]) * t["weight"].unsqueeze(-1)).sum(2), t["points1"]], -1).reshape(-1, C + 5)
    return (rows,)                                       # 19 + 5 = 24 columns: no pad column


def _call_pad_cols(t, hold=None):
    from gspn_amd.pointnet_util import _PadCols          # (private: the SA module reaches it for feature widths that are no multiple of 4)
    return (_PadCols.apply(t["x"], 20),)


def _build_crop():
    from tests import heads_ref as HR
    pc, fea, cen, rois, idx, w, bias = HR.crop_linear_case(B, N, 20, 6, 16, 32, seed=37)
    return {"pc": pc.double(), "pc_fea": fea.double(), "pc_center": cen.double(), "rois": rois.double(), "idx": idx, "w0": w.double(), "b0": bias.double()}


def _build_crop_gather():
    t = _build_crop()
    return {k: v for k, v in t.items() if k not in ("w0", "b0")}


def _call_crop_gather(t, hold=None):
    from gspn_amd.roi import points_cropping
    return tuple(points_cropping(t["pc"], t["pc_fea"], t["pc_center"], t["rois"], t["idx"], 6, 16, True))


def _ref_crop_gather(t):
    from tests import heads_ref as HR
    rows = HR.crop_rows(t["pc"], t["pc_fea"], t["pc_center"], t["rois"], t["idx"], True)
    raw = take(t["pc"], t["idx"].reshape(B, -1)).reshape(B, 6, 16, 3)
    return rows[..., :20], rows[..., 20:23], rows[..., 23:], raw


def _call_crop_linear(t, hold=None):
    from gspn_amd.heads import crop_linear
    from gspn_amd.mlp import LayerParams
    return (crop_linear(t["pc"], t["pc_fea"], t["pc_center"], t["rois"], t["idx"], LayerParams(t["w0"], t["b0"], False), True),)


def _ref_crop_linear(t):
    from tests import heads_ref as HR
    return (HR.crop_linear(t["pc"], t["pc_fea"], t["pc_center"], t["rois"], t["idx"], t["w0"], t["b0"], True),)


def _build_gather_rows():
    g = _gen(38)
    label = torch.randint(0, 6, (B, 50), generator=g)                           # int64, as shape_proposal_net's group_label.long(); row 6 is never named
    label[:, -1] = label[:, 0]
    return {"src": _randn(g, B, 7, C), "label": label}


def _call_gather_rows(t, hold=None):
    from gspn_amd.shape_proposal import _GatherRows      # (private: shape_proposal_net's gather of the instance rows at the seeds' labels)
    return (_GatherRows.apply(t["src"], t["label"]),)


TILE_G, TILE_P = 6, 50


def _build_tile():
    g = _gen(39)
    return {"local": _randn(g, TILE_G * TILE_P, 19), "glob": _randn(g, TILE_G, 21), "w0": _randn(g, 40, 20) / 40 ** 0.5, "b0": _randn(g, 20)}


def _call_tile(t, hold=None):
    from gspn_amd.heads import tile_linear
    from gspn_amd.mlp import LayerParams
    return (tile_linear(t["local"], t["glob"], LayerParams(t["w0"], t["b0"], False), TILE_P),)


def _ref_tile(t):
    rows = torch.cat([t["glob"].repeat_interleave(TILE_P, 0), t["local"]], 1)
    return (rows @ t["w0"] + t["b0"],)


_P2, _S2 = _layer_names(2)
_ZERO2 = {"b0": "w0", "b1": "w1"}                        # a bias in front of a batch norm: zero up to rounding (tests.test_gpu_mlp.bias_err)
_MLP_FROM = "tests/test_gpu_mlp.py::test_mlp_stack_forward_backward"
_SA_FROM = "tests/test_gpu_modules.py::test_sa_module_matches_oracle"

CASES = [
    Case("mlp_stack", "_MlpStack", _build_stack(101), _call_stack(None), _ref_stack(None), REL5, REL4, _MLP_FROM, grads=["x"], params=_P2,
         state=_S2, reread=["x", "w0", "w1", "gamma0", "gamma1"], expand=["b0", "beta1"], zero_scale=_ZERO2,
         decisions=_decisions_stack(None)),
    Case("mlp_stack_pooled", "_MlpStack", _build_stack(102), _call_stack(32), _ref_stack(32), REL5, REL4, _MLP_FROM, grads=["x"], params=_P2,
         state=_S2, reread=["x", "w0", "w1", "b1", "gamma0", "gamma1"], expand=["b1", "gamma0"], zero_scale=_ZERO2,
         decisions=_decisions_stack(32)),
    Case("mlp_stack_gathered", "_MlpStack", _build_sa("gathered", 119), _call_sa("gathered"), _ref_sa("gathered"), REL5, REL4, _SA_FROM,
         grads=["points"], params=_P2, consts=["xyz"], state=_S2, reread=["points", "w0", "w1", "gamma0", "gamma1"], expand=["b0"],
         zero_scale=_ZERO2, decisions=_decisions_sa("gathered")),
    Case("mlp_stack_preagg", "_MlpStack", _build_sa("preagg", 117), _call_sa("preagg"), _ref_sa("preagg"), REL5, REL4, _SA_FROM,
         grads=["points"], params=_P2, consts=["xyz"], state=_S2, reread=["points", "w0", "w1", "gamma0", "gamma1"], expand=["b0"],
         zero_scale=_ZERO2, decisions=_decisions_sa("preagg")),
    Case("mlp_linear", "_Linear", _build_linear, _call_linear, lambda t: (t["x"] @ t["w0"] + t["b0"],), REL5, REL4,
         "tests/test_gpu_mlp.py::test_mlp_stack_no_bn", grads=["x"], params=["w0", "b0"], reread=["x", "w0"], expand=["b0"], second="pad_cols"),
    Case("batch_norm", "_BatchNormRows", _build_bn, _call_bn, _ref_bn, REL5, REL4, "tests/test_gpu_batchnorm.py::test_batch_norm_matches_fp64",
         grads=["x"], params=["gamma", "beta"], state=["mm", "mv"], reread=["x", "gamma"], expand=["gamma", "beta"], second="sync_bn_relu"),
    Case("sync_bn_relu", "_SyncBNReLU", _build_sync_bn, _call_sync_bn, _ref_sync_bn, REL5, REL4,
         "tests/test_gpu_collective.py::test_fused_sync_bn_two_ranks_equal_the_whole_batch_on_one", grads=["x"], params=["gamma", "beta"],
         state=["mm", "mv"], reread=["x", "gamma"], expand=["gamma", "beta"]),
    Case("conv2d_transpose", "_Deconv2d", _build_deconv, _call_deconv, _ref_deconv, REL5, REL5, "tests/test_gpu_deconv.py::test_against_float64",
         grads=["x"], params=["kernel", "bias"], reread=["x", "kernel"], expand=["bias"]),
    Case("group_point", "_GroupPoint", _build_group, _call_group_point, lambda t: (take(t["points"], t["idx"]),), EXACT, CLOSE5,
         "tests/test_gpu_geometry.py::test_group_point_and_grad", grads=["points"], ints=["idx"], reread=["idx"], targets={"idx": N}),
    Case("group_maxpool", "_GroupMaxpool", _build_group, _call_group_maxpool, lambda t: (take(t["points"], t["idx"]).max(2).values,), EXACT, EXACT,
         "tests/test_gpu_geometry.py::test_group_maxpool_and_selection_sort", grads=["points"], ints=["idx"], int_grads=True, targets={"idx": N}),
    Case("gather_point", "_GatherPoint", _build_gather_point, _call_gather_point, lambda t: (take(t["inp"], t["idx"]),), EXACT, EXACT,
         "tests/test_gpu_geometry.py::test_gather_point_and_grad", grads=["inp"], ints=["idx"], reread=["idx"], int_grads=True, targets={"idx": N}),
    Case("three_interpolate", "_ThreeInterpolate", _build_interpolate, _call_interpolate, _ref_interpolate, CLOSE5, CLOSE5,
         "tests/test_gpu_geometry.py::test_three_interpolate_and_grad", grads=["points"], consts=["weight"], ints=["idx"], reread=["idx", "weight"], targets={"idx": 50}),
    Case("nn_distance", "_NnDistance", _build_nn_distance, _call_nn_distance, _ref_nn_distance, EXACT, EXACT,
         "tests/test_gpu_geometry.py::test_nn_distance_and_grad", grads=["xyz1", "xyz2"], reread=["xyz1", "xyz2"], int_grads=True),
    Case("group_concat", "_GroupConcat", _build_group_concat, _call_group_concat, _ref_group_concat, CLOSE5, CLOSE5,
         "tests/test_gpu_geometry.py::test_group_point_and_grad", grads=["points"], consts=["xyz", "new_xyz"], ints=["idx"], reread=["idx"], targets={"idx": N}),
    Case("fp_concat", "_FpConcat", _build_fp_concat, _call_fp_concat, _ref_fp_concat, CLOSE5, CLOSE5,
         "tests/test_gpu_geometry.py::test_three_interpolate_and_grad", grads=["points2", "points1"], consts=["weight"], ints=["idx"],
         reread=["idx", "weight"], targets={"idx": 50}),
    Case("pad_cols", "_PadCols", lambda: {"x": _randn(_gen(40), 300, 19)}, _call_pad_cols,
         lambda t: (torch.nn.functional.pad(t["x"], (0, 1)),), EXACT, EXACT, "tests/test_gpu_mlp.py::test_pad_rows", grads=["x"], second="tile_linear"),
    Case("points_cropping", "_CropGather", _build_crop_gather, _call_crop_gather, _ref_crop_gather, REL6, REL5,
         "tests/test_gpu_roi.py::test_points_cropping_forward_and_gradients", grads=["pc", "pc_fea", "pc_center"], consts=["rois"], ints=["idx"], reread=["idx"], targets={"idx": N}),
    Case("gather_rows", "_GatherRows", _build_gather_rows, _call_gather_rows, lambda t: (take(t["src"], t["label"]),), EXACT, REL5,
         "tests/test_gpu_spn_net.py::test_instance_feature_gradient_is_a_one_hot_product", grads=["src"], ints=["label"], reread=["label"], targets={"label": 7}),
    Case("crop_linear", "_CropLinearSide", _build_crop, _call_crop_linear, _ref_crop_linear, REL5, REL5,
         "tests/test_gpu_heads.py::test_crop_linear_gradients_against_float64", grads=["pc_fea", "pc_center"], params=["w0", "b0"],
         consts=["pc", "rois"], ints=["idx"], reread=["pc_center", "w0", "pc", "rois", "idx", "pc_fea"], expand=["b0"], declines=["w0"], targets={"idx": N}),
    Case("tile_linear", "_TileAdd", _build_tile, _call_tile, _ref_tile, REL5, REL5, "tests/test_gpu_tile_linear.py::test_tile_linear_against_float64",
         grads=["local", "glob"], params=["w0", "b0"], expand=["b0", "glob"], declines=["w0"], reread=["local", "glob", "w0"], second="mlp_linear"),
]
BY_NAME = {c.name: c for c in CASES}
NODES = sorted({c.node for c in CASES})
