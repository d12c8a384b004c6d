"""GPU tests of shape_proposal_net's two trunks (gspn_amd/spn_trunks.py) and of the nested 3-NN kernel behind their shared geometry:
three_nn_nested against per-level three_nn and the C oracle, spn_geometry against each trunk's own geometry, both trunks against the
oracle composition + the float64 MLP of oracle/mlp_ref.py, the full-feature mode, and a captured training step at full size."""
import numpy as np
import pytest
import torch

from oracle import mlp_ref as R
from oracle import oracle as O
from tests import data as D

pytestmark = pytest.mark.gpu

DECAY = 0.5


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def fresh_store(seed):
    from gspn_amd import tf_util
    return tf_util.set_variable_store(tf_util.VariableStore(seed=seed))


def cloud(kind, b, n, seed0=0):
    if kind == "T":            # exact ties: coordinates on a coarse grid, many duplicates
        return (np.floor(D.batch("U", b, n, seed0) * 6.0) / 4.0).astype(np.float32)
    return D.batch(kind, b, n, seed0)


# ---- 1. three_nn_nested ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,b,n,ordered", [("U", 1, 1, False), ("S", 8, 63, True), ("D", 2, 18000, False), ("T", 8, 18000, True),
                                              ("S", 8, 32768, True), ("U", 8, 32768, False), ("D", 1, 32768, True), ("T", 1, 63, False)])
def test_three_nn_nested_matches_per_level_and_oracle(kind, b, n, ordered):
    from gspn_amd.tf_interpolate import nested_local_maps, nested_members, three_nn, three_nn_nested
    m = 2048
    l1 = cloud(kind, b, m, seed0=11)
    q = cloud(kind, b, n, seed0=23)
    if kind == "T":
        q[:, : min(n, 40)] = l1[:, : min(n, 40)]            # queries ON known points: distance-0 ties
    g = torch.Generator().manual_seed(n + b)
    # general subsets (not prefixes): random FPS-like chains 2048 -> 512 -> 128 -> 32, plus levels of 2 and 1 points
    sizes = (m, 512, 128, 32)
    chain = [torch.stack([torch.randperm(sizes[i], generator=g)[:sizes[i + 1]] for _ in range(b)]).int().cuda() for i in range(3)]
    chain.append(torch.stack([torch.randperm(32, generator=g)[:2] for _ in range(b)]).int().cuda())
    local = nested_local_maps(m, chain, prefixes=(1,))
    members = [torch.arange(m, device="cuda").expand(b, -1)] + nested_members(chain) + [torch.zeros((b, 1), dtype=torch.long, device="cuda")]
    tq, tl1 = torch.from_numpy(q).cuda(), torch.from_numpy(l1).cuda()
    order = torch.stack([torch.randperm(n, generator=g) for _ in range(b)]).int().cuda() if ordered else None
    dist, idx = three_nn_nested(tq, tl1, local, order=order)
    assert tuple(dist.shape) == (len(members), b, n, 3) and idx.dtype == torch.int32
    for lvl, mem in enumerate(members):
        known = torch.gather(tl1, 1, mem.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        d_ref, i_ref = three_nn(tq, known)
        assert torch.equal(dist[lvl].view(torch.int32), d_ref.view(torch.int32)), lvl       # bits, +inf of the short levels included
        assert torch.equal(idx[lvl], i_ref), lvl
        od, oi = O.three_nn(q, known.cpu().numpy())
        np.testing.assert_array_equal(dist[lvl].cpu().numpy().view(np.int32), od.view(np.int32))
        np.testing.assert_array_equal(idx[lvl].cpu().numpy(), oi)


def test_three_nn_nested_rejects_bad_arguments():
    from gspn_amd.tf_interpolate import three_nn_nested
    q = torch.rand(1, 10, 3, device="cuda")
    k = torch.rand(1, 20, 3, device="cuda")
    with pytest.raises(NotImplementedError):
        three_nn_nested(q, k, torch.zeros((9, 1, 20), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        three_nn_nested(q, k, torch.zeros((2, 1, 19), dtype=torch.int32, device="cuda"))


# ---- 2. spn_geometry == each trunk's own geometry ----------------------------------------------------------------------------------------

def _same_sa(a, b):
    assert torch.equal(a.new_xyz, b.new_xyz) and torch.equal(a.idx, b.idx) and torch.equal(a.pts_cnt, b.pts_cnt)


def _same_fp(a, b):
    assert torch.equal(a.idx, b.idx) and torch.equal(a.weight.view(torch.int32), b.weight.view(torch.int32))


@pytest.mark.parametrize("kind,full", [("U", False), ("S", False), ("U", True), ("S", True)])
def test_spn_geometry_equals_each_trunks_own(kind, full):
    from gspn_amd.geometry import fp_geometry, sa_geometry
    from gspn_amd.spn_trunks import SPN_SA_SPEC, spn_geometry
    from gspn_amd.tf_sampling import farthest_point_sample, gather_point
    b, n, ns, nm = 2, 18000, 128, 1024
    xyz = torch.from_numpy(cloud(kind, b, n, 5)).cuda()
    geo = spn_geometry(xyz, ns, nm, return_fullfea=full, points=torch.rand(b, n, 3, device="cuda"))
    # what each trunk computes inline (model_rpointnet.py:91, :148 and the SA / FP modules' own geometry)
    ind_seed, ind_sem = farthest_point_sample(ns, xyz), farthest_point_sample(nm, xyz)
    assert torch.equal(geo["ind_seed"], ind_seed) and torch.equal(geo["ind_sem"], ind_sem)
    cur, own = xyz, []
    for npoint, r, nsample, _ in SPN_SA_SPEC:
        own.append(sa_geometry(cur, npoint, r, nsample))
        cur = own[-1].new_xyz
    for trunk in ("sa_shift", "sa_sem"):
        for a, o in zip(geo[trunk], own):
            _same_sa(a, o)
    assert geo["sa_shift"][0].feat4 is None and geo["sa_sem"][0].feat4 is not None
    l1, l2, l3, l4 = (o.new_xyz for o in own)
    for a, (x1, x2) in zip(geo["fp"], ((l3, l4), (l2, l3), (l1, l2))):
        _same_fp(a, fp_geometry(x1, x2))
    seed, sem = gather_point(xyz, ind_seed), gather_point(xyz, ind_sem)
    _same_fp(geo["fa4_shift"], fp_geometry(torch.cat([seed, xyz], 1) if full else seed, l1))
    _same_fp(geo["fa4_sem"], fp_geometry(torch.cat([seed, sem, xyz], 1) if full else torch.cat([seed, sem], 1), l1))
    if full:
        for a, lk in zip(geo["fpn"], (l4, l3, l2, l1)):
            _same_fp(a, fp_geometry(xyz, lk))
        nested = spn_geometry(xyz, ns, nm, return_fullfea=True, nested=True)
        for a, o in zip(nested["fpn"] + [nested["fa4_shift"], nested["fa4_sem"]], geo["fpn"] + [geo["fa4_shift"], geo["fa4_sem"]]):
            _same_fp(a, o)


# ---- 3./4. both trunks against the oracle composition + the float64 MLP -----------------------------------------------------------------

def _params(store, scope, names, bn=True):
    ps = []
    for nm in names:
        g = lambda k: store.vars["%s/%s/%s" % (scope, nm, k)].detach().double().cpu()
        w = g("weights")
        p = {"name": "%s/%s" % (scope, nm), "w": w.view(w.shape[-2], w.shape[-1]).clone().requires_grad_(True),
             "b": g("biases").clone().requires_grad_(True), "bn": bn}
        if bn:
            p.update(gamma=g("bn/gamma").clone().requires_grad_(True), beta=g("bn/beta").clone().requires_grad_(True),
                     moving_mean=g("bn/moving_mean"), moving_var=g("bn/moving_variance"))
        ps.append(p)
    return ps


def _bidx(idx):
    gi = torch.from_numpy(np.ascontiguousarray(idx).astype(np.int64))
    return torch.arange(gi.shape[0]).view(-1, *([1] * (gi.dim() - 1))).expand_as(gi), gi


def _interp(q, known, p2):
    d, i = O.three_nn(q, known)
    w = R.fp_weights(torch.from_numpy(d).double())
    bi, gi = _bidx(i)
    return (p2[bi, gi] * w[..., None]).sum(2)


class Ref:
    """oracle geometry (C) + float64 layers, the reference's composition of shift_pred_net / sem_net"""

    def __init__(self, store, x, col, ind_seed, ind_sem, training, full):
        from gspn_amd.spn_trunks import SPN_FP_MLP, SPN_SA_SPEC
        self.store, self.training, self.params = store, training, []
        self.x, self.col, self.full = x, col, full
        self.sa, cur = [], x
        for npoint, r, ns, mlp in SPN_SA_SPEC:
            nx = O.gather_point(cur, O.farthest_point_sample(npoint, cur))
            self.sa.append((cur, nx, O.query_ball_point(r, ns, cur, nx)[0], ns, len(mlp)))
            cur = nx
        self.seed_xyz, self.sem_xyz = O.gather_point(x, ind_seed), O.gather_point(x, ind_sem)
        self.ind_seed, self.ind_sem, self.fp_mlp = ind_seed, ind_sem, SPN_FP_MLP

    def stack(self, rows, scope, names, pool=None, bn=True, relu=True):
        ps = _params(self.store, scope, names, bn)
        self.params += ps
        if bn and relu:
            return R.stack(rows, ps, self.training, DECAY, pool)[0]
        y = rows
        for p in ps:
            y = R.layer(y, p["w"], p["b"], p.get("gamma"), p.get("beta"), p.get("moving_mean"), p.get("moving_var"), self.training, DECAY, bn, relu)[0]
        return y

    def levels(self, scope, pts):
        outs = []
        for k, (xyz, nx, idx, ns, nl) in enumerate(self.sa):
            b, m = idx.shape[0], idx.shape[1]
            rows = torch.from_numpy(O.group_point(xyz, idx) - nx[:, :, None, :]).double()
            if pts is not None:
                bi, gi = _bidx(idx)
                rows = torch.cat([rows, pts[bi, gi]], -1)
            pts = self.stack(rows.reshape(b * m * ns, -1), scope + "/layer%d" % (k + 1), ["conv%d" % i for i in range(nl)], pool=ns).view(b, m, -1)
            outs.append(pts)
        return outs

    def fp(self, scope, q, known, p1, p2, mlp):
        cat = _interp(q, known, p2)
        if p1 is not None:
            cat = torch.cat([cat, p1], -1)
        b, n = cat.shape[0], cat.shape[1]
        return self.stack(cat.reshape(b * n, -1), scope, ["conv_%d" % i for i in range(len(mlp))]).view(b, n, -1)

    def fp123(self, scope, lv):
        l1, l2, l3, l4 = (s[1] for s in self.sa)
        p3 = self.fp(scope + "/fa_layer1", l3, l4, lv[2], lv[3], self.fp_mlp[0])
        p2 = self.fp(scope + "/fa_layer2", l2, l3, lv[1], p3, self.fp_mlp[1])
        return self.fp(scope + "/fa_layer3", l1, l2, lv[0], p2, self.fp_mlp[2])

    def shift(self):
        lv = self.levels("shift_predictor", None)
        p1 = self.fp123("shift_predictor", lv)
        q = np.concatenate([self.seed_xyz, self.x], 1) if self.full else self.seed_xyz
        p0 = self.fp("shift_predictor/fa_layer4", q, self.sa[0][1], None, p1, self.fp_mlp[3])
        b, r = p0.shape[0], p0.shape[1]
        return self.stack(p0.reshape(b * r, -1), "shift_predictor", ["conv_shift_pred"], bn=False, relu=False).view(b, r, 4)

    def sem(self, mode):
        col = torch.from_numpy(self.col).double()
        lv = self.levels("sem_predictor", col)
        out = {}
        if self.full:
            for k, lk in enumerate((3, 2, 1, 0)):
                out["sem_fea_full_l%d" % (lk + 1)] = torch.cat([_interp(self.x, self.sa[lk][1], lv[lk]), col], -1)
        p1 = self.fp123("sem_predictor", lv)
        q = [self.seed_xyz, self.sem_xyz] + ([self.x] if self.full else [])
        c = [col[_bidx(self.ind_seed)[0], _bidx(self.ind_seed)[1]], col[_bidx(self.ind_sem)[0], _bidx(self.ind_sem)[1]]] + ([col] if self.full else [])
        p0 = self.fp("sem_predictor/fa_layer4", np.concatenate(q, 1), self.sa[0][1], torch.cat(c, 1), p1, self.fp_mlp[3])
        b, r = p0.shape[0], p0.shape[1]
        net = self.stack(p0.reshape(b * r, -1), "sem_predictor", ["fc1"]).view(b, r, -1)
        ns, nm = self.ind_seed.shape[1], self.ind_sem.shape[1]
        out["sem_fea_seed"], out["sem_fea"] = net[:, :ns], net[:, ns:ns + nm]
        if self.full:
            out["sem_fea_full"] = net[:, ns + nm:]
        if not self.training:                       # dropout is the identity in eval mode
            x = out["sem_fea"] if mode == "training" else out["sem_fea_full"]
            out["sem_class_logits"] = self.stack(x.reshape(-1, x.shape[-1]), "sem_predictor", ["fc2"], bn=False, relu=False).view(b, x.shape[1], -1)
        return out


def _run(xyz, col, ns, nm, ncat, training, full, mode, geometry):
    from gspn_amd.spn_trunks import sem_net, shift_pred_net
    ep = shift_pred_net(xyz, col, ns, {}, 'shift_predictor', training, DECAY, return_fullfea=full, geometry=geometry)
    return sem_net(xyz, col, nm, ncat, ep['ind_seed'], ep, 'sem_predictor', training, DECAY, return_fullfea=full, mode=mode, geometry=geometry)


@pytest.mark.parametrize("tag,n1,n2,c1,c2,mlp,on_sources", [
    ("fa_layer4 shift: 64 seeds onto l1, pre-aggregated", 64, 2048, 0, 128, [128, 128, 128], True),
    ("fa_layer4 sem: 64 + 256 rows onto l1, pre-aggregated", 320, 2048, 3, 128, [128, 128, 128], True),
    ("fa_layer1: 256 + 512 = 768 input channels", 128, 32, 256, 512, [256, 256], False),
    ("fa_layer3", 2048, 512, 64, 256, [256, 128], False),
])
def test_fp_module_at_trunk_shapes(tag, n1, n2, c1, c2, mlp, on_sources):
    """the FP modules of the trunks alone, at their exact shapes, against float64: values 1e-5, every parameter and input gradient 1e-4.
    on_sources: the queries are the first n1 known points (seeds / sem samples ARE l1 points), the few-rows-onto-many case of fa_layer4"""
    from gspn_amd import pointnet_util as PU
    b = 2
    store = fresh_store(99)
    if on_sources:
        xyz2 = cloud("S", b, n2, 3)
        xyz1 = np.ascontiguousarray(xyz2[:, :n1])
    else:
        xyz1 = cloud("S", b, n1, 3)
        xyz2 = cloud("S", b, n2, 7)
    rng = np.random.default_rng(17)
    p1 = rng.standard_normal((b, n1, c1)).astype(np.float32) if c1 else None
    p2 = rng.standard_normal((b, n2, c2)).astype(np.float32)
    g1 = c1 > 4                                      # skip links wider than colours carry a gradient (fa_layer1..3)
    t1 = torch.from_numpy(p1).cuda().requires_grad_(g1) if c1 else None
    t2 = torch.from_numpy(p2).cuda().requires_grad_(True)
    calls = []
    real = PU._fp_stack_preagg
    PU._fp_stack_preagg = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        out = PU.pointnet_fp_module(torch.from_numpy(xyz1).cuda(), torch.from_numpy(xyz2).cuda(), t1, t2, mlp, True, DECAY, 'fa')
    finally:
        PU._fp_stack_preagg = real
    assert bool(calls) == on_sources, "fa_layer4 must take the pre-aggregated first layer, the others must not"
    p2r = torch.from_numpy(p2).double().requires_grad_(True)
    p1r = torch.from_numpy(p1).double().requires_grad_(g1) if c1 else None
    cat = _interp(xyz1, xyz2, p2r)
    cat = torch.cat([cat, p1r], 2) if c1 else cat
    ps = _params(store, 'fa', ['conv_%d' % i for i in range(len(mlp))])
    for p in ps:
        p["moving_mean"] = torch.zeros_like(p["moving_mean"])
        p["moving_var"] = torch.ones_like(p["moving_var"])
    ref = R.stack(cat.reshape(b * n1, -1), ps, True, DECAY, None)[0].view(b, n1, mlp[-1])
    assert rel_err(out, ref) < 1e-5
    g = torch.from_numpy(rng.standard_normal(tuple(ref.shape)))
    ref.backward(g)
    out.backward(g.float().cuda())
    assert rel_err(t2.grad, p2r.grad) < 1e-4
    if g1:
        assert rel_err(t1.grad, p1r.grad) < 1e-4
    for i, p in enumerate(ps):
        for k, var in (("w", "weights"), ("gamma", "bn/gamma"), ("beta", "bn/beta")):
            assert rel_err(store.vars['fa/conv_%d/%s' % (i, var)].grad.view(p[k].shape), p[k].grad) < 1e-4, (i, var)


def test_trunks_training_match_oracle_composition():
    """training mode, per-trunk and shared geometry: values against the oracle composition + float64 layers, eval-mode logits too; the
    parameter gradients of the two geometry paths agree.  (Whole-trunk gradients against float64 are not compared: the seed rows that
    fa_layer4 reads back from l1 carry whole seeds' gradients, and a ReLU entry that the float32 forward and the float64 composition put on
    opposite sides of the kink within rounding -- one such entry measured in shift_predictor/fa_layer3/conv_1 -- moves a parameter gradient
    by up to 10 %.  The modules alone are checked against float64 at these shapes in test_fp_module_at_trunk_shapes.)"""
    from gspn_amd.spn_trunks import spn_geometry
    b, n, ns, nm, ncat = 2, 4096, 64, 256, 9
    x = cloud("S", b, n, 31)
    col = np.random.default_rng(3).random((b, n, 3), dtype=np.float32)
    xyz, tcol = torch.from_numpy(x).cuda(), torch.from_numpy(col).cuda()
    grads = {}
    for shared in (False, True):
        store = fresh_store(41)
        geo = spn_geometry(xyz, ns, nm, points=tcol) if shared else None
        ep = _run(xyz, tcol, ns, nm, ncat, True, False, 'training', geo)
        ind_seed, ind_sem = ep['ind_seed'].cpu().numpy(), ep['ind_sem'].cpu().numpy()
        np.testing.assert_array_equal(ind_seed, O.farthest_point_sample(ns, x))        # the reference's own, separate FPS calls
        np.testing.assert_array_equal(ind_sem, O.farthest_point_sample(nm, x))
        assert tuple(ep['sem_class_logits'].shape) == (b, nm, ncat)
        rng = np.random.default_rng(9)
        outs = [ep['shift_pred_seed_4d'], ep['sem_fea'], ep['sem_fea_seed']]
        sum((o * torch.from_numpy(rng.standard_normal(tuple(o.shape))).float().cuda()).sum() for o in outs).backward()
        grads[shared] = {k: v.grad.clone() for k, v in store.named_parameters() if v.grad is not None}
        for p in store.vars:                        # the forward updated the moving statistics: the reference starts from the initial ones
            if p.endswith("moving_mean"):
                store.vars[p].zero_()
            elif p.endswith("moving_variance"):
                store.vars[p].fill_(1.0)
        ref = Ref(store, x, col, ind_seed, ind_sem, True, False)
        sem = ref.sem('training')
        # float32 through 21 layers with batch statistics: each module alone holds ~5e-7 (test_fp_module_at_trunk_shapes), the composition
        # reaches 1.5e-5 of the largest output (measured); the eval-mode comparisons below hold 1e-5
        errs = [rel_err(g, w) for g, w in zip(outs, [ref.shift(), sem['sem_fea'], sem['sem_fea_seed']])]
        assert max(errs) < 3e-5, errs
        with torch.no_grad():                       # eval mode: dropout is the identity, the layers use the moving statistics
            ep = _run(xyz, tcol, ns, nm, ncat, False, False, 'training', geo)
        ref = Ref(store, x, col, ind_seed, ind_sem, False, False)
        assert rel_err(ep['sem_class_logits'], ref.sem('training')['sem_class_logits']) < 1e-5
        assert rel_err(ep['shift_pred_seed_4d'], ref.shift()) < 1e-5
    assert grads[True].keys() == grads[False].keys() and len(grads[True]) > 100
    for k in grads[True]:
        assert rel_err(grads[True][k], grads[False][k]) < 1e-5, k


def test_trunks_full_feature_eval():
    from gspn_amd.spn_trunks import spn_geometry
    b, n, ns, nm, ncat = 2, 18000, 128, 1024, 20
    x = np.concatenate([cloud("S", 1, n, 2), cloud("U", 1, n, 3) * 4.0], 0)
    col = np.random.default_rng(4).random((b, n, 3), dtype=np.float32)
    store = fresh_store(43)
    xyz, tcol = torch.from_numpy(x).cuda(), torch.from_numpy(col).cuda()
    with torch.no_grad():
        _run(xyz, tcol, ns, nm, ncat, False, True, 'inference', None)        # creates the variables
        gen = torch.Generator().manual_seed(8)
        for k, v in store.vars.items():                                      # non-trivial moving statistics
            if k.endswith("moving_mean"):
                v.copy_(torch.randn(v.shape, generator=gen) * 0.2)
            elif k.endswith("moving_variance"):
                v.copy_(torch.rand(v.shape, generator=gen) + 0.5)
        eps = {}
        for nested in (False, True):
            eps[nested] = _run(xyz, tcol, ns, nm, ncat, False, True, 'inference', spn_geometry(xyz, ns, nm, True, points=tcol, nested=nested))
        inline = _run(xyz, tcol, ns, nm, ncat, False, True, 'inference', None)
    shapes = {'pc_seed': (b, ns, 3), 'shift_pred_seed_4d': (b, ns, 4), 'ind_seed': (b, ns), 'shift_pred_full_4d': (b, n, 4), 'ind_sem': (b, nm),
              'sem_fea_full_l4': (b, n, 515), 'sem_fea_full_l3': (b, n, 259), 'sem_fea_full_l2': (b, n, 131), 'sem_fea_full_l1': (b, n, 67),
              'sem_fea_seed': (b, ns, 128), 'sem_fea': (b, nm, 128), 'sem_fea_full': (b, n, 128), 'sem_class_logits': (b, n, ncat)}
    for ep in (eps[False], eps[True], inline):
        assert {k: tuple(v.shape) for k, v in ep.items()} == shapes
    for k in shapes:                                 # nested 3-NN == per-level 3-NN == inline geometry, bit for bit
        assert torch.equal(eps[True][k], eps[False][k]), k
        assert torch.equal(inline[k], eps[False][k]), k
    ep = eps[True]
    s = 0                                            # scene 0 against the float64 composition (eval mode: no batch coupling)
    ref = Ref(store, x[s:s + 1], col[s:s + 1], ep['ind_seed'][s:s + 1].cpu().numpy(), ep['ind_sem'][s:s + 1].cpu().numpy(), False, True)
    sem = ref.sem('inference')
    assert rel_err(ep['shift_pred_full_4d'][s:s + 1], ref.shift()[:, ns:]) < 1e-5
    for k in ('sem_fea_full_l4', 'sem_fea_full_l3', 'sem_fea_full_l2', 'sem_fea_full_l1', 'sem_fea_seed', 'sem_fea', 'sem_fea_full', 'sem_class_logits'):
        assert rel_err(ep[k][s:s + 1], sem[k]) < 1e-5, k


# ---- 5. captured training step at full size ----------------------------------------------------------------------------------------------

def test_trunks_captured_step_full_size():
    from gspn_amd import parallel
    from gspn_amd.graph import CapturedStep
    from gspn_amd.spn_trunks import spn_geometry
    b, n, ns, nm, ncat = 8, 32768, 128, 1024, 20
    xyz = torch.from_numpy(cloud("S", b, n, 50)).cuda()
    col = torch.rand(b, n, 3, device="cuda")
    store = fresh_store(47)
    geo = spn_geometry(xyz, ns, nm, points=col)
    st = {}

    def step():
        for p in store.parameters():
            p.grad = None
        ep = _run(xyz, col, ns, nm, ncat, True, False, 'training', geo)
        # the logits pass through dropout, whose mask differs between the eager run and a replay: they enter the loss with weight 0
        loss = (ep['shift_pred_seed_4d'].square().mean() + ep['sem_fea'].square().mean() + ep['sem_fea_seed'].square().mean()
                + 0.0 * ep['sem_class_logits'].sum())
        loss.backward()
        if "bucket" not in st:
            st["bucket"] = parallel.FlatGradBucket(store.parameters())
        st["bucket"].flatten()
        st["out"] = [ep['shift_pred_seed_4d'].detach(), ep['sem_fea'].detach(), ep['sem_class_logits'].detach()]
        return loss.detach()

    loss0 = step().clone()
    out0 = [o.clone() for o in st["out"]]
    flat0 = st["bucket"].flat.clone()
    cap = CapturedStep(step)
    st["bucket"].flat.zero_()
    loss1 = cap.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(loss0) and torch.isfinite(flat0).all() and all(bool(torch.isfinite(o).all()) for o in out0)
    assert torch.allclose(loss1, loss0, rtol=1e-6)
    for o1, o0 in zip(st["out"][:2], out0[:2]):
        assert torch.allclose(o1, o0, rtol=1e-5, atol=1e-6)
    assert torch.isfinite(st["out"][2]).all()
    assert torch.allclose(st["bucket"].flat, flat0, rtol=1e-4, atol=1e-7)
