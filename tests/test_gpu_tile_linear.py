"""GPU tests of csrc/tile_linear.hip and what heads.py builds on it: gspn_tile_add against the fp32 broadcast add (bit for bit),
gspn_tile_sum against the float64 sum, the shapes both decline, tile_linear and its gradients against a float64 restatement of
cat(tile(global), local) . W + b, segmentation_head(split_post=True) against the materialised concatenation on the same variables, and the
shared first layer of both heads against the two heads called separately."""
import pytest
import torch

from tests import test_gpu_heads as TH
from tests.test_gpu_modules import fresh_store

pytestmark = pytest.mark.gpu

rel_err = TH.rel_err

# groups, p, c: one group, one row; p below the row groups of a workgroup and no multiple of them; c / 4 no power of two; more columns than
# one 256-lane pass of floats; the real shape cut down; the widest row.  (3, 256, 256) and (2, 130, 260) spread a group over several
# workgroups and take the join kernel, the others do not.
SHAPES = [(1, 1, 4), (7, 3, 20), (5, 67, 64), (3, 256, 256), (2, 130, 260), (4, 64, 1024)]


def _lib():
    from gspn_amd import _lib as L
    return L


def tile_add(a, g, y, groups, p, c):
    L = _lib()
    return L.lib().gspn_tile_add(groups, p, c, L.ptr(a), L.ptr(g), L.ptr(y), L.stream())


def tile_sum(dy, groups, p, c, dg=None):
    L = _lib()
    lib = L.lib()
    dg = torch.empty(groups, c, device="cuda") if dg is None else dg
    nfloats = int(lib.gspn_tile_sum_part_floats(groups, p, c))
    part = torch.empty(nfloats, device="cuda") if nfloats else None
    rc = lib.gspn_tile_sum(groups, p, c, L.ptr(dy), L.ptr(part), L.ptr(dg), L.stream())
    return rc, dg


def test_the_cases_cover_both_paths_of_tile_sum():
    lib = _lib().lib()
    split = [int(lib.gspn_tile_sum_part_floats(*s)) > 0 for s in SHAPES]
    assert split == [False, False, True, True, True, False]


@pytest.mark.parametrize("shape", SHAPES)
def test_tile_add_is_the_fp32_broadcast_add(shape):
    groups, p, c = shape
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(groups * p, c, generator=gen).cuda()
    g = torch.randn(groups, c, generator=gen).cuda()
    want = (a.view(groups, p, c) + g.view(groups, 1, c)).view(groups * p, c)
    y = torch.full_like(a, float("nan"))
    assert tile_add(a, g, y, groups, p, c) == 0
    assert torch.equal(y, want)
    inplace = a.clone()
    assert tile_add(inplace, g, inplace, groups, p, c) == 0                        # Y == A
    assert torch.equal(inplace, want)


SUM_BOUND = 2.0 ** -23          # one rounding of a double sum (which is itself exact to far below that)


def within_one_rounding(got, want64):
    err = (got.double().cpu() - want64).abs()
    return bool((err <= SUM_BOUND * want64.abs() + 1e-30).all()), float((err / (want64.abs() + 1e-30)).max())


@pytest.mark.parametrize("scale,mean", [(1.0, 0.0), (1e4, 1e4)])
@pytest.mark.parametrize("shape", SHAPES)
def test_tile_sum_against_float64(shape, scale, mean):
    groups, p, c = shape
    dy = torch.randn(groups * p, c, generator=torch.Generator().manual_seed(4)) * scale + mean
    want = dy.double().view(groups, p, c).sum(1)
    rc, got = tile_sum(dy.cuda(), groups, p, c)
    assert rc == 0
    ok, worst = within_one_rounding(got, want)
    print("tile_sum %s scale %g mean %g: largest relative error %.3g" % (shape, scale, mean, worst))
    assert ok
    rc, again = tile_sum(dy.cuda(), groups, p, c)
    assert rc == 0 and torch.equal(again, got)                                     # two calls: the same bits


@pytest.mark.parametrize("groups,p,c", [(3, 256, 256), (2, 64, 20), (1, 1024, 1024)])
def test_tile_sum_of_identical_rows_is_exact(groups, p, c):
    row = torch.randn(groups, 1, c, generator=torch.Generator().manual_seed(5))
    dy = row.expand(groups, p, c).reshape(groups * p, c).contiguous()
    rc, got = tile_sum(dy.cuda(), groups, p, c)
    assert rc == 0 and torch.equal(got.cpu(), (row[:, 0] * p))                     # p a power of two: p * row is exact


def test_declined_before_any_launch():
    L = _lib()
    lib = L.lib()
    POISON = 12345.0
    for c in (6, 1028):
        a = torch.zeros(2 * 3, c, device="cuda")
        g = torch.zeros(2, c, device="cuda")
        y = torch.full_like(a, POISON)
        dg = torch.full_like(g, POISON)
        assert tile_add(a, g, y, 2, 3, c) == -2
        assert tile_sum(a, 2, 3, c, dg)[0] == -2
        assert int(lib.gspn_tile_sum_part_floats(2, 3, c)) == 0
        torch.cuda.synchronize()
        assert bool((y == POISON).all()) and bool((dg == POISON).all())
    # a pointer that is only 4-byte aligned, in every position
    c, groups, p = 8, 2, 3
    base = torch.zeros(groups * p * c + 4, device="cuda")
    off = base[1:1 + groups * p * c].view(groups * p, c)
    assert off.data_ptr() % 16 == 4
    a = torch.zeros(groups * p, c, device="cuda")
    gbase = torch.zeros(groups * c + 4, device="cuda")
    goff = gbase[1:1 + groups * c].view(groups, c)
    g = torch.zeros(groups, c, device="cuda")
    base.fill_(POISON)
    gbase.fill_(POISON)
    y = torch.full_like(a, POISON)
    assert tile_add(off, g, y, groups, p, c) == -2
    assert tile_add(a, goff, y, groups, p, c) == -2
    assert tile_add(a, g, off, groups, p, c) == -2
    assert tile_sum(off, groups, p, c, torch.full_like(g, POISON))[0] == -2
    assert tile_sum(a, groups, p, c, goff)[0] == -2
    assert tile_add(a, g, y, 0, p, c) == -1 and tile_add(a, g, y, groups, 0, c) == -1
    assert lib.gspn_tile_add(groups, p, c, None, L.ptr(g), L.ptr(y), L.stream()) == -1
    assert tile_add(a, g, y, 1 << 20, 1 << 11, c) == -2                            # groups * p = 2^31
    torch.cuda.synchronize()
    assert bool((y == POISON).all()) and bool((base == POISON).all()) and bool((gbase == POISON).all())


# ---- tile_linear ---------------------------------------------------------------------------------------------------------------------

TILE_LINEAR_SHAPES = [(3, 5, 8, 4, 8), (4, 67, 512, 64, 256), (2, 16, 12, 20, 36)]          # g, p, cg, cl, cout


def tile_linear_case(g, p, cg, cl, cout, seed):
    gen = torch.Generator().manual_seed(seed)
    local = torch.randn(g * p, cl, generator=gen)
    glob = torch.randn(g, cg, generator=gen)
    w = torch.randn(cg + cl, cout, generator=gen) / (cg + cl) ** 0.5
    bias = torch.randn(cout, generator=gen)
    dy = torch.randn(g * p, cout, generator=gen)
    return local, glob, w, bias, dy


def tile_linear_ref(local, glob, w, bias, p):
    g = glob.shape[0]
    rows = torch.cat((glob.view(g, 1, -1).expand(-1, p, -1), local.view(g, p, -1)), -1).reshape(g * p, -1)
    return rows @ w + bias


def run_tile_linear(case, p):
    from gspn_amd.mlp import LayerParams
    from gspn_amd.rpointnet import tile_linear
    leaves = [t.cuda().requires_grad_(True) for t in case[:4]]
    y = tile_linear(leaves[0], leaves[1], LayerParams(leaves[2], leaves[3], False), p)
    (y * case[4].cuda()).sum().backward()
    return y.detach(), [t.grad.clone() for t in leaves]


@pytest.mark.parametrize("shape", TILE_LINEAR_SHAPES)
def test_tile_linear_against_float64(shape):
    g, p, cg, cl, cout = shape
    case = tile_linear_case(*shape, seed=6)
    got, grads = run_tile_linear(case, p)
    leaves = [t.double().requires_grad_(True) for t in case[:4]]
    want = tile_linear_ref(*leaves, p)
    (want * case[4].double()).sum().backward()
    assert got.shape == (g * p, cout) and got.dtype == torch.float32
    err = rel_err(got, want)
    print("tile_linear %s: relative error %.3g" % (shape, err))
    assert err <= 1e-5
    assert grads[2].shape == (cg + cl, cout)                                       # all weight rows
    for name, gr, leaf in zip(("local", "global", "weights", "biases"), grads, leaves):
        err = rel_err(gr, leaf.grad)
        print("tile_linear %s gradient %s: relative error %.3g" % (shape, name, err))
        assert gr.shape == leaf.grad.shape and err <= 1e-5, name
    assert rel_err(grads[2][:cg], leaves[2].grad[:cg]) <= 1e-5 and rel_err(grads[2][cg:], leaves[2].grad[cg:]) <= 1e-5
    _, again = run_tile_linear(case, p)
    for a, b in zip(grads, again):
        assert torch.equal(a, b)                                                   # two backward calls give identical bits


def test_tile_linear_declines_before_anything_runs():
    from gspn_amd.mlp import LayerParams
    from gspn_amd.rpointnet import tile_linear
    local, glob = torch.zeros(2 * 4, 4, device="cuda"), torch.zeros(2, 8, device="cuda")
    with pytest.raises(NotImplementedError):
        tile_linear(local, glob, LayerParams(torch.zeros(12, 6, device="cuda"), torch.zeros(6, device="cuda"), False), 4)
    with pytest.raises(ValueError):
        tile_linear(local, glob, LayerParams(torch.zeros(12, 8, device="cuda"), torch.zeros(8, device="cuda"), False), 3)
    with pytest.raises(ValueError):
        tile_linear(local, glob, LayerParams(torch.zeros(13, 8, device="cuda"), torch.zeros(8, device="cuda"), False), 4)


def grad_rel_err(name, got, want, training):
    """rel_err on the tensor's own scale.  One kind of tensor has no scale of its own: the biases in front of a batch norm that runs on
    batch statistics.  The mean is subtracted again, so their true gradient is zero and what either form returns is the rounding noise of
    the column sum of the batch norm's input gradient; it is measured against the layer's beta gradient, the same column sum before the
    mean was taken out."""
    beta = name.rsplit("/", 1)[0] + "/bn/beta"
    if training and name.endswith("/biases") and beta in want:
        return float((got[name].double() - want[name].double()).abs().max() / want[beta].double().abs().max())
    return rel_err(got[name], want[name])


# ---- segmentation_head(split_post=True) ------------------------------------------------------------------------------------------------

SEG = TH.HEAD_LISTS["seg"]
POST0 = "segmentation_head/conv_post_0/bn/moving_"


def run_seg(pc, pc_fea, training, crop=None, split_post=False):
    from gspn_amd import rpointnet as RP
    return RP.segmentation_head(pc, pc_fea, TH.NCAT, SEG[0], SEG[1], SEG[2], training, TH.DECAY, 'segmentation_head', crop=crop,
                                split_post=split_post)


@pytest.mark.parametrize("through_crop", [False, True])
@pytest.mark.parametrize("training", [False, True])
def test_split_post_equals_the_materialised_concat(training, through_crop):
    b, r, p, c = 2, 3, 16, 20
    crop = TH.crop_inputs(b, 200, c, r, p, seed=7)
    pc, pc_fea = (None, None) if through_crop else TH.materialise(crop)
    kw = dict(crop=crop) if through_crop else {}
    dmask = torch.randn(b, r, p, TH.NCAT, generator=torch.Generator().manual_seed(8)).cuda()
    store = fresh_store(31)

    def run(split):
        TH.reset_moving(store)
        masks = run_seg(pc, pc_fea, training, split_post=split, **kw)
        grads = torch.autograd.grad((masks * dmask).sum(), store.parameters())
        return masks.detach(), dict(zip(store.trainable, grads)), {s: store.vars[POST0 + s].clone() for s in ("mean", "variance")}

    want, want_grads, want_moving = run(False)
    names = list(store.vars)
    assert names == TH.seg_names(*SEG)
    got, got_grads, got_moving = run(True)
    assert list(store.vars) == names                                               # the same variables, in the same order
    err = rel_err(got, want)
    print("split_post training=%s crop=%s masks: relative error %.3g" % (training, through_crop, err))
    assert err <= 1e-5
    for name in store.trainable:
        err = grad_rel_err(name, got_grads, want_grads, training)
        print("split_post training=%s crop=%s gradient %s: relative error %.3g" % (training, through_crop, name, err))
        assert err <= 1e-5, name
    for s in ("mean", "variance"):
        assert rel_err(got_moving[s], want_moving[s]) <= 1e-5, s
    if training:
        assert not torch.equal(got_moving["mean"], torch.zeros_like(got_moving["mean"]))


def test_split_post_declined_shape_takes_the_materialised_path():
    pc, pc_fea = TH.head_inputs(2, 3, 16, 13, 9)
    lists = ([8], [8], [6, 8])                                                     # conv_post_0 with 6 output channels: declined
    from gspn_amd import rpointnet as RP
    fresh_store(32)
    want = RP.segmentation_head(pc, pc_fea, TH.NCAT, *lists, False, None, 'segmentation_head')
    fresh_store(32)
    got = RP.segmentation_head(pc, pc_fea, TH.NCAT, *lists, False, None, 'segmentation_head', split_post=True)
    assert torch.equal(got, want)


# ---- the shared first layer --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("training", [False, True])
def test_shared_first_layer_equals_the_two_heads_called_separately(training, monkeypatch):
    from gspn_amd import heads, tf_util
    from gspn_amd.pointnet_util import _mlp_layers
    b, n, c, r, p = 2, 300, 24, 6, 32
    crop = TH.crop_inputs(b, n, c, r, p, seed=10)
    crop["pc_fea"].requires_grad_(True)
    crop["pc_center"].requires_grad_(True)
    gen = torch.Generator().manual_seed(11)
    weights = {"logits": torch.randn(b, r, TH.NCAT, generator=gen).cuda(), "bbox_deltas": torch.randn(b, r, TH.NCAT, 6, generator=gen).cuda(),
               "masks": torch.randn(b, r, p, TH.NCAT, generator=gen).cuda()}
    built = []
    real = heads._Lists

    class CountingLists(real):
        def __init__(self, *a, **kw):
            built.append(1)
            real.__init__(self, *a, **kw)

    monkeypatch.setattr(heads, "_Lists", CountingLists)
    lists = TH.HEAD_LISTS

    def backward(out, store):
        loss = sum((out[k] * w).sum() for k, w in weights.items())
        leaves = [crop["pc_fea"], crop["pc_center"]] + store.parameters()
        return dict(zip(["pc_fea", "pc_center"] + store.trainable, torch.autograd.grad(loss, leaves)))

    store = fresh_store(33)
    want = TH.run_heads(None, None, training, crop=crop)
    assert len(built) == 2                                                         # one set of inverse lists per head
    want_grads = backward(want, store)
    want_names = list(store.vars)
    want_moving = {k: store.vars[k].clone() for k in TH.FIRST_BN}

    del built[:]
    store = fresh_store(33)                                                        # fresh: the creation order is under test too
    cls_layer = heads.declare_classification_head(c + 6, TH.NCAT, lists["cls"][0], lists["cls"][1], 'classification_head')
    with tf_util.variable_scope('segmentation_head'):
        seg_layer = _mlp_layers(lists["seg"][0][:1], c + 6, 'conv_prev_', True)[0]
    cls_rows, seg_rows = heads.shared_first_layers(crop, cls_layer, seg_layer, training, TH.DECAY)
    assert cls_rows.shape == (b * r * p, lists["cls"][0][0]) and seg_rows.shape == (b * r * p, lists["seg"][0][0])
    from gspn_amd import rpointnet as RP
    logits, probs, deltas = RP.classification_head(None, None, TH.NCAT, lists["cls"][0], lists["cls"][1], training, TH.DECAY,
                                                   'classification_head', crop=dict(crop, first=cls_rows))
    masks = RP.segmentation_head(None, None, TH.NCAT, *lists["seg"], training, TH.DECAY, 'segmentation_head', crop=dict(crop, first=seg_rows))
    got = {"logits": logits, "probs": probs, "bbox_deltas": deltas, "masks": masks}
    assert len(built) == 1                                                         # ONE set of inverse lists
    assert list(store.vars) == want_names and store.trainable == [k for k in want_names if "moving" not in k]
    got_grads = backward(got, store)
    for k in want:
        err = rel_err(got[k], want[k])
        print("shared first layer training=%s %s: relative error %.3g" % (training, k, err))
        assert err <= 1e-5, k
    for k in want_grads:
        err = grad_rel_err(k, got_grads, want_grads, training)
        print("shared first layer training=%s gradient %s: relative error %.3g" % (training, k, err))
        assert err <= 1e-5, k
    if training:
        for k in TH.FIRST_BN:
            assert rel_err(store.vars[k], want_moving[k]) <= 1e-5, k
