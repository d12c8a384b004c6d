"""GPU tests of gspn_amd/heads.py on csrc/heads.hip: crop_linear and its gradients against float64, the shapes it declines, the two heads
against the same layers called by hand and their crop-fused form against the materialised one on the same variables, fpn_features, and
heads -> get_rpointnet_loss -> backward captured in a graph."""
import pytest
import torch

from tests import heads_ref as HR
from tests.test_gpu_modules import fresh_store

pytestmark = pytest.mark.gpu

DECAY = 0.5
BN = ["bn/beta", "bn/gamma", "bn/moving_mean", "bn/moving_variance"]


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def layer_names(name, bn=True):
    return [name + "/" + v for v in ["weights", "biases"] + (BN if bn else [])]


# ---- 1-3. crop_linear --------------------------------------------------------------------------------------------------------------

CROP_SHAPES = [(2, 300, 20, 5, 33, 64), (1, 64, 1024, 3, 32, 128), (1, 7, 8, 2, 5, 4)]          # B, N, C, R, P, cout


def run_crop_linear(case, normalize, grads=False):
    from gspn_amd.mlp import LayerParams
    from gspn_amd.rpointnet import crop_linear
    pc, fea, cen, rois, idx, w, bias = case
    leaves = [t.cuda().requires_grad_(True) for t in (pc, fea, cen, w, bias)]
    pc_d, fea_d, cen_d, w_d, bias_d = leaves
    y = crop_linear(pc_d, fea_d, cen_d, rois.cuda(), idx.cuda(), LayerParams(w_d, bias_d, False), normalize)
    if grads is False:
        return y
    (y * grads.cuda()).sum().backward()
    assert pc_d.grad is None                                                       # pc is an input: no gradient
    return y, [t.grad.clone() for t in (fea_d, cen_d, w_d, bias_d)]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", CROP_SHAPES)
def test_crop_linear_forward_against_float64(shape, normalize):
    b, n, c, r, p, cout = shape
    case = HR.crop_linear_case(*shape, seed=1)
    rois, idx = case[3], case[4]
    assert not rois[:, -1].any() and not idx[:, -1].any()                          # one all-zero ROI row whose index row is all zeros
    assert all(int(idx[i, k].unique().numel()) < p for i in range(b) for k in range(r))          # duplicate indices in every row
    want = HR.crop_linear(*[t.double() if t.is_floating_point() else t for t in case], normalize)
    got = run_crop_linear(case, normalize)
    assert got.shape == (b, r, p, cout) and got.dtype == torch.float32
    err = rel_err(got, want)
    print("crop_linear %s normalize=%s: relative error %.3g" % (shape, normalize, err))
    assert err <= 1e-5


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", CROP_SHAPES)
def test_crop_linear_gradients_against_float64(shape, normalize):
    b, n, c, r, p, cout = shape
    case = HR.crop_linear_case(*shape, seed=2)
    dy = torch.randn(b, r, p, cout, generator=torch.Generator().manual_seed(7))
    _, got = run_crop_linear(case, normalize, dy)
    pc, fea, cen, rois, idx, w, bias = [t.double() if t.is_floating_point() else t for t in case]
    leaves = [t.requires_grad_(True) for t in (fea, cen, w, bias)]
    (HR.crop_linear(pc, leaves[0], leaves[1], rois, idx, leaves[2], leaves[3], normalize) * dy.double()).sum().backward()
    assert got[2].shape == (c + 6, cout)                                           # all C + 6 weight rows
    for name, g, leaf in zip(("pc_fea", "pc_center", "weights", "biases"), got, leaves):
        err = rel_err(g, leaf.grad)
        print("crop_linear %s normalize=%s gradient %s: relative error %.3g" % (shape, normalize, name, err))
        assert g.shape == leaf.grad.shape and err <= 1e-5, name
    err_side = rel_err(got[2][c:], leaves[2].grad[c:])                              # the six side rows on their own scale
    assert err_side <= 1e-5
    _, again = run_crop_linear(case, normalize, dy)
    for g, h in zip(got, again):
        assert torch.equal(g, h)                                                   # two backward calls give identical bits


HEAD_LISTS = dict(cls=([16, 32], [16, 16]), seg=([16, 16], [16, 32], [16, 16]))
NCAT = 5


def crop_inputs(b, n, c, r, p, seed):
    pc, fea, cen, rois, idx, _, _ = HR.crop_linear_case(b, n, c, r, p, 4, seed=seed)
    return dict(pc=pc.cuda(), pc_fea=fea.cuda(), pc_center=cen.cuda(), rois=rois.cuda(), idx=idx.cuda(), normalize=True)


def materialise(crop):
    from gspn_amd.rpointnet import points_cropping
    b, r, p = crop["idx"].shape
    fea, cen, coord, _ = points_cropping(crop["pc"], crop["pc_fea"], crop["pc_center"], crop["rois"], crop["idx"], r, p, crop["normalize"])
    return coord, torch.cat((fea, cen), -1)


def run_heads(pc, pc_fea, training, crop=None, lists=HEAD_LISTS, bn=True):
    from gspn_amd import rpointnet as RP
    logits, probs, deltas = RP.classification_head(pc, pc_fea, NCAT, lists["cls"][0], lists["cls"][1], training, DECAY, 'classification_head',
                                                   bn=bn, crop=crop)
    masks = RP.segmentation_head(pc, pc_fea, NCAT, lists["seg"][0], lists["seg"][1], lists["seg"][2], training, DECAY, 'segmentation_head',
                                 bn=bn, crop=crop)
    return {"logits": logits, "probs": probs, "bbox_deltas": deltas, "masks": masks}


def test_declined_shape_raises_and_the_head_takes_the_materialised_path():
    from gspn_amd.mlp import LayerParams
    from gspn_amd.rpointnet import crop_linear
    crop = crop_inputs(2, 60, 8, 3, 32, seed=4)
    w = torch.randn(8 + 6, 6, generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.raises(NotImplementedError):
        crop_linear(crop["pc"], crop["pc_fea"], crop["pc_center"], crop["rois"], crop["idx"], LayerParams(w, torch.zeros(6).cuda(), False))
    lists = dict(cls=([6, 8], [8]), seg=([6], [8], [8]))                            # first layers of 6 channels: declined
    pc, pc_fea = materialise(crop)
    fresh_store(21)
    want = run_heads(pc, pc_fea, False, lists=lists)
    fresh_store(21)
    got = run_heads(None, None, False, crop=crop, lists=lists)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ---- 4. the heads on materialised inputs ---------------------------------------------------------------------------------------------

def cls_names(l1, l2):
    return sum([layer_names("classification_head/conv_prev_%d" % i) for i in range(len(l1))], []) + \
        sum([layer_names("classification_head/conv_post_%d" % i) for i in range(len(l2))], []) + \
        layer_names("classification_head/conv_classify", False) + layer_names("classification_head/conv_bbox_regress", False)


def seg_names(l1, l2, l3):
    return sum([layer_names("segmentation_head/conv_prev_%d" % i) for i in range(len(l1))], []) + \
        sum([layer_names("segmentation_head/conv_%d" % i) for i in range(len(l2))], []) + \
        sum([layer_names("segmentation_head/conv_post_%d" % i) for i in range(len(l3))], []) + layer_names("segmentation_head/conv_seg", False)


def heads_by_hand(pc, pc_fea, training, lists=HEAD_LISTS):
    """the same layers through the public tf_util calls of the reference's text (:926-944, :955-978); the post-pool conv1d layers as a linear
    conv1d + batch_norm_for_conv1d + ReLU"""
    from gspn_amd import tf_util
    kw = dict(padding='VALID', bn=True, is_training=training, bn_decay=DECAY)
    b, r, p, _ = pc.shape
    with tf_util.variable_scope('classification_head'):
        x = torch.cat((pc_fea, pc), -1)
        for i, c in enumerate(lists["cls"][0]):
            x = tf_util.conv2d(x, c, [1, 1], stride=[1, 1], scope='conv_prev_%d' % i, **kw)
        x = x.max(dim=2).values
        for i, c in enumerate(lists["cls"][1]):
            x = tf_util.conv1d(x, c, 1, padding='VALID', stride=1, scope='conv_post_%d' % i, activation_fn=None)
            with tf_util.variable_scope('conv_post_%d' % i):
                x = torch.relu(tf_util.batch_norm_for_conv1d(x, training, DECAY, 'bn'))
        logits = tf_util.conv1d(x, NCAT, 1, padding='VALID', stride=1, scope='conv_classify', activation_fn=None)
        deltas = tf_util.conv1d(x, NCAT * 6, 1, padding='VALID', stride=1, scope='conv_bbox_regress', activation_fn=None)
    with tf_util.variable_scope('segmentation_head'):
        x = torch.cat((pc_fea, pc), -1)
        for i, c in enumerate(lists["seg"][0]):
            x = tf_util.conv2d(x, c, [1, 1], stride=[1, 1], scope='conv_prev_%d' % i, **kw)
        local = x
        for i, c in enumerate(lists["seg"][1]):
            x = tf_util.conv2d(x, c, [1, 1], stride=[1, 1], scope='conv_%d' % i, **kw)
        x = torch.cat((x.max(dim=2, keepdim=True).values.expand(-1, -1, p, -1), local), -1).contiguous()
        for i, c in enumerate(lists["seg"][2]):
            x = tf_util.conv2d(x, c, [1, 1], stride=[1, 1], scope='conv_post_%d' % i, **kw)
        masks = tf_util.conv2d(x, NCAT, [1, 1], padding='VALID', stride=[1, 1], scope='conv_seg', activation_fn=None)
    return {"logits": logits, "probs": torch.softmax(logits, 2), "bbox_deltas": deltas.reshape(-1, r, NCAT, 6), "masks": masks}


def head_inputs(b, r, p, nfea, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(b, r, p, 3, generator=g) - 0.5).cuda(), torch.randn(b, r, p, nfea, generator=g).cuda()


# NFEA + 3 input channels: 32 (16-byte rows), 30 (padded rows; held to 1e-5 in both modes: another row pitch may sum in another order)
# and 1030, which is wider than one MLP launch takes
@pytest.mark.parametrize("b,r,p,nfea,bitwise", [(2, 3, 32, 29, True), (2, 3, 33, 27, False), (1, 2, 32, 1027, True)])
def test_heads_materialised_equal_the_layers_by_hand(b, r, p, nfea, bitwise):
    pc, pc_fea = head_inputs(b, r, p, nfea, 31)
    store = fresh_store(22)
    got = run_heads(pc, pc_fea, False)
    assert store.trainable + [] == [n for n in cls_names(*HEAD_LISTS["cls"]) + seg_names(*HEAD_LISTS["seg"]) if "moving" not in n]
    assert list(store.vars) == cls_names(*HEAD_LISTS["cls"]) + seg_names(*HEAD_LISTS["seg"])        # the reference's scopes, in creation order
    assert store.vars["classification_head/conv_prev_0/weights"].shape == (1, 1, nfea + 3, 16)
    assert store.vars["classification_head/conv_post_0/weights"].shape == (1, 32, 16)
    assert store.vars["segmentation_head/conv_post_0/weights"].shape == (1, 1, 32 + 16, 16)
    assert got["logits"].shape == (b, r, NCAT) and got["probs"].shape == (b, r, NCAT) and got["bbox_deltas"].shape == (b, r, NCAT, 6)
    assert got["masks"].shape == (b, r, p, NCAT)
    assert torch.equal(got["probs"], torch.softmax(got["logits"], 2))
    fresh_store(22)
    want = heads_by_hand(pc, pc_fea, False)
    for k in want:
        if bitwise:
            assert torch.equal(got[k], want[k]), k
        else:
            assert rel_err(got[k], want[k]) <= 1e-5, k
    fresh_store(23)
    got = run_heads(pc, pc_fea, True)
    fresh_store(23)
    want = heads_by_hand(pc, pc_fea, True)
    for k in want:
        err = rel_err(got[k], want[k])
        print("heads (%d, %d, %d, %d) training %s: relative error %.3g" % (b, r, p, nfea, k, err))
        assert err <= 1e-5, k
    assert torch.equal(got["probs"], torch.softmax(got["logits"], 2))


# ---- 5. fused against materialised ------------------------------------------------------------------------------------------------------

def reset_moving(store):
    for name, v in store.vars.items():
        if name.endswith("moving_mean"):
            v.zero_()
        elif name.endswith("moving_variance"):
            v.fill_(1.0)


FIRST_BN = ["%s/conv_prev_0/bn/moving_%s" % (h, s) for h in ("classification_head", "segmentation_head") for s in ("mean", "variance")]


@pytest.mark.parametrize("training", [False, True])
def test_fused_heads_equal_materialised_on_the_same_variables(training):
    crop = crop_inputs(2, 300, 24, 6, 32, seed=5)
    pc, pc_fea = materialise(crop)
    store = fresh_store(24)
    want = run_heads(pc, pc_fea, training)
    moving = {k: store.vars[k].clone() for k in FIRST_BN}
    nvars = len(store.vars)
    reset_moving(store)
    got = run_heads(None, None, training, crop=crop)
    assert len(store.vars) == nvars                                                # the same variables: nothing new was created
    for k in want:
        err = rel_err(got[k], want[k])
        print("fused against materialised, training=%s, %s: relative error %.3g" % (training, k, err))
        assert err <= 1e-5, k
    if training:
        for k in FIRST_BN:
            assert rel_err(store.vars[k], moving[k]) <= 1e-5, k
            assert not torch.equal(store.vars[k], torch.zeros_like(moving[k])) and not torch.equal(store.vars[k], torch.ones_like(moving[k]))


@pytest.mark.parametrize("training", [False, True])
def test_fused_heads_backward_reaches_everything_and_repeats(training):
    crop = crop_inputs(2, 300, 24, 6, 32, seed=6)
    crop["pc_fea"].requires_grad_(True)
    crop["pc_center"].requires_grad_(True)
    store = fresh_store(25)
    g = torch.Generator().manual_seed(8)
    weights = {"logits": torch.randn(2, 6, NCAT, generator=g).cuda(), "bbox_deltas": torch.randn(2, 6, NCAT, 6, generator=g).cuda(),
               "masks": torch.randn(2, 6, 32, NCAT, generator=g).cuda()}

    def grads():
        out = run_heads(None, None, training, crop=crop)
        loss = sum((out[k] * w).sum() for k, w in weights.items())
        leaves = [crop["pc_fea"], crop["pc_center"]] + store.parameters()
        return dict(zip(["pc_fea", "pc_center"] + store.trainable, torch.autograd.grad(loss, leaves)))

    first = grads()
    assert len(first) == 2 + len([n for n in cls_names(*HEAD_LISTS["cls"]) + seg_names(*HEAD_LISTS["seg"]) if "moving" not in n])
    for name, gr in first.items():
        assert bool(torch.isfinite(gr).all()), name
        # the biases of a layer that is batch-normalised with batch statistics have a gradient of zero (the mean is subtracted again):
        # every other variable, and every variable in inference mode, must get a non-zero one
        if not (training and name.endswith("/biases") and name.rsplit("/", 1)[0] + "/bn/beta" in first):
            assert float(gr.abs().max()) > 0, name
    again = grads()
    for name in first:
        assert torch.equal(first[name], again[name]), name                        # a second run repeats it bit for bit


# ---- 6. fpn_features ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("training", [False, True])
def test_fpn_features(training):
    from gspn_amd import tf_util
    from gspn_amd.rpointnet import fpn_features
    g = torch.Generator().manual_seed(9)
    widths = {1: 4 + 3, 2: 8 + 3, 3: 16 + 3, 4: 32 + 3}
    ep = {'sem_fea_full_l%d' % i: torch.randn(2, 50, w, generator=g).cuda() for i, w in widths.items()}
    ep['entity_fea'] = torch.randn(2, 50, 12, generator=g).cuda()
    store = fresh_store(26)
    got = fpn_features(ep, training, DECAY)
    assert got.shape == (2, 50, 12 + 4 * 64)
    assert list(store.vars) == sum([layer_names("fpn%d" % i) for i in (1, 2, 3, 4)], [])
    assert torch.equal(got[..., :12], ep['entity_fea'])
    fresh_store(26)
    for i in (1, 2, 3, 4):
        want = tf_util.conv1d(ep['sem_fea_full_l%d' % i], 64, 1, padding='VALID', bn=True, is_training=training, scope='fpn%d' % i, bn_decay=DECAY)
        assert torch.equal(got[..., 12 + 64 * (i - 1):12 + 64 * i], want), i
    assert float(got[..., 12:].min()) == 0.0                                       # behind a ReLU


# ---- 7. the chain, captured --------------------------------------------------------------------------------------------------------

def test_heads_loss_backward_captured():
    from gspn_amd import rpointnet as RP
    from gspn_amd.graph import CapturedStep
    b, n, r, p, c = 2, 2000, 16, 64, 64
    crop = crop_inputs(b, n, c, r, p, seed=10)
    crop["pc_fea"].requires_grad_(True)
    crop["pc_center"].requires_grad_(True)
    cfg = RP.Config()
    cfg.NUM_CATEGORY, cfg.NUM_POINT_INS_MASK, cfg.TRAIN_ROIS_PER_IMAGE = NCAT, p, r
    g = torch.Generator().manual_seed(11)
    cls = torch.zeros(b, r, dtype=torch.int32)
    cls[:, :5] = torch.randint(1, NCAT, (b, 5), generator=g).int()                  # positives first, negatives, the last ROI is padding
    targets = {"rois": crop["rois"], "target_class_ids": cls.cuda(), "target_bbox": torch.randn(b, r, 6, generator=g).cuda(),
               "target_mask": (torch.rand(b, r, p, generator=g) < 0.4).cuda()}
    lists = dict(cls=([128, 256, 512], [256, 256]), seg=([64, 64], [64, 128, 512], [256, 256]))       # the reference's widths (:1110, :1115)
    store = fresh_store(27)
    st = {}

    def step():
        crop["pc_fea"].grad = crop["pc_center"].grad = None
        for v in store.parameters():
            v.grad = None
        out = run_heads(None, None, True, crop=crop, lists=lists)
        ep = dict(targets, rpointnet_class_logits=out["logits"], rpointnet_class=out["probs"], rpointnet_bbox=out["bbox_deltas"],
                  rpointnet_mask=out["masks"])
        loss, ep = RP.get_rpointnet_loss(ep, cfg)
        loss.backward()
        st["terms"] = [ep[k].detach() for k in ("rpointnet_class_loss", "rpointnet_bbox_loss", "rpointnet_mask_loss")]
        return loss.detach()

    loss0 = step().clone()
    terms0 = [t.clone() for t in st["terms"]]
    g_fea0, g_cen0 = crop["pc_fea"].grad.clone(), crop["pc_center"].grad.clone()
    g_w0 = store.vars["classification_head/conv_prev_0/weights"].grad.clone()
    cap = CapturedStep(step)                                                       # the capture itself proves that nothing synchronises with the host
    loss1 = cap.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(loss0) and float(loss0) > 0 and torch.allclose(loss1, loss0, rtol=1e-6)
    assert all(float(t) > 0 for t in terms0)
    for a, w in zip(st["terms"], terms0):
        assert torch.allclose(a, w, rtol=1e-6)
    assert float(g_fea0.abs().max()) > 0 and float(g_cen0.abs().max()) > 0 and float(g_w0.abs().max()) > 0
    assert rel_err(crop["pc_fea"].grad, g_fea0) <= 1e-5 and rel_err(crop["pc_center"].grad, g_cen0) <= 1e-5
    assert rel_err(store.vars["classification_head/conv_prev_0/weights"].grad, g_w0) <= 1e-5
