"""GPU tests of gspn_amd/training.py at the small operating point of tests/test_gpu_inference.py (restated here): 2 x 4096 points, 64 seeds,
SPN_NMS_MAX_SIZE_TRAINING 32, TRAIN_ROIS_PER_IMAGE 16, NUM_POINT_INS_MASK 64.  Keys, shapes, dtypes and variable names; every output
bit-equal to the parts chained by hand; which variables get a gradient; and, on planted proposals -- freshly initialised ones match no
ground truth, so the box and mask terms would be tested at 0 --, the losses against float64 restatements, the three switches against the
materialised form, and the step captured in a graph with a seed bumped on the device."""
import pytest
import torch

from tests import heads_ref as HR
from tests import test_gpu_heads as TH
from tests import test_gpu_spn_net as TS
from tests.test_gpu_modules import fresh_store
from tests.test_gpu_tile_linear import grad_rel_err

pytestmark = pytest.mark.gpu

rel_err = TH.rel_err

B, N, NGROUP, NINS, NCAT = TS.B, TS.N, TS.NGROUP, TS.NINS, TS.NCAT                   # 2, 4096, 12, 512, 9
NSMP, M, R, P = 64, 32, 16, 64
DECAY = 0.5
STORE_SEED = 61
SEED = 3
ALPHA = 0.7
CLS_LISTS = ([128, 256, 512], [256, 256])
SEG_LISTS = ([64, 64], [64, 128, 512], [256, 256])
HEAD_SCOPES = ("fpn1/", "fpn2/", "fpn3/", "fpn4/", "classification_head/", "segmentation_head/")


def small_config(**over):
    from gspn_amd.rpointnet import Config

    class SmallConfig(Config):
        NUM_CATEGORY = NCAT
        NUM_GROUP = NGROUP
        NUM_POINT = N
        NUM_SAMPLE = NSMP
        SPN_PRE_NMS_LIMIT = 48
        SPN_NMS_MAX_SIZE_TRAINING = M
        TRAIN_ROIS_PER_IMAGE = R
        NUM_POINT_INS_MASK = P
        TRAIN_MODULE = ['RPOINTNET']

    cfg = SmallConfig()
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def scene_args(sc):
    return (sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], sc["seg_label"], sc["bbox_ins"])


def make_noise():
    return torch.randn(B, NSMP, 256, generator=torch.Generator().manual_seed(12)).cuda()


def proposals(sc, cfg, noise, **kw):
    """the frozen proposal net of :1070, as rpointnet_head_training calls it"""
    from gspn_amd.rpointnet import shape_proposal_net
    with torch.no_grad():
        return shape_proposal_net(sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], cfg.NUM_CATEGORY,
                                  'shape_proposal_net', False, bn_decay=None, nsmp=cfg.NUM_SAMPLE, return_fullfea=True, mode='training',
                                  noise=noise, **kw)


class Run:
    def __init__(self):
        from gspn_amd.rpointnet import rpointnet_head_training
        self.sc = TS.scene()
        self.cfg = small_config()
        self.noise = make_noise()
        self.store = fresh_store(STORE_SEED)
        self.ep = rpointnet_head_training(*scene_args(self.sc), self.cfg, True, DECAY, noise=self.noise, seed=SEED)
        self.names = list(self.store.vars)


@pytest.fixture(scope="module")
def run():
    return Run()


EXTRA_KEYS = {
    'group_label': (B, N), 'seg_label': (B, N), 'seg_label_per_group': (B, NGROUP), 'bbox_ins': (B, NGROUP, 6),                        # :1194-1197
    'selected_indices': (B, M), 'spn_rois': (B, M, 6), 'rois': (B, R, 6), 'target_class_ids': (B, R), 'target_bbox': (B, R, 6),        # :1199-1209
    'target_mask_selection_idx': (B, R, P), 'target_mask': (B, R, P), 'rpointnet_class_logits': (B, R, NCAT), 'rpointnet_class': (B, R, NCAT),
    'rpointnet_bbox': (B, R, NCAT, 6), 'rpointnet_mask': (B, R, P, NCAT),
}
REFERENCE_ORDER = ['group_label', 'seg_label', 'seg_label_per_group', 'bbox_ins', 'selected_indices', 'spn_rois', 'rois', 'target_class_ids',
                   'target_bbox', 'target_mask_selection_idx', 'target_mask', 'rpointnet_class_logits', 'rpointnet_class', 'rpointnet_bbox',
                   'rpointnet_mask']


def expected_names():
    fpn = sum([TH.layer_names("fpn%d" % i) for i in (1, 2, 3, 4)], [])
    return TS.expected_variable_names() + fpn + TH.cls_names(*CLS_LISTS) + TH.seg_names(*SEG_LISTS)


def test_driver_keys_shapes_dtypes_and_variable_names(run):
    # mode='training' with full features: the semantic logits stay those of the sampled points, which the semantic loss reads
    shapes = {**TS.KEYS, **TS.FULL_KEYS, **TS.TRUNK_KEYS, **EXTRA_KEYS}
    assert set(run.ep) == set(shapes)
    assert list(run.ep)[-len(REFERENCE_ORDER):] == REFERENCE_ORDER                 # stored in the reference's order, behind the proposal net's
    for k, shape in shapes.items():
        assert tuple(run.ep[k].shape) == shape, k
    for k in ('selected_indices', 'target_mask_selection_idx', 'seg_label_per_group', 'target_class_ids'):
        assert run.ep[k].dtype == torch.int32, k
    assert run.ep['target_mask'].dtype == torch.bool
    for k in ('rois', 'spn_rois', 'target_bbox', 'rpointnet_class_logits', 'rpointnet_class', 'rpointnet_bbox', 'rpointnet_mask'):
        assert run.ep[k].dtype == torch.float32, k
    for k in list(TS.KEYS) + list(TS.FULL_KEYS) + ['rois', 'target_bbox', 'spn_rois']:
        assert not run.ep[k].requires_grad, k                                      # dict_stop_gradient; targets carry no graph
    for k in ('rpointnet_class_logits', 'rpointnet_class', 'rpointnet_bbox', 'rpointnet_mask'):
        assert run.ep[k].requires_grad, k
    assert run.names == expected_names()
    assert tuple(run.store.vars["segmentation_head/conv_post_0/weights"].shape) == (1, 1, 512 + 64, 256)


def by_hand(ep, sc, cfg, seed, training):
    """:1074-1115 restated from the public parts, in the reference's order, behind the proposal net's end_points"""
    from gspn_amd import rpointnet as RP
    pc = sc["pc"]
    ep = dict(ep)
    per = RP.seg_label_per_group(sc["seg_label"], sc["group_label"], cfg.NUM_GROUP)
    sel = RP.nms_3d(ep['bbox_ins_pred'], ep['fb_prob'][:, :, 1], cfg.SPN_PRE_NMS_LIMIT, M, cfg.SPN_IOU_THRESHOLD, cfg.SPN_SCORE_THRESHOLD)
    spn_rois = RP.gather_selection(ep['bbox_ins_pred'], sel, M)
    rois, cls, tbox, idx, tmask = RP.detection_target_gen_batch(spn_rois, per, sc["bbox_ins"], sc["group_label"], pc, cfg, seed)
    fea = RP.fpn_features(ep, training, DECAY)
    fea_c, cen_c, coord_c, _ = RP.points_cropping(pc, fea, ep['center_pos'], rois, idx, R, P, cfg.NORMALIZE_CROP_REGION)
    head_fea = torch.cat((fea_c, cen_c), -1)
    logits, probs, deltas = RP.classification_head(coord_c, head_fea, cfg.NUM_CATEGORY, *CLS_LISTS, training, DECAY, 'classification_head')
    mask = RP.segmentation_head(coord_c, head_fea, cfg.NUM_CATEGORY, *SEG_LISTS, training, DECAY, 'segmentation_head')
    ep.update(seg_label_per_group=per, selected_indices=sel, spn_rois=spn_rois, rois=rois, target_class_ids=cls, target_bbox=tbox,
              target_mask_selection_idx=idx, target_mask=tmask, rpointnet_class_logits=logits, rpointnet_class=probs, rpointnet_bbox=deltas,
              rpointnet_mask=mask)
    return ep


def test_driver_bit_equal_to_the_parts_chained_by_hand(run):
    """the driver on the freshly initialised net, whose proposals match no ground truth (every ROI row is padding), and
    rpointnet_heads_from_proposals on planted proposals, where the rows are positives and negatives"""
    from gspn_amd.rpointnet import rpointnet_heads_from_proposals
    fresh_store(STORE_SEED)
    want = by_hand(proposals(run.sc, run.cfg, run.noise), run.sc, run.cfg, SEED, True)
    assert set(want) == set(run.ep) - {'group_label', 'seg_label', 'bbox_ins'}
    for k, w in want.items():
        assert torch.equal(run.ep[k], w), k
    for k in ('group_label', 'seg_label', 'bbox_ins'):
        assert run.ep[k] is run.sc[k]
    sc = run.sc
    fresh_store(STORE_SEED)
    ep0 = plant(proposals(sc, run.cfg, run.noise), sc, run.cfg)
    got = rpointnet_heads_from_proposals(ep0, sc["pc"], sc["group_label"], sc["seg_label"], sc["bbox_ins"], run.cfg, True, DECAY, seed=SEED)
    pos, neg = positives_and_negatives(got)
    assert bool((pos >= 4).all()) and bool((neg >= 4).all())                       # not vacuous
    fresh_store(STORE_SEED)
    want = by_hand(plant(proposals(sc, run.cfg, run.noise), sc, run.cfg), sc, run.cfg, SEED, True)
    for k, w in want.items():
        assert torch.equal(got[k], w), k


def test_driver_equals_proposal_net_plus_heads_from_proposals(run):
    from gspn_amd.rpointnet import rpointnet_heads_from_proposals
    fresh_store(STORE_SEED)
    ep = proposals(run.sc, run.cfg, run.noise)
    sc = run.sc
    got = rpointnet_heads_from_proposals(ep, sc["pc"], sc["group_label"], sc["seg_label"], sc["bbox_ins"], run.cfg, True, DECAY, seed=SEED)
    assert list(got) == list(run.ep)
    for k, w in run.ep.items():
        assert torch.equal(got[k], w), k


# ---- planted proposals ---------------------------------------------------------------------------------------------------------------

def plant(ep, sc, cfg):
    """end_points whose proposals match the ground truth: the seeds 0..NUM_GROUP-1 of the groups that have a box of non-zero size (an ROI of
    size 0 divides its crop by 0, here as in the reference) and a foreground class
    carry that box exactly (IoU 1), every other seed a cube of side 0.3 about a point of the scene -- it holds that point, and against
    ground-truth boxes of more than a unit in every direction its IoU is below 0.03.  Scores fall with the seed index, so NMS meets the
    ground-truth boxes first.  All on the device, static shapes (the captured step plants inside its graph)."""
    from gspn_amd.rpointnet import seg_label_per_group
    pc, gt = sc["pc"], sc["bbox_ins"]
    per = seg_label_per_group(sc["seg_label"], sc["group_label"], cfg.NUM_GROUP)
    fg = ((per > 0) & (gt[:, :, 3:].amin(-1) > 0)).unsqueeze(-1)
    at = (torch.arange(NSMP, device=pc.device) * 61 + 7) % N
    centres = pc[:, at]
    boxes = torch.cat((centres, torch.full_like(centres, 0.3)), -1)
    boxes = torch.cat((torch.where(fg, gt, boxes[:, :NGROUP]), boxes[:, NGROUP:]), 1)
    score = torch.linspace(0.99, 0.01, NSMP, device=pc.device).expand(B, -1)
    out = dict(ep)
    out['bbox_ins_pred'] = boxes.contiguous()
    out['fb_prob'] = torch.stack((1 - score, score), -1).contiguous()
    return out


def positives_and_negatives(ep):
    valid = ep['rois'].abs().sum(-1) != 0
    cls = ep['target_class_ids']
    return (valid & (cls > 0)).sum(1), (valid & (cls == 0)).sum(1)


class Planted:
    """one store, the planted end_points and the four forms run on them in training mode"""
    FORMS = {"materialised": {}, "fused_crop": dict(fused_crop=True), "shared_first": dict(fused_crop=True, shared_first=True),
             "split_post": dict(fused_crop=True, shared_first=True, split_post=True)}

    def __init__(self):
        self.sc = TS.scene()
        self.cfg = small_config()
        self.store = fresh_store(STORE_SEED)
        self.ep0 = plant(proposals(self.sc, self.cfg, make_noise()), self.sc, self.cfg)
        self.results = {}

    def heads(self, training=True, seed=SEED, **switches):
        from gspn_amd import tf_util
        from gspn_amd.rpointnet import rpointnet_heads_from_proposals
        tf_util.set_variable_store(self.store)
        sc = self.sc
        return rpointnet_heads_from_proposals(self.ep0, sc["pc"], sc["group_label"], sc["seg_label"], sc["bbox_ins"], self.cfg, training, DECAY,
                                              seed=seed, **switches)

    def form(self, name):
        """(end_points with the losses, {variable: gradient}) of a form, computed once"""
        from gspn_amd.rpointnet import get_head_training_loss
        if name not in self.results:
            ep = self.heads(**self.FORMS[name])
            loss, ep = get_head_training_loss(ep, self.cfg, ALPHA, self.sc["smpw"])
            params = [(n, v) for n, v in self.store.named_parameters() if n.startswith(HEAD_SCOPES)]
            grads = torch.autograd.grad(loss, [v for _, v in params])
            self.results[name] = (ep, {n: g for (n, _), g in zip(params, grads)})
        return self.results[name]


@pytest.fixture(scope="module")
def planted():
    return Planted()


def test_planted_proposals_give_positive_and_negative_rois(planted):
    ep, _ = planted.form("materialised")
    pos, neg = positives_and_negatives(ep)
    print("planted proposals: positive ROIs per scene %s, negative %s of %d" % (pos.tolist(), neg.tolist(), R))
    assert bool((pos >= 4).all()) and bool((neg >= 4).all())
    assert bool(ep['target_mask'].any()) and float(ep['target_bbox'].abs().max()) < 1e-5          # exact boxes: (next to) zero deltas


def test_losses_against_float64_restatements(planted):
    from gspn_amd.rpointnet import get_loss
    ep, _ = planted.form("materialised")
    pos, neg = positives_and_negatives(ep)
    assert bool((pos >= 4).all()) and bool((neg >= 4).all())
    c = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in ep.items() if isinstance(v, torch.Tensor)}
    valid = (c['rois'].abs().sum(-1) != 0).double()
    cls = c['target_class_ids']
    want = {
        'rpointnet_class_loss': HR.class_loss(c['rpointnet_class_logits'], cls, valid),
        'rpointnet_bbox_loss': HR.bbox_loss(c['target_bbox'], cls, c['rpointnet_bbox'], valid, NCAT)[0],
        'rpointnet_mask_loss': HR.mask_loss(c['target_mask'], cls, c['rpointnet_mask'], valid, NCAT, P),
    }
    for k, w in want.items():
        err = abs(float(ep[k].detach()) - float(w)) / abs(float(w))
        print("%s: %.9g vs %.9g, relative error %.3g" % (k, float(ep[k].detach()), float(w), err))
        assert float(w) > 0 and err <= 1e-5, k
    total = ep['rpointnet_class_loss'] + ep['rpointnet_bbox_loss'] + ep['rpointnet_mask_loss']
    assert torch.equal(ep['loss'], total)                                          # :1399
    # the five SPN terms: get_loss's on the same end_points, bit for bit
    spn_cfg = small_config(TRAIN_MODULE=['SPN'])
    heads_ep = planted.heads()
    _, spn = get_loss(dict(heads_ep), spn_cfg, ALPHA, planted.sc["smpw"])
    for k in ('spn_class_loss', 'recons_loss', 'shift_loss', 'sem_loss', 'kl_loss'):
        assert torch.equal(ep[k], spn[k].detach()), k
        assert bool(torch.isfinite(ep[k])) and not ep[k].requires_grad, k
    assert torch.equal(ep['spn_match'], spn['spn_match']) and torch.equal(ep['sem_labels'], spn['sem_labels'])


def test_only_the_fpn_layers_and_the_heads_get_gradients(planted):
    """inference-mode batch norm, so that no bias sits in front of a subtracted batch mean: every variable of the FPN layers and the heads
    must get a finite, non-zero gradient, no variable of the proposal net any"""
    from gspn_amd.rpointnet import get_head_training_loss
    for v in planted.store.parameters():
        v.grad = None
    ep = planted.heads(training=False)
    loss, _ = get_head_training_loss(ep, planted.cfg, ALPHA, planted.sc["smpw"])
    loss.backward()
    seen = 0
    for name, v in planted.store.named_parameters():
        if name.startswith("shape_proposal_net/"):
            assert v.grad is None, name
        else:
            assert name.startswith(HEAD_SCOPES), name
            assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0, name
            seen += 1
    assert seen == len([n for n in expected_names() if n.startswith(HEAD_SCOPES) and "moving" not in n])
    for v in planted.store.parameters():
        v.grad = None


@pytest.mark.parametrize("name", ["fused_crop", "shared_first", "split_post"])
def test_switches_against_the_materialised_form(planted, name):
    want_ep, want = planted.form("materialised")
    nvars = list(planted.store.vars)
    got_ep, got = planted.form(name)
    assert list(planted.store.vars) == nvars                                       # the same variables: nothing new was created
    for k in ('rois', 'target_class_ids', 'target_bbox', 'target_mask_selection_idx', 'target_mask'):
        assert torch.equal(got_ep[k], want_ep[k]), k
    for k in ('loss', 'rpointnet_class_loss', 'rpointnet_bbox_loss', 'rpointnet_mask_loss'):
        err = rel_err(got_ep[k], want_ep[k])
        print("%s against materialised, %s: relative error %.3g" % (name, k, err))
        assert err <= 1e-5, k
    assert set(got) == set(want)
    for k in want:
        err = grad_rel_err(k, got, want, True)
        print("%s against materialised, gradient %s: relative error %.3g" % (name, k, err))
        assert err <= 1e-5, k


def test_shared_first_on_a_fresh_store_creates_the_variables_in_the_reference_order():
    from gspn_amd.rpointnet import rpointnet_head_training
    sc, cfg = TS.scene(), small_config()
    store = fresh_store(STORE_SEED)
    rpointnet_head_training(*scene_args(sc), cfg, True, DECAY, noise=make_noise(), seed=SEED, shared_first=True, split_post=True)
    assert list(store.vars) == expected_names()


# ---- capture -------------------------------------------------------------------------------------------------------------------------

def test_step_captured_with_a_device_seed():
    from gspn_amd.graph import CapturedStep
    from gspn_amd.rpointnet import get_head_training_loss, rpointnet_heads_from_proposals
    from gspn_amd.shape_proposal import valid_instances
    from gspn_amd.spn_trunks import spn_geometry
    sc, cfg = TS.scene(), small_config()
    geo = spn_geometry(sc["pc"], cfg.NUM_SAMPLE, TS.SEM, True, points=sc["color"])
    valid = valid_instances(sc["group_indicator"])
    noise = make_noise()
    seed = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    store = fresh_store(STORE_SEED)
    st = {}
    keep = ('rois', 'target_class_ids', 'target_mask_selection_idx', 'rpointnet_class_logits', 'rpointnet_bbox', 'rpointnet_mask', 'loss',
            'spn_class_loss', 'kl_loss')

    def step():
        for v in store.parameters():
            v.grad = None
        ep = plant(proposals(sc, cfg, noise, geometry=geo, valid_idx=valid), sc, cfg)
        ep = rpointnet_heads_from_proposals(ep, sc["pc"], sc["group_label"], sc["seg_label"], sc["bbox_ins"], cfg, True, DECAY, seed=seed,
                                            fused_crop=True, shared_first=True, split_post=True)
        loss, ep = get_head_training_loss(ep, cfg, ALPHA, sc["smpw"])
        loss.backward()
        st["ep"] = {k: ep[k].detach() for k in keep}
        st["grads"] = {n: v.grad for n, v in store.named_parameters() if v.grad is not None}
        return loss.detach()

    step()
    eager = {k: v.clone() for k, v in st["ep"].items()}
    eager_grads = {n: g.clone() for n, g in st["grads"].items()}
    assert all(n.startswith(HEAD_SCOPES) for n in eager_grads) and len(eager_grads) > 0
    cap = CapturedStep(step)                                                       # the capture itself proves that nothing synchronises with the host
    cap.replay()
    torch.cuda.synchronize()
    for k, w in eager.items():
        assert torch.equal(st["ep"][k], w), k
    for n, w in eager_grads.items():
        assert torch.equal(st["grads"][n], w), n
    seed.add_(1)
    cap.replay()
    torch.cuda.synchronize()
    assert not torch.equal(st["ep"]['target_mask_selection_idx'], eager['target_mask_selection_idx'])
    assert bool(torch.isfinite(st["ep"]['loss']))


# ---- the guard -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("modules", [['SPN'], ['SPN', 'RPOINTNET']])
def test_guard(modules):
    from gspn_amd.rpointnet import get_head_training_loss, rpointnet_head_training, rpointnet_heads_from_proposals
    sc, cfg = TS.scene(), small_config(TRAIN_MODULE=modules)
    store = fresh_store(STORE_SEED)
    with pytest.raises(NotImplementedError, match="TRAIN_MODULE"):
        rpointnet_head_training(*scene_args(sc), cfg, True)
    with pytest.raises(NotImplementedError, match="TRAIN_MODULE"):
        rpointnet_heads_from_proposals({}, sc["pc"], sc["group_label"], sc["seg_label"], sc["bbox_ins"], cfg, True)
    with pytest.raises(NotImplementedError, match="TRAIN_MODULE"):
        get_head_training_loss({}, cfg, 1.0, sc["smpw"])
    assert not store.vars                                                          # before anything has run
