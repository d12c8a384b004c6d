"""GPU tests of gspn_amd/inference.py: crop_mean (gspn_crop_mean of csrc/crop_mean.hip) against float64, the shapes it declines, and the
driver rpointnet_inference at a small operating point -- keys, shapes and variable names, every output bit-equal to the same parts chained by
hand, the glue against the restatements of tests/inference_ref.py and tests/detect_ref.py, the crop-fused heads against the materialised
ones, the whole call captured in a graph with a seed bumped on the device, and a scene without a single proposal."""
import pytest
import torch

from tests import detect_ref as DR
from tests import inference_ref as IR
from tests import test_gpu_heads as TH
from tests import test_gpu_spn_net as TS
from tests.test_gpu_modules import fresh_store

pytestmark = pytest.mark.gpu

rel_err = TH.rel_err


# ---- a, b. crop_mean ------------------------------------------------------------------------------------------------------------------

CROP_MEAN_SHAPES = [(2, 300, 5, 64, 20), (1, 257, 3, 1, 1), (3, 50, 7, 33, 5), (2, 1000, 4, 1000, 19), (1, 4096, 2, 4096, 64)]      # b, n, r, p, c


def crop_mean_case(b, n, r, p, c, seed, scale=None):
    """table (b, n, c) uniform in [0, 1) (or scale * randn) and idx (b, r, p) with, in scene 0: the all-zero row 0; a row that names one
    point p times (row 1; with only two rows the all-zero row is that row, and it names point 0); and the indices -1 and n, which are
    clamped (in row min(2, r - 1); with one point per row, n is what the constant row names).  -> table, idx, (row, point) of the
    constant row"""
    g = torch.Generator().manual_seed(seed)
    table = torch.rand(b, n, c, generator=g) if scale is None else scale * torch.randn(b, n, c, generator=g)
    idx = torch.randint(0, n, (b, r, p), generator=g).int()
    idx[0, 0] = 0
    const, mixed = (0, 0), min(2, r - 1)
    if r >= 3:
        k = n if p == 1 else n // 2
        idx[0, 1] = k
        const = (1, min(k, n - 1))
    idx[0, mixed, 0] = -1
    if p > 1:
        idx[0, mixed, 1] = n
    assert not idx[0, 0].any() and bool((idx == -1).any()) and bool((idx == n).any())
    return table, idx, const


@pytest.mark.parametrize("shape,scale", [(s, None) for s in CROP_MEAN_SHAPES] + [(CROP_MEAN_SHAPES[3], 1e4)])
def test_crop_mean_against_float64(shape, scale):
    """the bound: the sum is exact to double rounding (p <= 4096 terms of 24 bits each), so the one rounding to float leaves at most
    2**-24 of the value, within 2**-22 of the largest one"""
    from gspn_amd.rpointnet import crop_mean
    b, n, r, p, c = shape
    table, idx, (row, point) = crop_mean_case(*shape, seed=11, scale=scale)
    want = IR.crop_mean(table, idx)
    got = crop_mean(table.cuda(), idx.cuda())
    assert got.shape == (b, r, c) and got.dtype == torch.float32
    err = rel_err(got, want)
    print("crop_mean %s scale %s: relative error %.3g" % (shape, scale, err))
    assert err <= 2.0 ** -22
    assert torch.equal(got[0, row].cpu(), table[0, point])                         # one point p times: exactly that table row
    assert torch.equal(got[0, 0].cpu(), table[0, 0])                               # the all-zero row: point 0, no masking
    assert torch.equal(crop_mean(table.cuda(), idx.cuda()), got)                   # a second call repeats the bits


def test_crop_mean_declines_and_rejects():
    from gspn_amd.rpointnet import crop_mean
    idx = torch.zeros(2, 3, 4, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        crop_mean(torch.zeros(2, 8, 65, device="cuda"), idx)
    with pytest.raises(ValueError):
        crop_mean(torch.zeros(3, 8, 20, device="cuda"), idx)                       # another batch size
    with pytest.raises(ValueError):
        crop_mean(torch.zeros(2, 8, 20, device="cuda"), idx.long())
    with pytest.raises(ValueError):
        crop_mean(torch.zeros(2, 8, device="cuda"), idx)
    assert crop_mean(torch.ones(2, 8, 64, device="cuda"), idx).eq(1).all()         # the widest table it takes


# ---- c. the driver at a small operating point -----------------------------------------------------------------------------------------

B, N, NGROUP, NINS, NCAT = TS.B, TS.N, TS.NGROUP, TS.NINS, TS.NCAT                   # 2, 4096, 12, 512, 9
NSMP, M, P, D = 64, 32, 64, 16
STORE_SEED = 106          # chosen on the device: every scene then has at least 4 detections and at least one empty row (asserted below)
SEED = 3
CLS_LISTS = ([128, 256, 512], [256, 256])
SEG_LISTS = ([64, 64], [64, 128, 512], [256, 256])


def small_config(**over):
    from gspn_amd.rpointnet import Config

    class SmallConfig(Config):
        NUM_CATEGORY = NCAT
        NUM_GROUP = NGROUP
        NUM_POINT = N
        NUM_SAMPLE = NSMP
        SPN_PRE_NMS_LIMIT = 48
        SPN_NMS_MAX_SIZE_INFERENCE = M
        NUM_POINT_INS_MASK = P
        DETECTION_MAX_INSTANCES = D
        DETECTION_MIN_CONFIDENCE = 0          # freshly initialised heads never reach 0.7

    cfg = SmallConfig()
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def scene_args(sc):
    return (sc["pc"], sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], sc["seg_label"], sc["bbox_ins"])


def tensors(ep):
    return {k: v.clone() for k, v in ep.items() if isinstance(v, torch.Tensor)}


class Run:
    def __init__(self, store_seed=STORE_SEED, seed=SEED, cfg=None):
        from gspn_amd.rpointnet import rpointnet_inference
        self.sc = TS.scene()
        self.cfg = cfg or small_config()
        self.store = fresh_store(store_seed)
        self.ep = rpointnet_inference(*scene_args(self.sc), self.cfg, seed=seed)
        self.names = list(self.store.vars)


@pytest.fixture(scope="module")
def run():
    return Run()


EXTRA_KEYS = {
    'group_label': (B, N), 'seg_label': (B, N), 'seg_label_per_group': (B, NGROUP), 'bbox_ins': (B, NGROUP, 6),                        # :1194-1197
    'selected_indices': (B, M), 'spn_rois': (B, M, 6), 'rois': (B, M, 6), 'rpointnet_class_logits': (B, M, NCAT),                       # :1211-1220
    'rpointnet_class': (B, M, NCAT), 'rpointnet_bbox': (B, M, NCAT, 6), 'detections': (B, D, 8), 'rpointnet_mask': (B, D, P, NCAT),
    'rpointnet_mask_selected': (B, D, P), 'pc_coord_cropped_final_unnormalized': (B, D, P, 3),
    'fb_prob_cropped': (B, M), 'sem_prob_cropped': (B, M),                                                                            # :1149, :1163
    'mask_selection_idx': (B, M, P), 'rois_final': (B, D, 6), 'mask_selection_idx_final': (B, D, P),                                    # extensions
}


def test_driver_keys_shapes_and_variable_names(run):
    shapes = {**TS.KEYS, **TS.TRUNK_KEYS, **TS.FULL_KEYS, **EXTRA_KEYS}
    assert set(run.ep) == set(shapes)
    for k, shape in shapes.items():
        assert tuple(run.ep[k].shape) == shape, k
        assert not run.ep[k].requires_grad, k
    for k in ('selected_indices', 'mask_selection_idx', 'mask_selection_idx_final', 'seg_label_per_group'):
        assert run.ep[k].dtype == torch.int32, k
    fpn = sum([TH.layer_names("fpn%d" % i) for i in (1, 2, 3, 4)], [])
    assert run.names == TS.expected_variable_names() + fpn + TH.cls_names(*CLS_LISTS) + TH.seg_names(*SEG_LISTS)
    assert tuple(run.store.vars["classification_head/conv_prev_0/weights"].shape) == (1, 1, 1024 + 6, 128)      # the features stay 1024 wide


def first_max(values):
    """the first maximal column, by counting the columns in front of it"""
    eq = values == values.max(-1, keepdim=True).values
    return (eq.cumsum(-1) == 0).sum(-1)


def by_hand(sc, cfg, seed, store_seed):
    """:1064-1221 for mode='inference' restated from the public parts, in the reference's order"""
    from gspn_amd import rpointnet as RP
    pc = sc["pc"]
    fresh_store(store_seed)
    with torch.no_grad():
        ep = RP.shape_proposal_net(pc, sc["color"], sc["pc_ins"], sc["group_label"], sc["group_indicator"], cfg.NUM_CATEGORY, 'shape_proposal_net',
                                   False, bn_decay=None, nsmp=cfg.NUM_SAMPLE, return_fullfea=True, mode='inference')
        ep['seg_label_per_group'] = RP.seg_label_per_group(sc["seg_label"], sc["group_label"], cfg.NUM_GROUP)
        sel = RP.nms_3d(ep['bbox_ins_pred'], ep['fb_prob'][:, :, 1], cfg.SPN_PRE_NMS_LIMIT, M, cfg.SPN_IOU_THRESHOLD, cfg.SPN_SCORE_THRESHOLD)
        spn_rois = RP.gather_selection(ep['bbox_ins_pred'], sel, M)
        rois, idx = RP.mask_selection_gen_batch(spn_rois, pc, M, cfg, True, seed)
        fea = RP.fpn_features(ep, False, None)
        near = RP.nearest_in_sets(pc, ep['pc_seed'])[:, 0].long()
        table = torch.cat((torch.gather(ep['fb_prob'][:, :, 1], 1, near).unsqueeze(-1), torch.softmax(ep['sem_class_logits'], -1)), -1)
        means = RP.crop_mean(table, idx)
        fea_c, cen_c, coord_c, _ = RP.points_cropping(pc, fea, ep['center_pos'], rois, idx, M, P, cfg.NORMALIZE_CROP_REGION)
        logits, probs, deltas = RP.classification_head(coord_c, torch.cat((fea_c, cen_c), -1), cfg.NUM_CATEGORY, *CLS_LISTS, False, None,
                                                       'classification_head')
        fb_c = means[:, :, 0].contiguous()
        sem_c = torch.gather(means[:, :, 1:], 2, first_max(logits).unsqueeze(-1)).squeeze(-1)
        det = RP.refine_detections_batch(rois, probs, deltas, pc, fb_c, sem_c, cfg)
        rois_f, idx_f = RP.mask_selection_gen_batch(det[:, :, :6], pc, D, cfg, False, seed + 1)
        fea_c, cen_c, coord_c, unnorm = RP.points_cropping(pc, fea, ep['center_pos'], rois_f, idx_f, D, P, cfg.NORMALIZE_CROP_REGION)
        mask = RP.segmentation_head(coord_c, torch.cat((fea_c, cen_c), -1), cfg.NUM_CATEGORY, *SEG_LISTS, False, None, 'segmentation_head')
        ep.update(selected_indices=sel, spn_rois=spn_rois, rois=rois, mask_selection_idx=idx, fb_prob_cropped=fb_c, sem_prob_cropped=sem_c,
                  rpointnet_class_logits=logits, rpointnet_class=probs, rpointnet_bbox=deltas, detections=det, rois_final=rois_f,
                  mask_selection_idx_final=idx_f, pc_coord_cropped_final_unnormalized=unnorm, rpointnet_mask=mask,
                  rpointnet_mask_selected=RP.select_segmentation(torch.sigmoid(mask), det[:, :, 6]))
        return ep


def detection_rows(det):
    return (det.abs().sum(-1) != 0).sum(1)


def test_driver_bit_equal_to_the_parts_chained_by_hand(run):
    found = detection_rows(run.ep['detections'])
    print("detections per scene at store seed %d: %s of %d" % (STORE_SEED, found.tolist(), D))
    assert bool((found >= 4).all()) and bool((found < D).all())                     # not vacuous: real rows and padding in every scene
    want = by_hand(run.sc, run.cfg, SEED, STORE_SEED)
    assert set(want) == set(run.ep) - {'group_label', 'seg_label', 'bbox_ins'}
    for k, w in want.items():
        assert torch.equal(run.ep[k], w), k
    for k in ('group_label', 'seg_label', 'bbox_ins'):
        assert run.ep[k] is run.sc[k]


def test_driver_glue_against_the_restatements(run):
    from gspn_amd.detect import classified_boxes
    ep = {k: v.cpu() for k, v in run.ep.items()}
    pc = run.sc["pc"].cpu()
    # the per-ROI probabilities (:1136-1150, :1159-1162) from what the call returned
    means = IR.crop_mean(IR.point_probabilities(pc, ep['pc_seed'], ep['fb_prob'], ep['sem_class_logits']), ep['mask_selection_idx'])
    err_fb = rel_err(ep['fb_prob_cropped'], means[:, :, 0])
    err_sem = rel_err(ep['sem_prob_cropped'], IR.first_max_pick(means[:, :, 1:], ep['rpointnet_class_logits']))
    print("fb_prob_cropped: relative error %.3g, sem_prob_cropped: %.3g" % (err_fb, err_sem))
    assert err_fb <= 1e-5 and err_sem <= 1e-5
    assert float(ep['fb_prob_cropped'].min()) > 0 and float(ep['sem_prob_cropped'].max()) < 1
    # the selected masks (:1191)
    probs = torch.sigmoid(run.ep['rpointnet_mask']).cpu()
    assert torch.equal(ep['rpointnet_mask_selected'], DR.select_segmentation(probs, ep['detections'][:, :, 6]))
    # the detections (:818-913): exact from the device's own refined boxes on (exp differs by an ulp between host and device)
    ids, scores, refined = classified_boxes(run.ep['rois'], run.ep['rpointnet_class'], run.ep['rpointnet_bbox'], run.sc["pc"], run.cfg)
    want_ids, want_scores = DR.first_argmax(ep['rpointnet_class'])
    assert torch.equal(ids.cpu(), want_ids) and torch.equal(scores.cpu(), want_scores)
    want = DR.refine_detections(refined.cpu(), ids.cpu(), scores.cpu(), ep['fb_prob_cropped'], ep['sem_prob_cropped'],
                                run.cfg.DETECTION_MIN_CONFIDENCE, D, run.cfg.DETECTION_NMS_THRESHOLD)
    assert torch.equal(ep['detections'], want)
    # the first crop draws inside its ROIs (within mask_selection_gen's margin), and padding rows name point 0
    rois, idx = ep['rois'], ep['mask_selection_idx']
    pts = torch.gather(pc, 1, idx.reshape(B, -1, 1).long().expand(-1, -1, 3)).reshape(B, M, P, 3)
    live = rois.abs().sum(-1) != 0
    inside = ((pts - rois[:, :, None, :3]).abs() <= rois[:, :, None, 3:] / 2 + 2e-3).all(-1).all(-1)
    assert bool(live.any()) and bool(inside[live].all()) and not bool(idx[~live].any())
    assert torch.equal(ep['rois_final'], ep['detections'][:, :, :6])
    assert torch.equal(ep['pc_coord_cropped_final_unnormalized'],
                       torch.gather(pc, 1, ep['mask_selection_idx_final'].reshape(B, -1, 1).long().expand(-1, -1, 3)).reshape(B, D, P, 3))


# ---- d. fused against materialised -------------------------------------------------------------------------------------------------------

def test_fused_crop_against_materialised(run):
    from gspn_amd import tf_util
    from gspn_amd.rpointnet import rpointnet_inference
    tf_util.set_variable_store(run.store)                                          # the same variables
    TH.reset_moving(run.store)
    got = rpointnet_inference(*scene_args(run.sc), run.cfg, seed=SEED, fused_crop=True)
    assert list(run.store.vars) == run.names                                       # nothing new was created
    for k in ('rpointnet_class_logits', 'rpointnet_bbox'):
        err = rel_err(got[k], run.ep[k])
        print("fused against materialised %s: relative error %.3g" % (k, err))
        assert err <= 1e-5, k
    for k in ('rois', 'mask_selection_idx', 'selected_indices', 'spn_rois', 'fb_prob_cropped', 'sem_prob_cropped'):
        assert torch.equal(got[k], run.ep[k]), k                                   # they do not depend on the heads' values
    assert set(got) == set(run.ep) and got['rpointnet_mask_selected'].shape == (B, D, P)
    assert bool(torch.isfinite(got['rpointnet_mask_selected']).all())


# ---- e. capture --------------------------------------------------------------------------------------------------------------------------

def test_driver_captured_with_a_device_seed():
    from gspn_amd.graph import CapturedStep
    from gspn_amd.rpointnet import rpointnet_inference
    from gspn_amd.shape_proposal import valid_instances
    from gspn_amd.spn_trunks import spn_geometry
    sc, cfg = TS.scene(), small_config()
    geo = spn_geometry(sc["pc"], cfg.NUM_SAMPLE, TS.SEM, True, points=sc["color"])
    valid = valid_instances(sc["group_indicator"])
    seed = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    fresh_store(STORE_SEED)
    st = {}

    def step():
        st["ep"] = rpointnet_inference(*scene_args(sc), cfg, geometry=geo, valid_idx=valid, seed=seed)

    step()
    eager = tensors(st["ep"])
    cap = CapturedStep(step)                                                       # the capture itself proves that nothing synchronises with the host
    cap.replay()
    torch.cuda.synchronize()
    assert set(st["ep"]) == set(eager)
    for k, w in eager.items():
        assert torch.equal(st["ep"][k], w), k
    seed.add_(1)
    cap.replay()
    torch.cuda.synchronize()
    bumped = tensors(st["ep"])
    assert torch.equal(bumped['rois'], eager['rois'])
    assert not torch.equal(bumped['mask_selection_idx'], eager['mask_selection_idx'])
    step()                                                                         # eager, at the bumped seed
    for k, w in st["ep"].items():
        assert torch.equal(bumped[k], w), k


# ---- f. a scene without a proposal ------------------------------------------------------------------------------------------------------

def test_scene_with_no_foreground_proposal(run):
    """a score threshold between the two scenes' best proposals: the weaker scene keeps no proposal, all its ROIs are padding.  As in the
    reference, a padding ROI that the classification head puts in a foreground class would still come out as one row (an all-zero box with
    that class and its score, :846-908): STORE_SEED was chosen among the seeds at which these freshly initialised heads call the padding
    ROI background (seed 77, the first with 4..15 detections per scene, put it in class 6 and returned such a row; seed 106 does not)."""
    from gspn_amd import tf_util
    from gspn_amd.rpointnet import rpointnet_inference
    best = run.ep['fb_prob'][:, :, 1].max(1).values.cpu()
    empty = int(best.argmin())
    assert float(best[empty]) < float(best[1 - empty])
    cfg = small_config(SPN_SCORE_THRESHOLD=float((best[0].double() + best[1].double()) / 2))
    tf_util.set_variable_store(run.store)
    ep = rpointnet_inference(*scene_args(run.sc), cfg, seed=SEED)
    assert bool((ep['selected_indices'][empty] == -1).all()) and bool((ep['selected_indices'][1 - empty] >= 0).any())
    assert not ep['rois'][empty].any() and not ep['mask_selection_idx'][empty].any()
    assert bool(ep['rois'][1 - empty].any())
    assert not ep['detections'][empty].any()
    assert bool(torch.isfinite(ep['rpointnet_mask_selected']).all()) and bool(torch.isfinite(ep['rpointnet_mask']).all())
    assert tuple(ep['rpointnet_mask_selected'].shape) == (B, D, P)
