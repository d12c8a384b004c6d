"""GPU tests of gspn_amd/predict.py on the kernels of csrc/predict.hip: gspn_scene_confidence against the exact sums of
tests/predict_ref.py (below, at and across the workgroup's stride of 256 points), the double threshold of the masks, gspn_scene_rank on the
device's own confidences against the ordering restatement (ties, empty scenes, a scene of the second group only, confidences equal to a
threshold, the declined R = 1025), scene_predictions end to end against the literal restatement of test.py:155-205 and its files, the stage
behind rpointnet_inference and captured in a graph with it, and gspn_sem_iou_counts against the loop of train.py:365-368."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import detect_ref as DR
from tests import predict_ref as PR

pytestmark = pytest.mark.gpu


def cuda(ep):
    return {k: v.cuda() for k, v in ep.items()}


def host_tables(pc, ep):
    """predict_ref.point_tables for every scene -> sem_prob (B, N, C), point_fb (B, N) float32 numpy"""
    both = [PR.point_tables(pc[i].numpy(), ep["sem_class_logits"][i].numpy(), ep["pc_seed"][i].numpy(), ep["fb_prob"][i].numpy())
            for i in range(pc.shape[0])]
    return np.stack([s for s, _ in both]), np.stack([f for _, f in both])


def class_ids_of(ep):
    return ep["detections"][:, :, 6].int()


def host_idx(pc, ep):
    return DR.nearest_in_sets(pc, ep["pc_coord_cropped_final_unnormalized"], ep["detections"][:, :, :6].contiguous())


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- gspn_scene_confidence ----------------------------------------------------------------------------------------------------------------

CONFIDENCE_SHAPES = [(1, 1, 1, 1, 2), (2, 3, 257, 5, 19), (2, 5, 1000, 64, 19), (1, 4, 4099, 256, 19)]          # b, r, n, p, c


@pytest.mark.parametrize("shape", CONFIDENCE_SHAPES)
def test_scene_confidence_against_the_exact_sums(shape):
    from gspn_amd.predict import scene_confidence
    from gspn_amd.rpointnet import nearest_in_sets
    b, r, n, p, c = shape
    pc, ep = PR.stage_inputs(*shape, seed=21, ladder=False, empty_row=True, full_row=True)
    if r >= 3:
        ep["detections"][0, r - 1, 6] = 0                                           # a row of class 0 for certain
    cls = class_ids_of(ep)
    idx = host_idx(pc, ep)
    assert bool((idx[:, 0] >= 0).all()) and (r == 1 or bool((idx[:, 1] == -1).all()))          # every point inside; no point inside
    sem_prob, point_fb = host_tables(pc, ep)
    masks = ep["rpointnet_mask_selected"]
    dev_idx = nearest_in_sets(pc.cuda(), ep["pc_coord_cropped_final_unnormalized"].cuda(), ep["detections"][:, :, :6].contiguous().cuda())
    assert torch.equal(dev_idx.cpu(), idx)
    args = (dev_idx, masks.cuda(), cls.cuda(), torch.from_numpy(sem_prob).cuda(), torch.from_numpy(point_fb).cuda())
    sem_conf, fb_conf, mask, points = scene_confidence(*args)
    assert sem_conf.dtype == fb_conf.dtype == torch.float64 and mask.dtype == torch.uint8 and points.dtype == torch.int32
    assert tuple(sem_conf.shape) == tuple(fb_conf.shape) == tuple(points.shape) == (b, r) and tuple(mask.shape) == (b, r, n)
    want_sem, want_fb, want_mask, want_points = PR.confidence_fsum(idx.numpy(), masks.numpy(), cls.numpy(), sem_prob, point_fb)
    got_sem, got_fb = sem_conf.cpu().numpy(), fb_conf.cpu().numpy()
    live = want_sem != 0
    print("scene_confidence %s: largest relative error sem %.3g fb %.3g, bound %.3g"
          % (shape, np.max(np.abs(got_sem - want_sem)[live] / want_sem[live], initial=0), np.max(np.abs(got_fb - want_fb)[live] / want_fb[live], initial=0),
             4.0 * n * 2.0 ** -53))
    assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(points.cpu().numpy(), want_points)
    assert PR.within_bound(got_sem, want_sem, n) and PR.within_bound(got_fb, want_fb, n)
    dead = cls.numpy() <= 0
    assert not got_sem[dead].any() and not got_fb[dead].any() and not mask.cpu().numpy()[dead].any() and not points.cpu().numpy()[dead].any()
    assert bits(got_sem[dead]) == bits(np.zeros(int(dead.sum()))) and (r < 3 or dead.any())
    if r > 1:                                                                       # the row with no inside point: 0 / 1e-8, exactly 0
        assert bool((cls[:, 1] > 0).all()) and not got_sem[:, 1].any() and not got_fb[:, 1].any() and not want_points[:, 1].any()
    assert bool((cls[:, 0] > 0).all()) and (got_sem[:, 0] > 0).all() and (n == 1 or (want_points[:, 0] > 0).all())          # one point: its value may be below 0.4
    again = scene_confidence(*args)
    for a, w in zip(again, (sem_conf, fb_conf, mask, points)):
        assert torch.equal(a, w)                                                    # a second call repeats the bits
    if r == 1:                                                                      # the only row as a dropped one
        zero = scene_confidence(args[0], args[1], torch.zeros_like(args[2]), args[3], args[4])
        assert not any(bool(t.any()) for t in zero)


def test_mask_threshold_is_a_double():
    """test.py:204 compares a float64 copy of the float32 mask value with the Python double 0.4: float32(0.4) = 0.4000000059... is above
    it.  With the constant rounded to float32 the first value would come out 0."""
    from gspn_amd.predict import scene_confidence
    at = np.float32(0.4)
    values = np.array([at, np.nextafter(at, np.float32(0)), np.nextafter(at, np.float32(1))], np.float32)
    assert float(values[0]) > 0.4 > float(values[1]) and not (values[0] > np.float32(0.4))
    idx = torch.tensor([[[0, 1, 2, -1]]], dtype=torch.int32)
    out = scene_confidence(idx.cuda(), torch.from_numpy(values).reshape(1, 1, 3).cuda(), torch.ones(1, 1, dtype=torch.int32).cuda(),
                           torch.full((1, 4, 2), 0.5).cuda(), torch.full((1, 4), 0.25).cuda(), 0.4)
    assert out[2].cpu().tolist() == [[[1, 0, 1, 0]]] and out[3].cpu().tolist() == [[2]]
    want = PR.confidence_fsum(idx.numpy(), values.reshape(1, 1, 3), np.ones((1, 1), np.int32), np.full((1, 4, 2), 0.5, np.float32),
                              np.full((1, 4), 0.25, np.float32))
    assert np.array_equal(out[2].cpu().numpy(), want[2])
    assert PR.within_bound(out[0].cpu().numpy(), want[0], 4) and PR.within_bound(out[1].cpu().numpy(), want[1], 4)


# ---- gspn_scene_rank ------------------------------------------------------------------------------------------------------------------------

def device_confidences(pc, ep):
    from gspn_amd.predict import scene_confidence
    from gspn_amd.rpointnet import nearest_in_sets
    sem_prob, point_fb = host_tables(pc, ep)
    idx = nearest_in_sets(pc.cuda(), ep["pc_coord_cropped_final_unnormalized"].cuda(), ep["detections"][:, :, :6].contiguous().cuda())
    sem_conf, fb_conf, _, _ = scene_confidence(idx, ep["rpointnet_mask_selected"].cuda(), class_ids_of(ep).cuda(), torch.from_numpy(sem_prob).cuda(),
                                               torch.from_numpy(point_fb).cuda())
    return sem_conf, fb_conf


def duplicate_row(ep, src, dst):
    for k in ("detections", "pc_coord_cropped_final_unnormalized", "rpointnet_mask_selected"):
        ep[k][:, dst] = ep[k][:, src]


def check_rank(ep, sem_conf, fb_conf, **th):
    from gspn_amd.predict import scene_rank
    det_score, cls = ep["detections"][:, :, 7].contiguous(), class_ids_of(ep)
    got = scene_rank(det_score.cuda(), cls.cuda(), sem_conf, fb_conf, **th)
    want = PR.rank(det_score.numpy(), cls.numpy(), sem_conf.cpu().numpy(), fb_conf.cpu().numpy(), *[th[k] for k in ("sem_conf_th", "fb_conf_th") if k in th])
    for g, w, dtype in zip(got, want, (torch.int32, torch.int32, torch.int32, torch.float32, torch.float64)):
        assert g.dtype == dtype and np.array_equal(g.cpu().numpy(), w)
    assert bits(got[4].cpu().numpy()) == bits(want[4])                              # the scores: equal bits
    return [g.cpu().numpy() for g in got]


@pytest.mark.parametrize("r", [1, 2, 65, 100, 1024])
def test_scene_rank_on_the_device_s_own_confidences(r):
    pc, ep = PR.stage_inputs(2, r, 300, 8, 19, seed=30 + r, ladder=False, empty_row=r > 2)
    if r == 2:
        ep["detections"][:, 0, 6] = 3
        duplicate_row(ep, 0, 1)
    if r > 2:
        ep["detections"][:, 2, 6] = 5
        duplicate_row(ep, 2, r - 1)                                                 # a tie between far rows
        duplicate_row(ep, 2, 3)                                                     # and between neighbours
    sem_conf, fb_conf = device_confidences(pc, ep)
    order, count, label_ids, confidence, score = check_rank(ep, sem_conf, fb_conf)
    assert all(sorted(order[i].tolist()) == list(range(r)) for i in range(2))
    if r >= 2:
        a, b = (0, 1) if r == 2 else (2, r - 1)
        for i in range(2):
            at = {int(row): k for k, row in enumerate(order[i])}
            assert score[i, at[a]] == score[i, at[b]] > 0 and at[a] < at[b]         # a real tie, the lower row first
            assert r == 2 or at[3] == at[2] + 1
    if r >= 65:
        assert set(np.unique(confidence).tolist()) == {0.0, float(np.float32(0.97)), 1.0}


def test_scene_rank_edge_scenes():
    r = 65
    pc, ep = PR.stage_inputs(2, r, 300, 8, 19, seed=77, ladder=False)
    ep["detections"][0, :, 6] = 0                                                   # a scene whose rows are all of class 0
    sem_conf, fb_conf = device_confidences(pc, ep)
    order, count, label_ids, confidence, score = check_rank(ep, sem_conf, fb_conf)
    assert count[0] == 0 and count[1] > 30 and order[0].tolist() == list(range(r))
    assert not label_ids[0].any() and not confidence[0].any() and not score[0].any()
    # thresholds no confidence reaches: every valid row is in the second group
    order, count, label_ids, confidence, score = check_rank(ep, sem_conf, fb_conf, sem_conf_th=2.0, fb_conf_th=0.01)
    assert (confidence[1, :count[1]] == np.float32(0.97)).all() and np.all(np.diff(score[1, :count[1]]) <= 0)
    # a confidence exactly equal to its threshold is not above it
    plain = check_rank(ep, sem_conf, fb_conf)
    first = int(plain[0][1, 0])                                                     # the best row of scene 1, of the first group
    assert plain[3][1, 0] == 1.0
    for th in (dict(sem_conf_th=float(sem_conf[1, first]), fb_conf_th=0.01), dict(sem_conf_th=0.01, fb_conf_th=float(fb_conf[1, first]))):
        order, count, label_ids, confidence, score = check_rank(ep, sem_conf, fb_conf, **th)
        at = order[1].tolist().index(first)
        assert confidence[1, at] == np.float32(0.97) and count[1] == plain[1][1]


def test_scene_rank_declines_more_than_1024_rows():
    from gspn_amd import _lib as L
    r = 1025
    det = torch.rand(1, r).cuda()
    cls = torch.ones(1, r, dtype=torch.int32).cuda()
    conf = torch.rand(1, r, dtype=torch.float64).cuda()
    label_map = torch.arange(19, dtype=torch.int32).cuda()
    outs = [torch.full((1, r), -7, dtype=torch.int32).cuda(), torch.full((1,), -7, dtype=torch.int32).cuda(),
            torch.full((1, r), -7, dtype=torch.int32).cuda(), torch.full((1, r), -7.0).cuda(), torch.full((1, r), -7.0, dtype=torch.float64).cuda()]
    rc = L.lib().gspn_scene_rank(1, r, 19, L.ptr(det), L.ptr(cls), L.ptr(conf), L.ptr(conf), ctypes.c_double(0.01), ctypes.c_double(0.01),
                                 L.ptr(label_map), *[L.ptr(t) for t in outs], L.stream())
    torch.cuda.synchronize()
    assert rc == -2                                                                 # GSPN_ERR_UNSUPPORTED
    assert all(bool((t == -7).all()) for t in outs)                                 # nothing was launched


# ---- scene_predictions end to end ------------------------------------------------------------------------------------------------------------

def read_tree(root):
    out = {}
    for base, _, files in os.walk(root):
        for name in files:
            with open(os.path.join(base, name), "rb") as f:
                out[os.path.relpath(os.path.join(base, name), root)] = f.read()
    return out


@pytest.mark.parametrize("shape,file_scenes", [((2, 100, 18000, 256, 19), (0,)), ((2, 7, 3001, 64, 19), (0, 1))])
def test_scene_predictions_against_the_literal_restatement(shape, file_scenes, tmp_path):
    from gspn_amd.inference import _point_probabilities
    from gspn_amd.predict import scene_predictions, write_predictions
    b, r, n, p, c = shape
    pc, ep = PR.stage_inputs(*shape, seed=41)
    dev_ep = cuda(ep)
    pred = scene_predictions(dev_ep, pc.cuda())
    assert set(pred) == {"order", "count", "label_ids", "confidence", "sem_conf", "fb_conf", "score", "masks", "mask_points"}
    got = {k: v.cpu().numpy() for k, v in pred.items()}
    assert got["masks"].dtype == np.uint8 and got["masks"].shape == (b, r, n) and got["count"].shape == (b,)
    # the device's own float32 tables (its softmax differs from numpy's by float32 steps), for the sums to double rounding
    table = _point_probabilities(pc.cuda(), dev_ep).cpu().numpy()
    host_sem, host_fb = host_tables(pc, ep)
    assert np.array_equal(table[:, :, 0], host_fb)                                  # the same nearest seed on both sides
    print("softmax, device against numpy: largest difference %.3g" % np.abs(table[:, :, 1:] - host_sem).max())
    cls = class_ids_of(ep).numpy()
    exact = PR.confidence_fsum(host_idx(pc, ep).numpy(), ep["rpointnet_mask_selected"].numpy(), cls, np.ascontiguousarray(table[:, :, 1:]),
                               np.ascontiguousarray(table[:, :, 0]))
    for i in range(b):
        lit = PR.output_prediction(pc[i].numpy(), ep["rpointnet_mask_selected"][i].numpy(), ep["pc_coord_cropped_final_unnormalized"][i].numpy(),
                                   ep["detections"][i].numpy(), ep["sem_class_logits"][i].numpy(), ep["pc_seed"][i].numpy(), ep["fb_prob"][i].numpy())
        nd = len(lit["rows"])
        assert got["count"][i] == nd > 0
        assert np.array_equal(got["order"][i, :nd], lit["rows"]) and np.array_equal(got["order"][i, nd:], np.where(cls[i] <= 0)[0])
        assert np.array_equal(got["label_ids"][i, :nd], lit["seg_label_pred"]) and not got["label_ids"][i, nd:].any()
        assert np.array_equal(got["confidence"][i, :nd], lit["confidence_pred"].astype(np.float32)) and not got["confidence"][i, nd:].any()
        assert set(lit["confidence_pred"].tolist()) == {1.0, 0.97}                  # both groups
        assert np.array_equal(got["masks"][i, :nd], lit["group_label_pred"]) and not got["masks"][i, nd:].any()
        at = got["order"][i]
        assert np.array_equal(got["mask_points"][i], got["masks"][i].sum(-1)) and got["mask_points"][i, at.tolist().index(1)] == 0      # the empty row
        written = int((got["mask_points"][i, :nd] > 0).sum())
        assert 0 < written < nd
        assert PR.within_bound(got["sem_conf"][i], exact[0][i][at], n) and PR.within_bound(got["fb_conf"][i], exact[1][i][at], n)
        assert np.array_equal(got["score"][i, :nd], ep["detections"][i].numpy()[at[:nd], 7].astype(np.float64) * got["sem_conf"][i, :nd] * got["fb_conf"][i, :nd])
        print("scene %d: %d predictions, confidences against the literal restatement (numpy's softmax): %.3g relative"
              % (i, nd, max((np.abs(got[k][i, :nd] - lit[k])[lit[k] > 0] / lit[k][lit[k] > 0]).max() for k in ("sem_conf", "fb_conf"))))
        if i in file_scenes:
            ours, theirs = str(tmp_path / ("ours%d" % i)), str(tmp_path / ("ref%d" % i))
            os.makedirs(ours)
            os.makedirs(theirs)
            assert write_predictions(ours, "scene%04d_00" % i, pred, i) == written  # an empty mask is skipped
            PR.export_instance_ids_for_eval_customized(os.path.join(theirs, "scene%04d_00.txt" % i), lit["seg_label_pred"], lit["group_label_pred"],
                                                       lit["confidence_pred"])
            a, w = read_tree(ours), read_tree(theirs)
            assert sorted(a) == sorted(w) and len(a) == written + 1 and all(a[k] == w[k] for k in w)
            second = bool(((lit["confidence_pred"] == 0.97) & (lit["group_label_pred"].sum(1) > 0)).any())      # a written row of the second group
            assert (b" 0.970000\n" in a["scene%04d_00.txt" % i]) == second and (second or r < 100) and b" 1.000000\n" in a["scene%04d_00.txt" % i]


# ---- behind rpointnet_inference ---------------------------------------------------------------------------------------------------------------

def by_hand(ep, pc, label_map):
    from gspn_amd.inference import _point_probabilities
    from gspn_amd.predict import scene_confidence, scene_rank
    from gspn_amd.rpointnet import nearest_in_sets
    det = ep["detections"]
    table = _point_probabilities(pc, ep)
    cls = det[:, :, 6].int()
    idx = nearest_in_sets(pc, ep["pc_coord_cropped_final_unnormalized"], det[:, :, :6])
    sem_conf, fb_conf, mask, points = scene_confidence(idx, ep["rpointnet_mask_selected"], cls, table[:, :, 1:].contiguous(), table[:, :, 0].contiguous(), 0.4)
    order, count, label_ids, confidence, score = scene_rank(det[:, :, 7], cls, sem_conf, fb_conf, 0.01, 0.01, label_map)
    at = order.long()
    rows = lambda t: torch.stack([t[i][at[i]] for i in range(t.shape[0])])
    return dict(order=order, count=count, label_ids=label_ids, confidence=confidence, score=score, sem_conf=rows(sem_conf), fb_conf=rows(fb_conf),
                masks=rows(mask), mask_points=rows(points)), mask


def test_stage_behind_rpointnet_inference():
    from gspn_amd.predict import SCANNET_LABEL_MAP, scene_predictions
    from gspn_amd.rpointnet import unmold_segmentation
    from tests import test_gpu_inference as TI
    run = TI.Run()
    keys = set(run.ep)
    label_map = SCANNET_LABEL_MAP[:TI.NCAT]
    pc = run.sc["pc"]
    pred = scene_predictions(run.ep, pc, label_map=label_map)
    assert set(run.ep) == keys                                                      # the stage adds no key to end_points
    shapes = dict(order=(TI.B, TI.D), count=(TI.B,), label_ids=(TI.B, TI.D), confidence=(TI.B, TI.D), sem_conf=(TI.B, TI.D), fb_conf=(TI.B, TI.D),
                  score=(TI.B, TI.D), masks=(TI.B, TI.D, TI.N), mask_points=(TI.B, TI.D))
    assert set(pred) == set(shapes)
    for k, shape in shapes.items():
        assert tuple(pred[k].shape) == shape and not pred[k].requires_grad, k
    want, mask = by_hand(run.ep, pc, label_map)
    for k, w in want.items():
        assert torch.equal(pred[k], w), k
    found = TI.detection_rows(run.ep["detections"])
    assert torch.equal(pred["count"].cpu(), found.int().cpu()) and bool((found >= 4).all())
    # the unpermuted masks are unmold_segmentation's tensor behind the threshold, which the stage never writes
    det = run.ep["detections"]
    unmolded = unmold_segmentation(torch.sigmoid(run.ep["rpointnet_mask"]), det[:, :, :6].contiguous(), det[:, :, 6], run.ep["pc_coord_cropped_final_unnormalized"], pc)
    assert torch.equal(mask, ((unmolded.double() > 0.4) & (det[:, :, 6] > 0).unsqueeze(-1)).to(torch.uint8))
    assert bool(pred["mask_points"].sum() > 0)


def test_stage_captured_behind_rpointnet_inference_and_replayed_on_new_inputs():
    from gspn_amd.graph import CapturedStep
    from gspn_amd.predict import SCANNET_LABEL_MAP, scene_predictions
    from gspn_amd.rpointnet import rpointnet_inference
    from gspn_amd.shape_proposal import valid_instances
    from gspn_amd.spn_trunks import spn_geometry
    from tests import test_gpu_inference as TI
    from tests import test_gpu_spn_net as TS
    from tests.test_gpu_modules import fresh_store
    sc, cfg = TS.scene(), TI.small_config()
    geo = spn_geometry(sc["pc"], cfg.NUM_SAMPLE, TS.SEM, True, points=sc["color"])
    valid = valid_instances(sc["group_indicator"])
    seed = torch.tensor([TI.SEED], dtype=torch.int64, device="cuda")
    label_map = SCANNET_LABEL_MAP[:TI.NCAT]
    fresh_store(TI.STORE_SEED)
    st, ep_of = {}, {}

    def step():
        ep_of["ep"] = rpointnet_inference(*TI.scene_args(sc), cfg, geometry=geo, valid_idx=valid, seed=seed)
        st["pred"] = scene_predictions(ep_of["ep"], sc["pc"], label_map=label_map)

    step()
    eager = TI.tensors(st["pred"])
    cap = CapturedStep(step)                                                        # the capture itself proves that nothing synchronises with the host
    cap.replay()
    torch.cuda.synchronize()
    for k, w in eager.items():
        assert torch.equal(st["pred"][k], w), k
    crops = ep_of["ep"]["pc_coord_cropped_final_unnormalized"].clone()
    seed.add_(1)                                                                    # other crops behind the same boxes
    cap.replay()
    torch.cuda.synchronize()
    bumped = TI.tensors(st["pred"])
    assert not torch.equal(ep_of["ep"]["pc_coord_cropped_final_unnormalized"], crops)
    step()                                                                          # eager, at the bumped seed
    for k, w in st["pred"].items():
        assert torch.equal(bumped[k], w), k
    # These freshly initialised heads give every crop point of a detection the same mask value, so other crops move no output of the
    # stage.  The stage alone, captured over persistent input buffers and replayed after another scene batch was copied into them:
    shape = (2, 7, 3001, 64, 19)
    first, second = (PR.stage_inputs(*shape, seed=s, ladder=False) for s in (51, 52))
    pc, ep = first[0].cuda(), cuda(first[1])
    cap = CapturedStep(lambda: st.update(alone=scene_predictions(ep, pc)))
    for inputs in (first, second, first):
        pc.copy_(inputs[0])
        for k, v in inputs[1].items():
            ep[k].copy_(v)
        cap.replay()
        torch.cuda.synchronize()
        replayed = TI.tensors(st["alone"])
        want = scene_predictions(cuda(inputs[1]), inputs[0].cuda())                 # eager, on fresh tensors
        for k, w in want.items():
            assert torch.equal(replayed[k], w), k
        if inputs is second:
            assert all(not torch.equal(replayed[k], before[k]) for k in ("order", "masks", "sem_conf", "fb_conf", "score", "mask_points"))
        before = replayed


# ---- gspn_sem_iou_counts ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [19, 2])
@pytest.mark.parametrize("rows", [1, 255, 256, 18000, 36001])
def test_semantic_iou_counts_against_the_loop(rows, c):
    from gspn_amd.predict import mean_iou, semantic_iou_counts
    rng = np.random.default_rng(rows + c)
    batches = []
    for _ in range(2):
        logits = np.round(1.5 * rng.standard_normal((rows, c)), 1).astype(np.float32)          # one decimal: equal maxima happen
        logits[::5, 0] = 9.0                                                        # two equal maxima, the first (class 0 here) wins
        logits[::5, c - 1] = 9.0
        logits[1::5, c - 1] = 9.0
        if c > 2:
            logits[2::5, 1] = 9.0
            logits[2::5, 2] = 9.0
        labels = rng.integers(0, c, rows).astype(np.int32)
        labels[::3] = 0
        batches.append((logits, labels))
    first = batches[0][0]
    assert ((first == first.max(-1, keepdims=True)).sum(-1) > 1).any() and (batches[0][1] == 0).any()
    want = PR.iou_counts(*batches[0], c)
    shape = (2, rows // 2) if rows == 18000 else (rows,)                             # a batch of scenes, as the drivers hold it
    dev = [(torch.from_numpy(l).reshape(shape + (c,)).cuda(), torch.from_numpy(t).reshape(shape).cuda()) for l, t in batches]
    inter, union = semantic_iou_counts(*dev[0])
    assert inter.dtype == union.dtype == torch.int64 and tuple(inter.shape) == tuple(union.shape) == (c - 1,)
    assert np.array_equal(inter.cpu().numpy(), want[0]) and np.array_equal(union.cpu().numpy(), want[1])
    assert want[1].sum() > 0 or rows == 1
    again = semantic_iou_counts(*dev[1], inter, union)                              # the second call adds into the same accumulators
    assert again[0] is inter and again[1] is union
    want = PR.iou_counts(*batches[1], c, want[0].copy(), want[1].copy())
    assert np.array_equal(inter.cpu().numpy(), want[0]) and np.array_equal(union.cpu().numpy(), want[1])
    assert PR.within_bound(np.float64(float(mean_iou(inter, union))), PR.mean_iou(want[0], want[1]), c - 1)
    assert float(mean_iou(inter, union)) == float(PR.mean_iou(want[0], want[1]))     # np.mean's order of adding: the same double
