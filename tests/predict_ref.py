"""Restatements, in numpy on the CPU, of the prediction export stage -- test.py:155-205 line for line (with tests/detect_ref.nearest_in_sets
in place of the ball tree per detection), its exporters (:96-114, :128-129, and ScanNet's util_3d.export_ids as one '%d' per line), the
IoU loop of train.py:365-368, 385-386 -- written from the reference's text for the tests of gspn_amd/predict.py, with
  * an exact variant of the three sums (math.fsum over the points inside each box: every term is a float32 or a product of two, exact in
    double, so fsum returns the correctly rounded sum),
  * the ordering of :191-205 as a function of given confidences, with the device's tie rule (the lower row first),
  * a generator of synthetic stage inputs whose scores lie on a ladder, so that the literal restatement (which leaves equal scores where
    np.argsort(...)[::-1] happens to) and the device agree on the order for a reason."""
import math
import os

import numpy as np
import torch

from tests import detect_ref as DR

SEG_LABEL_MAP = np.array([0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])          # test.py:121, :136


# ---- the point tables (:175-177, :182-187) ---------------------------------------------------------------------------------------------

def point_tables(pc, sem_class_logits, pc_seed, fb_prob):
    """one scene.  pc (N, 3), sem_class_logits (N, NC), pc_seed (NS, 3), fb_prob (NS, 2) float32 numpy -> sem_class_prob (N, NC) float32,
    fb (N,) float32.  The nearest seed is detect_ref's first minimum of the float32 distance instead of the ball tree's"""
    sem_class_prob = np.exp(sem_class_logits)                                                            # :176
    sem_class_prob = np.divide(sem_class_prob, np.sum(sem_class_prob, -1, keepdims=True))                # :177
    sidx = DR.nearest_in_sets(torch.from_numpy(pc)[None], torch.from_numpy(pc_seed)[None, None])[0, 0].numpy()
    return sem_class_prob, fb_prob[sidx, 1]                                                              # :187


# ---- test.py:155-205 for one scene -----------------------------------------------------------------------------------------------------

def output_prediction(batch_pc, rpointnet_mask_selected, pc_coord_cropped_final_unnormalized, detections, sem_class_logits, pc_seed, fb_prob,
                      sem_conf_th=0.01, fb_conf_th=0.01, mask_th=0.4, seg_label_map=SEG_LABEL_MAP, tables=None):
    """the body of output_prediction's loop behind sess.run, on float32 numpy arrays of one scene.  tables: (sem_class_prob (N, NC),
    fb (N,)) to use in place of :175-187 (the tests pass the device's own float32 tables where they check the sums to double rounding:
    a float32 softmax differs by float32 steps between the host and the device).  -> a dict: rows (the original row of each output
    row), seg_label_pred, group_label_pred (ND, N) int32, confidence_pred, sem_conf, fb_conf, score"""
    rows = np.where(detections[:, 6] > 0)[0]
    rpointnet_mask_selected = rpointnet_mask_selected[detections[:, 6] > 0, :]                          # :159
    pc_coord_cropped_final_unnormalized = pc_coord_cropped_final_unnormalized[detections[:, 6] > 0, :, :]
    detections = detections[detections[:, 6] > 0, :]                                                    # :161

    group_label_pred = np.zeros((detections.shape[0], batch_pc.shape[0]))                               # :163, float64
    if detections.shape[0]:
        near = DR.nearest_in_sets(torch.from_numpy(batch_pc)[None], torch.from_numpy(pc_coord_cropped_final_unnormalized)[None],
                                  torch.from_numpy(np.ascontiguousarray(detections[:, :6]))[None])[0].numpy()
    for j in range(detections.shape[0]):
        sidx = near[j]                                                                                  # :165-167 (-1 outside the box: not searched)
        roi_mask = np.logical_and(batch_pc >= np.reshape(detections[j, :3] - detections[j, 3:6] / 2, [1, 3]),
                                  batch_pc <= np.reshape(detections[j, :3] + detections[j, 3:6] / 2, [1, 3]))
        roi_mask = np.logical_and(np.logical_and(roi_mask[:, 0], roi_mask[:, 1]), roi_mask[:, 2])
        assert np.array_equal(roi_mask, sidx >= 0)                                                      # the box test of both is the same
        group_label_pred[j, :] = rpointnet_mask_selected[j, np.maximum(sidx, 0)]                        # :168
        roi_mask = roi_mask.astype(np.float32)
        group_label_pred[j, :] = np.multiply(group_label_pred[j, :], roi_mask)                          # :173
    if tables is None:
        sem_class_prob, fb = point_tables(batch_pc, sem_class_logits, pc_seed, fb_prob)
    else:
        sem_class_prob, fb = tables
    sem_conf = np.matmul(group_label_pred, sem_class_prob)                                              # :178
    sem_conf = np.divide(sem_conf, 1e-8 + np.sum(group_label_pred, 1, keepdims=True))                   # :179
    sem_conf = sem_conf.reshape(-1)[detections[:, 6].astype(np.int32) + np.arange(detections.shape[0]) * sem_conf.shape[1]]
    fb_conf = np.matmul(group_label_pred, fb)                                                           # :188
    fb_conf = np.divide(fb_conf, 1e-8 + np.sum(group_label_pred, 1))                                    # :189

    sidx = np.where(np.logical_and(sem_conf > sem_conf_th, fb_conf > fb_conf_th))[0]                    # :192
    sidx2 = np.where(np.logical_or(sem_conf <= sem_conf_th, fb_conf <= fb_conf_th))[0]
    sidx_idx = np.argsort(detections[sidx, 7] * sem_conf[sidx] * fb_conf[sidx])[::-1]
    sidx = sidx[sidx_idx]
    sidx2_idx = np.argsort(detections[sidx2, 7] * sem_conf[sidx2] * fb_conf[sidx2])[::-1]
    sidx2 = sidx2[sidx2_idx]
    score = detections[:, 7] * sem_conf * fb_conf
    order = np.concatenate((sidx, sidx2), 0)
    group_label_pred = np.concatenate((group_label_pred[sidx, :], group_label_pred[sidx2, :]), 0)
    detections = np.concatenate((detections[sidx, :], detections[sidx2, :]), 0)
    sem_conf = np.concatenate((sem_conf[sidx], sem_conf[sidx2]), 0)
    fb_conf = np.concatenate((fb_conf[sidx], fb_conf[sidx2]), 0)
    confidence_pred = np.concatenate((np.ones(len(sidx)), 0.97 * np.ones(len(sidx2))), 0)               # :202

    group_label_pred = (group_label_pred > mask_th).astype(np.int32)                                    # :204
    seg_label_pred = seg_label_map[(detections[:, 6]).astype(np.int32)]                                 # :205
    return dict(rows=rows[order], seg_label_pred=seg_label_pred, group_label_pred=group_label_pred, confidence_pred=confidence_pred,
                sem_conf=sem_conf, fb_conf=fb_conf, score=score[order])


# ---- the exporters (:96-114, :128-129) -------------------------------------------------------------------------------------------------

def export_ids(filename, ids):
    """ScanNet BenchmarkScripts util_3d.export_ids: one integer per line"""
    with open(filename, 'w') as f:
        for id in ids:
            f.write('%d\n' % id)


def export_instance_ids_for_eval_customized(filename, label_ids, instance_ids, confidence):
    assert label_ids.shape[0] == instance_ids.shape[0]
    output_mask_path_relative = 'pred_mask'
    name = os.path.splitext(os.path.basename(filename))[0]
    output_mask_path = os.path.join(os.path.dirname(filename), output_mask_path_relative)
    if not os.path.isdir(output_mask_path):
        os.mkdir(output_mask_path)
    with open(filename, 'w') as f:
        for idx in np.arange(instance_ids.shape[0]):
            if np.sum(instance_ids[idx]) == 0:
                continue
            output_mask_file_relative = os.path.join(output_mask_path_relative, name + '_' + str(idx) + '.txt')
            f.write('%s %d %f\n' % (output_mask_file_relative, label_ids[idx], confidence[idx]))
            output_mask_file = os.path.join(output_mask_path, name + '_' + str(idx) + '.txt')
            export_ids(output_mask_file, instance_ids[idx])


def gen_gt(output_path, scan, batch_seg_label, batch_group_label, seg_label_map=SEG_LABEL_MAP):
    if not os.path.exists(output_path):
        os.makedirs(output_path)
    batch_seg_label = seg_label_map[batch_seg_label]                                                    # :128
    export_ids(os.path.join(output_path, scan + '.txt'), batch_seg_label * 1000 + batch_group_label)    # :129


# ---- the exact sums ---------------------------------------------------------------------------------------------------------------------

def confidence_fsum(idx, masks, class_ids, sem_prob, point_fb, mask_th=0.4):
    """idx (B, R, N) int32, masks (B, R, P), class_ids (B, R), sem_prob (B, N, C), point_fb (B, N) numpy float32 -> sem_conf, fb_conf
    (B, R) float64 from correctly rounded sums, mask (B, R, N) uint8, mask_points (B, R) int32; zeros in the rows of class <= 0"""
    b, r, n = idx.shape
    sem_conf, fb_conf = np.zeros((b, r)), np.zeros((b, r))
    mask, points = np.zeros((b, r, n), np.uint8), np.zeros((b, r), np.int32)
    for i in range(b):
        for k in range(r):
            cls = int(class_ids[i, k])
            if cls <= 0:
                continue
            inside = np.nonzero(idx[i, k] >= 0)[0]
            g = masks[i, k][idx[i, k][inside]].astype(np.float64)
            assert masks.dtype == np.float32 and sem_prob.dtype == np.float32 and point_fb.dtype == np.float32
            s0 = math.fsum(g.tolist())
            s1 = math.fsum((g * sem_prob[i, inside, cls].astype(np.float64)).tolist())                  # 24 x 24 bits: exact products
            s2 = math.fsum((g * point_fb[i, inside].astype(np.float64)).tolist())
            sem_conf[i, k] = s1 / (1e-8 + s0)
            fb_conf[i, k] = s2 / (1e-8 + s0)
            full = np.zeros(n)
            full[inside] = g
            mask[i, k] = full > mask_th
            points[i, k] = mask[i, k].sum()
    return sem_conf, fb_conf, mask, points


def within_bound(got, want, n):
    """|got - want| <= 4 n 2^-53 |want|: the terms are exact and non-negative, so any two orders of adding n of them differ by less than
    n 2^-53 relative; the quotient and 1e-8 + S0 add a rounding each.  A bound, not a measurement."""
    return bool(np.all(np.abs(got - want) <= 4.0 * n * 2.0 ** -53 * np.abs(want)))


# ---- the ordering (:191-205) from given confidences ------------------------------------------------------------------------------------

def rank(det_score, class_ids, sem_conf, fb_conf, sem_conf_th=0.01, fb_conf_th=0.01, seg_label_map=SEG_LABEL_MAP):
    """det_score (B, R) float32, class_ids (B, R) int, sem_conf, fb_conf (B, R) float64 -> order, count, label_ids, confidence, score with
    the device's shapes and dtypes.  :192-202 with a stable sort of the negated scores (equal scores: the lower row first, where the
    reference's argsort(...)[::-1] leaves them in an order of its own), then the dropped rows (:159-161) in ascending order with zeros."""
    b, r = det_score.shape
    order, count = np.zeros((b, r), np.int32), np.zeros((b,), np.int32)
    label_ids, confidence, score = np.zeros((b, r), np.int32), np.zeros((b, r), np.float32), np.zeros((b, r))
    for i in range(b):
        rows = np.where(class_ids[i] > 0)[0]
        sc, fc = sem_conf[i][rows], fb_conf[i][rows]
        s = det_score[i][rows].astype(np.float64) * sc * fc                                             # :194, left to right
        sidx = np.where(np.logical_and(sc > sem_conf_th, fc > fb_conf_th))[0]
        sidx2 = np.where(np.logical_or(sc <= sem_conf_th, fc <= fb_conf_th))[0]
        sidx = sidx[np.argsort(-s[sidx], kind='stable')]
        sidx2 = sidx2[np.argsort(-s[sidx2], kind='stable')]
        both = np.concatenate((sidx, sidx2), 0)
        nd = len(both)
        assert nd == len(rows)
        order[i] = np.concatenate((rows[both], np.where(class_ids[i] <= 0)[0]), 0)
        count[i] = nd
        label_ids[i, :nd] = np.asarray(seg_label_map)[class_ids[i][rows[both]]]
        confidence[i, :nd] = np.concatenate((np.ones(len(sidx)), 0.97 * np.ones(len(sidx2))), 0)
        score[i, :nd] = s[both]
    return order, count, label_ids, confidence, score


# ---- train.py:365-368, 385-386 ---------------------------------------------------------------------------------------------------------

def iou_counts(pred_val, sem_labels_val, num_category, cum_intersection=None, cum_union=None):
    """pred_val (..., NC) logits, sem_labels_val (...) -> the two accumulators (NC - 1,) int64 (the reference's are float64 and hold
    whole numbers)"""
    if cum_intersection is None:
        cum_intersection, cum_union = np.zeros(num_category - 1, np.int64), np.zeros(num_category - 1, np.int64)
    pred_val = np.argmax(pred_val, -1)                                                                  # :365
    for s in range(num_category - 1):
        cum_intersection[s] += np.sum(np.logical_and(pred_val == (s + 1), sem_labels_val == (s + 1)))
        cum_union[s] += np.sum(np.logical_or(pred_val == (s + 1), sem_labels_val == (s + 1)))
    return cum_intersection, cum_union


def mean_iou(cum_intersection, cum_union):
    iou = np.divide(cum_intersection, cum_union + 1e-8)                                                 # :385
    return np.mean(iou)


# ---- synthetic stage inputs ---------------------------------------------------------------------------------------------------------------

LADDER = 0.97          # the ratio of neighbouring scores of a scene


def stage_inputs(b, r, n, p, c, seed, nseed=64, ladder=True, empty_row=True, full_row=False):
    """What rpointnet_inference hands to the stage, synthetic: pc (b, n, 3) uniform in the unit cube, and end_points with
      detections (b, r, 8): boxes of 0.25..0.55 per side around cloud points, a class in [0, c) -- 0 in about one row in five, the last
                            three classes (for c > 4) are rare in the logits, so their rows fall below the semantic threshold --, scores
      pc_coord_cropped_final_unnormalized (b, r, p, 3): drawn with replacement from the points inside the box (from the cloud if none)
      rpointnet_mask_selected (b, r, p): sigmoid(2.5 * randn)
      sem_class_logits (b, n, c), pc_seed (b, nseed, 3): cloud points, fb_prob (b, nseed, 2)
    empty_row: row 1 (if r > 1) of every scene has a valid class and a box that holds no point (both confidences 0, an empty mask);
    full_row: row 0 of every scene has a valid class and a box around the whole cloud.
    ladder: the scores (column 7) are chosen so that the products score * sem_conf * fb_conf of a scene's valid rows (computed here from
    the exact sums) lie on a ladder of ratio 0.97 in a shuffled order, and it is asserted that any two of them differ by more than 1e-6
    relative and that no confidence is within 1e-6 of 0.01: a float32 softmax on the device moves a confidence by float32 steps (1e-7),
    which then changes neither the order nor a group.  ladder=False: random scores (for tests that feed the ordering given values).
    -> pc, end_points (torch CPU tensors)"""
    rng = np.random.default_rng(seed)
    pc = rng.random((b, n, 3), dtype=np.float32)
    det = np.zeros((b, r, 8), np.float32)
    crops = np.zeros((b, r, p, 3), np.float32)
    cls = rng.integers(1, c, (b, r))
    cls[rng.random((b, r)) < 0.2] = 0
    for i in range(b):
        for k in range(r):
            det[i, k, :3] = pc[i, rng.integers(n)]
            det[i, k, 3:6] = 0.25 + 0.3 * rng.random(3, dtype=np.float32)
            if full_row and k == 0:
                det[i, k, :6] = (0.5, 0.5, 0.5, 2, 2, 2)
                cls[i, k] = max(cls[i, k], 1)
            if empty_row and k == 1:
                det[i, k, :6] = (3, 3, 3, 0.5, 0.5, 0.5)
                cls[i, k] = max(cls[i, k], 1)
            lo, hi = det[i, k, :3] - det[i, k, 3:6] / 2, det[i, k, :3] + det[i, k, 3:6] / 2
            inside = np.nonzero(np.all((pc[i] >= lo) & (pc[i] <= hi), -1))[0]
            pool = inside if len(inside) else np.arange(n)
            crops[i, k] = pc[i, pool[rng.integers(len(pool), size=p)]]
    det[:, :, 6] = cls
    det[:, :, 7] = 0.05 + 0.95 * rng.random((b, r), dtype=np.float32)
    masks = (1.0 / (1.0 + np.exp(-2.5 * rng.standard_normal((b, r, p))))).astype(np.float32)
    logits = (2.0 * rng.standard_normal((b, n, c))).astype(np.float32)
    if c > 4:
        logits[:, :, c - 3:] -= 6.0
    pc_seed = np.stack([pc[i, rng.choice(n, size=min(nseed, n), replace=False)] for i in range(b)])
    fb1 = (0.05 + 0.9 * rng.random((b, pc_seed.shape[1]))).astype(np.float32)
    fb_prob = np.stack((1 - fb1, fb1), -1).astype(np.float32)
    if ladder:
        for i in range(b):
            rows = np.nonzero(cls[i] > 0)[0]
            idx = DR.nearest_in_sets(torch.from_numpy(pc[i:i + 1]), torch.from_numpy(crops[i:i + 1]), torch.from_numpy(det[i:i + 1, :, :6])).numpy()
            sem_prob, fb = point_tables(pc[i], logits[i], pc_seed[i], fb_prob[i])
            sc, fc, _, _ = confidence_fsum(idx, masks[i:i + 1], cls[i:i + 1], sem_prob[None], fb[None])
            conf = (sc * fc)[0][rows]
            step = rng.permutation(len(rows))
            live = conf > 0
            det[i, rows[live], 7] = (0.9 * LADDER ** step[live] / conf[live]).astype(np.float32)
            score = det[i, rows, 7].astype(np.float64) * sc[0][rows] * fc[0][rows]
            assert (~live).sum() <= 1                                                                   # at most one score of 0
            top = np.sort(score)[::-1]
            assert np.all(top[:-1] - top[1:] > 1e-6 * top[:-1]), "scores are not separated"
            for v in (sc[0][rows], fc[0][rows]):
                assert np.all(np.abs(v - 0.01) > 1e-6), "a confidence is too close to its threshold"
    end_points = dict(detections=torch.from_numpy(det), pc_coord_cropped_final_unnormalized=torch.from_numpy(crops),
                      rpointnet_mask_selected=torch.from_numpy(masks), sem_class_logits=torch.from_numpy(logits),
                      pc_seed=torch.from_numpy(pc_seed), fb_prob=torch.from_numpy(fb_prob))
    return torch.from_numpy(pc), end_points
