"""The prediction export stage: what test.py:155-206 computes from the outputs of rpointnet_inference -- per-scene instance masks on the
scene's points, each with a label id and a confidence, in the files the ScanNet instance benchmark reads -- and the semantic IoU counts of
train.py:365-368, 385-386, on the HIP kernels of csrc/predict.hip.

The reference works on the host, one detection at a time: a ball tree per detection (:165), a (ND, N) float64 matrix of mask values, its
product with the (N, NC) softmax table (:178) and two argsorts (:194-197).  Here nearest_in_sets (csrc/detect.hip) searches all detections
in one launch, gspn_scene_confidence reads its indices and writes the two confidences, the thresholded masks and their sizes without the
float matrix, and gspn_scene_rank puts the rows into the reference's two-group order by counting.  Rows of equal score come out with the
lower row first (the reference leaves them where np.argsort(...)[::-1] happens to: DESIGN.md 2).

scene_predictions runs under torch.no_grad(); every shape is static and nothing reads a value back to the host, so it captures in a
graph.CapturedStep behind rpointnet_inference.  write_predictions and write_ground_truth are the host IO: plain Python once the tensors
are on the CPU.  No CPU fallback for the compute."""
import os

import torch

from . import _lib as L
from ._args import _on_device, _typed
from .detect import nearest_in_sets
from .inference import _point_probabilities

__all__ = ["SCANNET_LABEL_MAP", "SCENE_RANK_MAX_R", "SEM_IOU_MAX_C", "scene_confidence", "scene_rank", "scene_predictions",
           "semantic_iou_counts", "mean_iou", "write_predictions", "write_ground_truth"]

SCANNET_LABEL_MAP = (0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)          # test.py:121: class -> ScanNet label id
SCENE_RANK_MAX_R = 1024       # GSPN_SCENE_RANK_MAX_R of include/gspn_hip.h: the keys of one scene's rows sit in LDS
SEM_IOU_MAX_C = 256           # GSPN_SEM_IOU_MAX_C: the per-workgroup counters

_label_maps = {}


def _label_map(values, device):
    """the label map as an int32 device tensor, copied there once (a host-to-device copy has no place inside a captured step)"""
    key = (tuple(int(v) for v in values), device)
    if key not in _label_maps:
        _label_maps[key] = torch.tensor(key[0], dtype=torch.int32, device=device)
    return _label_maps[key]


def scene_confidence(idx, masks, class_ids, sem_prob, point_fb, mask_th=0.4):
    """test.py:163-189 and :204 for all detections at once.  idx (B, R, N) int32: nearest_in_sets(pc, crops, boxes), -1 outside the box;
    masks (B, R, P) float32; class_ids (B, R) int32; sem_prob (B, N, C), point_fb (B, N) float32; mask_th a Python float (a double)
    -> sem_conf, fb_conf (B, R) float64, mask (B, R, N) uint8, mask_points (B, R) int32.  With g = the mask value at each point's nearest
    crop point inside the box and 0 outside: sem_conf = sum(g * sem_prob[:, class]) / (1e-8 + sum(g)), fb_conf the same with point_fb,
    every term exact in double, added in an order that depends on the shape alone (the same bits on every call); mask = float64(g) >
    mask_th.  A row whose class is outside [1, C) gets zeros everywhere."""
    idx = _typed(idx, torch.int32, 3, "idx")
    masks = _typed(masks, torch.float32, 3, "masks")
    class_ids = _typed(class_ids, torch.int32, 2, "class_ids")
    sem_prob = _typed(sem_prob, torch.float32, 3, "sem_prob")
    point_fb = _typed(point_fb, torch.float32, 2, "point_fb")
    b, r, n = idx.shape
    p, c = masks.shape[2], sem_prob.shape[2]
    if tuple(masks.shape[:2]) != (b, r) or tuple(class_ids.shape) != (b, r) or tuple(sem_prob.shape[:2]) != (b, n) or tuple(point_fb.shape) != (b, n):
        raise ValueError("scene_confidence: expected idx (B, R, N), masks (B, R, P), class_ids (B, R), sem_prob (B, N, C) and point_fb (B, N), "
                         "got %s, %s, %s, %s and %s" % (tuple(idx.shape), tuple(masks.shape), tuple(class_ids.shape), tuple(sem_prob.shape),
                                                        tuple(point_fb.shape)))
    if min(b, r, n, p, c) <= 0:
        raise ValueError("scene_confidence: empty input, idx %s, masks %s, sem_prob %s" % (tuple(idx.shape), tuple(masks.shape), tuple(sem_prob.shape)))
    mask_th = float(mask_th)
    if mask_th != mask_th:
        raise ValueError("scene_confidence: mask_th is NaN")
    idx, masks, class_ids, sem_prob, point_fb = _on_device(idx=idx, masks=masks, class_ids=class_ids, sem_prob=sem_prob, point_fb=point_fb)
    dev = idx.device
    sem_conf = torch.empty((b, r), dtype=torch.float64, device=dev)
    fb_conf = torch.empty((b, r), dtype=torch.float64, device=dev)
    mask = torch.empty((b, r, n), dtype=torch.uint8, device=dev)
    mask_points = torch.empty((b, r), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_scene_confidence(b, r, n, p, c, L.ptr(idx), L.ptr(masks), L.ptr(class_ids), L.ptr(sem_prob), L.ptr(point_fb), mask_th,
                                              L.ptr(sem_conf), L.ptr(fb_conf), L.ptr(mask), L.ptr(mask_points), L.stream()), "scene_confidence")
    return sem_conf, fb_conf, mask, mask_points


def scene_rank(det_score, class_ids, sem_conf, fb_conf, sem_conf_th=0.01, fb_conf_th=0.01, label_map=SCANNET_LABEL_MAP):
    """test.py:159-161 and :191-205.  det_score (B, R) float32, class_ids (B, R) int32, sem_conf, fb_conf (B, R) float64, label_map: C
    integers (a sequence, or an int32 device tensor) -> order (B, R) int32, count (B,) int32, label_ids (B, R) int32, confidence (B, R)
    float32, score (B, R) float64.  score = (float64(det_score) * sem_conf) * fb_conf.  Group 0: class in [1, C) with sem_conf >
    sem_conf_th and fb_conf > fb_conf_th; group 1: the other rows of such a class; group 2: the rows the reference drops (score 0).
    order[k] is the row at output position k: by group, then by descending score, then by ascending row; count = the rows of groups 0
    and 1; label_ids = label_map[class] (0 in group 2), confidence = 1, 0.97, 0 by group, score: all three in output order.
    Raises NotImplementedError for R > 1024, before anything has run."""
    det_score = _typed(det_score, torch.float32, 2, "det_score")
    class_ids = _typed(class_ids, torch.int32, 2, "class_ids")
    sem_conf = _typed(sem_conf, torch.float64, 2, "sem_conf")
    fb_conf = _typed(fb_conf, torch.float64, 2, "fb_conf")
    b, r = det_score.shape
    if not (tuple(class_ids.shape) == tuple(sem_conf.shape) == tuple(fb_conf.shape) == (b, r)):
        raise ValueError("scene_rank: det_score, class_ids, sem_conf and fb_conf must share (B, R), got %s, %s, %s and %s"
                         % (tuple(det_score.shape), tuple(class_ids.shape), tuple(sem_conf.shape), tuple(fb_conf.shape)))
    if min(b, r) <= 0:
        raise ValueError("scene_rank: empty input %s" % (tuple(det_score.shape),))
    if isinstance(label_map, torch.Tensor):
        label_map = _typed(label_map, torch.int32, 1, "label_map")
    c = len(label_map)
    if c <= 0:
        raise ValueError("scene_rank: empty label_map")
    sem_conf_th, fb_conf_th = float(sem_conf_th), float(fb_conf_th)
    if sem_conf_th != sem_conf_th or fb_conf_th != fb_conf_th:
        raise ValueError("scene_rank: a threshold is NaN")
    if r > SCENE_RANK_MAX_R:
        raise NotImplementedError("scene_rank: R <= %d (got %d)" % (SCENE_RANK_MAX_R, r))
    det_score, class_ids, sem_conf, fb_conf = _on_device(det_score=det_score, class_ids=class_ids, sem_conf=sem_conf, fb_conf=fb_conf)
    label_map = _on_device(label_map=label_map)[0] if isinstance(label_map, torch.Tensor) else _label_map(label_map, det_score.device)
    dev = det_score.device
    order = torch.empty((b, r), dtype=torch.int32, device=dev)
    count = torch.empty((b,), dtype=torch.int32, device=dev)
    label_ids = torch.empty((b, r), dtype=torch.int32, device=dev)
    confidence = torch.empty((b, r), dtype=torch.float32, device=dev)
    score = torch.empty((b, r), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_scene_rank(b, r, c, L.ptr(det_score), L.ptr(class_ids), L.ptr(sem_conf), L.ptr(fb_conf), sem_conf_th, fb_conf_th,
                                        L.ptr(label_map), L.ptr(order), L.ptr(count), L.ptr(label_ids), L.ptr(confidence), L.ptr(score),
                                        L.stream()), "scene_rank")
    return order, count, label_ids, confidence, score


_KEYS = ("detections", "rpointnet_mask_selected", "pc_coord_cropped_final_unnormalized", "pc_seed", "fb_prob", "sem_class_logits")


def scene_predictions(end_points, pc, *, sem_conf_th=0.01, fb_conf_th=0.01, mask_th=0.4, label_map=SCANNET_LABEL_MAP, mask_nms_th=None):
    """test.py:155-205 for the whole batch.  end_points: rpointnet_inference's, as they are (read: detections (B, R, 8),
    rpointnet_mask_selected (B, R, P), pc_coord_cropped_final_unnormalized (B, R, P, 3), pc_seed, fb_prob, sem_class_logits (B, N, C));
    pc (B, N, 3); label_map: C integers.  -> a dict, every per-detection entry in output order (scene_rank's):
      order (B, R) int32, count (B,) int32: the first count rows of a scene are its predictions, the rest are the rows the reference drops
      label_ids (B, R) int32, confidence (B, R) float32, sem_conf, fb_conf, score (B, R) float64
      masks (B, R, N) uint8 (0 or 1), mask_points (B, R) int32: the set bytes of each mask
    The point tables come from inference._point_probabilities, the nearest crop points from nearest_in_sets behind the detection boxes.
    mask_nms_th: a float in [0, 1), or None.  Then mask_nms.mask_nms at that IoU runs on the rows in output order with
    count and label_ids as they are: a row that an earlier kept row of its label overlaps above the threshold comes out all zero with
    mask_points 0, and the dict gains 'keep' (B, R) uint8; nothing else changes.  With None the keys and bits are what they were.
    Raises ValueError on a missing key or a shape or dtype that does not fit, NotImplementedError for R > 1024, before anything runs."""
    for k in _KEYS:
        if k not in end_points:
            raise ValueError("scene_predictions: end_points has no %r (pass rpointnet_inference's end_points)" % k)
    pc = _typed(pc, torch.float32, 3, "pc")
    detections = _typed(end_points["detections"], torch.float32, 3, "detections")
    masks = _typed(end_points["rpointnet_mask_selected"], torch.float32, 3, "rpointnet_mask_selected")
    crops = _typed(end_points["pc_coord_cropped_final_unnormalized"], torch.float32, 4, "pc_coord_cropped_final_unnormalized")
    logits = _typed(end_points["sem_class_logits"], torch.float32, 3, "sem_class_logits")
    pc_seed = _typed(end_points["pc_seed"], torch.float32, 3, "pc_seed")
    fb_prob = _typed(end_points["fb_prob"], torch.float32, 3, "fb_prob")
    b, n, _ = pc.shape
    r, p = masks.shape[1:]
    c = logits.shape[2]
    if (pc.shape[2] != 3 or tuple(detections.shape) != (b, r, 8) or masks.shape[0] != b or tuple(crops.shape) != (b, r, p, 3)
            or tuple(logits.shape[:2]) != (b, n) or pc_seed.shape[0] != b or pc_seed.shape[2] != 3
            or tuple(fb_prob.shape) != (b, pc_seed.shape[1], 2)):
        raise ValueError("scene_predictions: expected pc (B, N, 3), detections (B, R, 8), rpointnet_mask_selected (B, R, P), "
                         "pc_coord_cropped_final_unnormalized (B, R, P, 3), sem_class_logits (B, N, C), pc_seed (B, S, 3) and fb_prob (B, S, 2), "
                         "got %s, %s, %s, %s, %s, %s and %s" % tuple(tuple(t.shape) for t in (pc, detections, masks, crops, logits, pc_seed, fb_prob)))
    if min(b, n, r, p, c) <= 0:
        raise ValueError("scene_predictions: empty input, pc %s, rpointnet_mask_selected %s" % (tuple(pc.shape), tuple(masks.shape)))
    if isinstance(label_map, torch.Tensor):
        label_map = _typed(label_map, torch.int32, 1, "label_map")
    if len(label_map) != c:
        raise ValueError("scene_predictions: label_map must have one entry per class, %d, got %d" % (c, len(label_map)))
    if mask_nms_th is not None:
        mask_nms_th = float(mask_nms_th)
        if not 0.0 <= mask_nms_th < 1.0:
            raise ValueError("scene_predictions: mask_nms_th must lie in [0, 1), got %r" % mask_nms_th)
    if r > SCENE_RANK_MAX_R:
        raise NotImplementedError("scene_predictions: R <= %d (got %d)" % (SCENE_RANK_MAX_R, r))
    pc, detections, masks, crops, logits, pc_seed, fb_prob = _on_device(
        pc=pc, detections=detections, rpointnet_mask_selected=masks, pc_coord_cropped_final_unnormalized=crops, sem_class_logits=logits,
        pc_seed=pc_seed, fb_prob=fb_prob)
    with torch.no_grad():
        table = _point_probabilities(pc, {"pc_seed": pc_seed, "fb_prob": fb_prob, "sem_class_logits": logits})      # (B, N, 1 + C)
        point_fb = table[:, :, 0].contiguous()
        sem_prob = table[:, :, 1:].contiguous()
        class_ids = detections[:, :, 6].int()                                                           # :180, .astype(np.int32)
        idx = nearest_in_sets(pc, crops, detections[:, :, :6])
        sem_conf, fb_conf, mask, mask_points = scene_confidence(idx, masks, class_ids, sem_prob, point_fb, mask_th)
        order, count, label_ids, confidence, score = scene_rank(detections[:, :, 7], class_ids, sem_conf, fb_conf, sem_conf_th, fb_conf_th,
                                                                label_map)
        at = order.long()
        pred = {
            "order": order, "count": count, "label_ids": label_ids, "confidence": confidence,
            "sem_conf": torch.gather(sem_conf, 1, at), "fb_conf": torch.gather(fb_conf, 1, at), "score": score,
            "masks": torch.gather(mask, 1, at.unsqueeze(-1).expand(b, r, n)), "mask_points": torch.gather(mask_points, 1, at),
        }
        if mask_nms_th is not None:                                                                     # 4.24: in place, on the rows in output order
            from .mask_nms import mask_nms                  # (mask_nms imports this module's helpers)
            pred["masks"], pred["keep"], pred["mask_points"] = mask_nms(pred["masks"], count, label_ids, iou_th=mask_nms_th, out=pred["masks"])
        return pred


def semantic_iou_counts(logits, labels, inter=None, union=None):
    """train.py:365-368 on the device.  logits (..., C) float32, labels (...) int32 (the leading shapes equal), inter, union (C - 1,)
    int64 accumulators or None (zeros) -> (inter, union): for s = 1..C-1, inter[s-1] += #(pred == s and label == s) and union[s-1] +=
    #(pred == s or label == s), with pred the FIRST maximal column (np.argmax).  Added in place: an epoch accumulates on the device
    without a read-back.  Integer adds: exact in any order."""
    logits = _typed(logits, torch.float32, None, "logits")
    labels = _typed(labels, torch.int32, None, "labels")
    if logits.dim() < 1 or tuple(labels.shape) != tuple(logits.shape[:-1]):
        raise ValueError("semantic_iou_counts: logits must be (..., C) and labels (...), got %s and %s" % (tuple(logits.shape), tuple(labels.shape)))
    c = int(logits.shape[-1])
    rows = labels.numel()
    if rows <= 0 or c < 2:
        raise ValueError("semantic_iou_counts: needs at least one row and two classes, got logits %s" % (tuple(logits.shape),))
    if c > SEM_IOU_MAX_C:
        raise NotImplementedError("semantic_iou_counts: C <= %d (got %d)" % (SEM_IOU_MAX_C, c))
    if (inter is None) != (union is None):
        raise ValueError("semantic_iou_counts: pass both accumulators or neither")
    for name, t in (("inter", inter), ("union", union)):
        if t is not None and (_typed(t, torch.int64, 1, name).shape[0] != c - 1 or not t.is_contiguous()):
            raise ValueError("semantic_iou_counts: %s must be a contiguous (C - 1,) = (%d,) tensor, got %s" % (name, c - 1, tuple(t.shape)))
    logits, labels = _on_device(logits=logits, labels=labels)
    if inter is None:
        inter = torch.zeros((c - 1,), dtype=torch.int64, device=logits.device)
        union = torch.zeros((c - 1,), dtype=torch.int64, device=logits.device)
    _on_device(inter=inter, union=union)
    with torch.cuda.device(logits.device):
        L.check(L.lib().gspn_sem_iou_counts(rows, c, L.ptr(logits), L.ptr(labels), L.ptr(inter), L.ptr(union), L.stream()), "semantic_iou_counts")
    return inter, union


def _numpy_sum(v):
    """The sum of a 1-D float64 tensor in the order np.add.reduce adds a contiguous vector (numpy's pairwise summation): below 8
    elements one after the other; up to 128, eight running sums over strides of 8, combined as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)),
    then the n % 8 last elements one after the other; above 128, the two halves (the first a multiple of 8) summed so and added.
    Element-wise IEEE adds on slices: the same bits on the host and on the device, nothing read back, every shape static."""
    n = v.shape[0]
    if n < 8:
        res = v[0]
        for i in range(1, n):
            res = res + v[i]
        return res
    if n <= 128:
        r = v[:8]
        for i in range(8, n - n % 8, 8):
            r = r + v[i:i + 8]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(n - n % 8, n):
            res = res + v[i]
        return res
    half = n // 2
    half -= half % 8
    return _numpy_sum(v[:half]) + _numpy_sum(v[half:])


def mean_iou(inter, union):
    """train.py:385-386: mean(inter / (union + 1e-8)) in float64 (a class that never occurs contributes 0 / 1e-8 = 0) -> a 0-d tensor.
    The quotients are added in np.mean's order (_numpy_sum) and the sum is divided, not multiplied by 1 / n, so the result is the
    reference's double bit for bit; torch's own mean on the device is one step of a double away from it on some inputs
    (tests/golden/predict/iou_ref.npz is one: sum * (1 / 18) is not sum / 18 there)."""
    iou = inter.double() / (union.double() + 1e-8)
    total = _numpy_sum(iou.reshape(-1))
    # divided by a TENSOR: by a Python number torch's device kernel multiplies by the rounded reciprocal, which loses the last bit
    return total / torch.full_like(total, float(iou.numel()))


# ---- host IO (test.py:96-114, :128-129), plain Python ---------------------------------------------------------------------------------

def _ints(values):
    return values.tolist() if hasattr(values, "tolist") else [int(v) for v in values]


def _write_ids(path, ids):
    """one integer per line, '%d\\n' each: the format of ScanNet's util_3d.export_ids"""
    with open(path, "w") as f:
        f.write("".join("%d\n" % v for v in ids))


def write_predictions(out_dir, scan, pred, scene=0):
    """test.py:96-114 for one scene of scene_predictions' result.  Writes <out_dir>/<scan>.txt with one line
    'pred_mask/<scan>_<k>.txt <label id> <confidence as %f>' per output row k < count whose mask is not empty, and that mask to
    <out_dir>/pred_mask/<scan>_<k>.txt, one 0 or 1 per scene point.  k is the position in output order: a row with an empty mask is
    skipped and still counted.  -> the number of masks written."""
    count = int(pred["count"][scene])
    labels = _ints(pred["label_ids"][scene][:count].cpu())
    confidence = _ints(pred["confidence"][scene][:count].cpu())
    points = _ints(pred["mask_points"][scene][:count].cpu())
    masks = pred["masks"][scene][:count].cpu().numpy()
    mask_dir = os.path.join(out_dir, "pred_mask")
    os.makedirs(mask_dir, exist_ok=True)
    written = 0
    with open(os.path.join(out_dir, scan + ".txt"), "w") as f:
        for k in range(count):
            if points[k] == 0:
                continue
            f.write("%s %d %f\n" % (os.path.join("pred_mask", "%s_%d.txt" % (scan, k)), labels[k], confidence[k]))
            _write_ids(os.path.join(mask_dir, "%s_%d.txt" % (scan, k)), masks[k].tobytes())
            written += 1
    return written


def write_ground_truth(out_dir, scan, seg_label, group_label, label_map=SCANNET_LABEL_MAP):
    """test.py:128-129 for one scene: seg_label, group_label (N,) integers -> <out_dir>/<scan>.txt with label_map[seg] * 1000 + group,
    one per line"""
    seg, group = _ints(seg_label.cpu() if isinstance(seg_label, torch.Tensor) else seg_label), \
        _ints(group_label.cpu() if isinstance(group_label, torch.Tensor) else group_label)
    if len(seg) != len(group):
        raise ValueError("write_ground_truth: seg_label and group_label must have one entry per point, got %d and %d" % (len(seg), len(group)))
    table = [int(v) for v in _ints(label_map)]
    os.makedirs(out_dir, exist_ok=True)
    _write_ids(os.path.join(out_dir, scan + ".txt"), (table[s] * 1000 + g for s, g in zip(seg, group)))
