"""The detection output stage of models/model_rpointnet.py, from the outputs of the two heads to the final detections and their masks on
the whole cloud, on the HIP kernels of csrc/detect.hip: refine_detections (:818-913), select_segmentation (:986-1006) and
unmold_segmentation (:1008-1048).  None of them is a head and none owns a variable.

refine_detections calls nms_3d once per class through a py_func in the reference; here class_nms_3d takes all classes of all scenes in
one launch.  unmold_segmentation is a (B, R, N, P) distance tensor in the reference, which does not fit at the inference shapes (test.py
redoes it on the host with a ball tree, one detection at a time, :163-173); here nearest_in_sets searches only the points inside each
detection's box and writes (B, R, N) indices.  Every shape is static and nothing reads a value back to the host, so the chain
refine_detections_batch -> mask_selection_gen_batch -> points_cropping -> unmold_segmentation captures in a graph.CapturedStep.  Nothing
here has a gradient (the reference runs all of it behind stop_gradient or at inference).  No CPU fallback."""
import torch

from . import _lib as L
from .roi import _constant, _take_rows, apply_box_delta
from .spn_boxes import box_shrink

__all__ = ["class_nms_3d", "first_max_column", "classified_boxes", "refine_detections_batch", "refine_detections", "select_segmentation", "nearest_in_sets",
           "unmold_segmentation"]


def class_nms_3d(boxes, scores, class_ids, max_per_class, max_output_size, iou_threshold):
    """The per-class NMS of :855-901 for the whole batch (an extension).  boxes (B, N, 6), scores (B, N), class_ids (B, N) int32 ->
    (B, max_output_size) int32, -1 padded.  The rows with class_ids > 0 are the candidates; within one class the picks are nms_3d's
    (pre_nms_limit -1, no score threshold, at most max_per_class picks, a pick that survives its own IoU test repeated until the class
    is full and counted once); classes do not suppress each other.  The picked rows of all classes come out in descending score, the
    lower index first among equal scores, the first max_output_size of them.  N <= 4096."""
    boxes = L.need(boxes.detach(), torch.float32, 3, "boxes")
    scores = L.need(scores.detach(), torch.float32, 2, "scores")
    class_ids = L.need(class_ids, torch.int32, 2, "class_ids")
    b, n, _ = boxes.shape
    if boxes.shape[2] != 6 or tuple(scores.shape) != (b, n) or tuple(class_ids.shape) != (b, n):
        raise ValueError("class_nms_3d: boxes must be (B, N, 6), scores and class_ids (B, N), got %s, %s and %s"
                         % (tuple(boxes.shape), tuple(scores.shape), tuple(class_ids.shape)))
    if int(max_per_class) <= 0 or int(max_output_size) <= 0:
        raise ValueError("class_nms_3d: max_per_class and max_output_size must be positive, got %d and %d" % (max_per_class, max_output_size))
    out = torch.empty((b, int(max_output_size)), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        L.check(L.lib().gspn_class_nms3d(b, n, int(max_per_class), int(max_output_size), float(iou_threshold), L.ptr(boxes), L.ptr(scores),
                                         L.ptr(class_ids), L.ptr(out), L.stream()), "class_nms_3d")
    return out


def first_max_column(values):
    """values (..., C) -> (...) int64: the FIRST maximal column, as tf.argmax picks it (torch.argmax leaves the choice among equal maxima
    open).  Shared by classified_boxes (:832) and the inference driver's pick of each ROI's semantic probability (:1159)."""
    c = values.shape[-1]
    top = values.max(-1, keepdim=True).values
    columns = torch.arange(c, device=values.device)
    return torch.where(values == top, columns, columns.new_full((), c - 1)).min(-1).values      # the lowest column of the maximum


def classified_boxes(rois, probs, deltas, pc, config):
    """:832-844 for the whole batch.  rois (B, R, 6), probs (B, R, C), deltas (B, R, C, 6), pc (B, N, 3) -> class_ids (B, R) int32: the
    FIRST maximal column of probs (tf.argmax; torch.argmax leaves the choice among equal maxima open), class_scores (B, R): that
    probability, refined_rois (B, R, 6): apply_box_delta with the deltas of that class times BBOX_STD_DEV, shrunk when SHRINK_BOX."""
    rois = L.need(rois.detach(), torch.float32, 3, "rois")
    probs = L.need(probs.detach(), torch.float32, 3, "probs")
    deltas = L.need(deltas.detach(), torch.float32, 4, "deltas")
    pc = L.need(pc.detach(), torch.float32, 3, "pc")
    b, r, c = probs.shape
    if tuple(rois.shape) != (b, r, 6) or tuple(deltas.shape) != (b, r, c, 6) or pc.shape[0] != b or pc.shape[2] != 3:
        raise ValueError("refine_detections: expected rois (B, R, 6), probs (B, R, C), deltas (B, R, C, 6) and pc (B, N, 3), got %s, %s, %s, %s"
                         % (tuple(rois.shape), tuple(probs.shape), tuple(deltas.shape), tuple(pc.shape)))
    class_ids = first_max_column(probs)
    class_scores = torch.gather(probs, 2, class_ids.unsqueeze(-1)).squeeze(-1)
    deltas_specific = torch.gather(deltas, 2, class_ids.reshape(b, r, 1, 1).expand(b, r, 1, 6)).squeeze(2)
    refined = apply_box_delta(rois, deltas_specific * _constant(config.BBOX_STD_DEV, rois.device))
    if config.SHRINK_BOX:
        refined = box_shrink(refined, pc)
    return class_ids.int(), class_scores, refined.contiguous()


def refine_detections_batch(rois, probs, deltas, pc, fb_prob, sem_prob, config):
    """:818-913 for the whole batch.  rois (B, R, 6) zero padded, probs (B, R, C), deltas (B, R, C, 6), pc (B, N, 3), fb_prob, sem_prob
    (B, R) -> detections (B, DETECTION_MAX_INSTANCES, 8): [refined box, class id, class score] in descending NMS score
    (class score * fb_prob) * sem_prob, rows of zeros behind the last detection.  The candidates are the ROIs of a class > 0 whose class
    score is >= DETECTION_MIN_CONFIDENCE (when that is truthy); the per-class NMS is class_nms_3d with DETECTION_MAX_INSTANCES picks per
    class and in all, at DETECTION_NMS_THRESHOLD.  Column 7 is the class score, not the product (:907)."""
    class_ids, class_scores, refined = classified_boxes(rois, probs, deltas, pc, config)
    fb_prob = L.need(fb_prob.detach(), torch.float32, 2, "fb_prob")
    sem_prob = L.need(sem_prob.detach(), torch.float32, 2, "sem_prob")
    if fb_prob.shape != class_ids.shape or sem_prob.shape != class_ids.shape:
        raise ValueError("refine_detections: fb_prob and sem_prob must be (B, R) = %s, got %s and %s"
                         % (tuple(class_ids.shape), tuple(fb_prob.shape), tuple(sem_prob.shape)))
    keep = class_ids > 0
    if config.DETECTION_MIN_CONFIDENCE:
        keep = keep & (class_scores >= _constant((config.DETECTION_MIN_CONFIDENCE,), rois.device))
    score = (class_scores * fb_prob) * sem_prob                                                     # :859
    m = int(config.DETECTION_MAX_INSTANCES)
    selected = class_nms_3d(refined, score, torch.where(keep, class_ids, torch.zeros_like(class_ids)), m, m, config.DETECTION_NMS_THRESHOLD)
    rows = torch.cat((refined, class_ids.float().unsqueeze(-1), class_scores.unsqueeze(-1)), -1)
    return _take_rows(rows, selected)


def refine_detections(rois, probs, deltas, pc, fb_prob, sem_prob, config):
    """:818-913 with the reference's per-scene signature: rois (R, 6), probs (R, C), deltas (R, C, 6), pc (N, 3), fb_prob, sem_prob (R,)
    -> (DETECTION_MAX_INSTANCES, 8).  A thin wrapper of the batch form."""
    return refine_detections_batch(rois.unsqueeze(0), probs.unsqueeze(0), deltas.unsqueeze(0), pc.unsqueeze(0), fb_prob.unsqueeze(0),
                                   sem_prob.unsqueeze(0), config)[0]


def select_segmentation(rpointnet_masks, class_ids):
    """:986-1006.  rpointnet_masks (B, R, P, C), class_ids (B, R) (any integer or float dtype, cast to an integer as the reference does)
    -> (B, R, P): each ROI's mask of its own class."""
    if rpointnet_masks.dim() != 4 or tuple(class_ids.shape) != tuple(rpointnet_masks.shape[:2]):
        raise ValueError("select_segmentation: expected rpointnet_masks (B, R, P, C) and class_ids (B, R), got %s and %s"
                         % (tuple(rpointnet_masks.shape), tuple(class_ids.shape)))
    b, r, p, _ = rpointnet_masks.shape
    return torch.gather(rpointnet_masks.detach(), 3, class_ids.long().reshape(b, r, 1, 1).expand(b, r, p, 1)).squeeze(3)


def nearest_in_sets(query, sets, rois=None):
    """The nearest point of each set for every query point (an extension: the argmin of :1032-1033 behind the box test of :1042, and with
    one set per scene the nearest seed of :1136).  query (B, N, 3), sets (B, R, P, 3) -- or (B, P, 3), one set per scene, R = 1 --,
    rois (B, R, 6) or None -> (B, R, N) int32: the position in the set of smallest (dx*dx + dy*dy) + dz*dz, the lowest position among
    equal distances.  With rois, a query outside box k (q >= c - s/2 and q <= c + s/2 on all axes is inside) gets -1 in row k and is not
    searched.  P <= 4096, N <= 32768."""
    query = L.need(query.detach(), torch.float32, 3, "query")
    if isinstance(sets, torch.Tensor) and sets.dim() == 3:
        sets = sets.unsqueeze(1)
    sets = L.need(sets.detach(), torch.float32, 4, "sets")
    b, n, _ = query.shape
    r, p = sets.shape[1], sets.shape[2]
    if query.shape[2] != 3 or sets.shape[0] != b or sets.shape[3] != 3:
        raise ValueError("nearest_in_sets: query must be (B, N, 3) and sets (B, R, P, 3) or (B, P, 3), got %s and %s"
                         % (tuple(query.shape), tuple(sets.shape)))
    if rois is not None:
        rois = L.need(rois.detach(), torch.float32, 3, "rois")
        if tuple(rois.shape) != (b, r, 6):
            raise ValueError("nearest_in_sets: rois must be (B, R, 6) = (%d, %d, 6), got %s" % (b, r, tuple(rois.shape)))
    out = torch.empty((b, r, n), dtype=torch.int32, device=query.device)
    with torch.cuda.device(query.device):
        L.check(L.lib().gspn_nearest_in_sets(b, r, n, p, L.ptr(query), L.ptr(sets), L.ptr(rois), L.ptr(out), L.stream()), "nearest_in_sets")
    return out


def unmold_segmentation(rpointnet_masks, rois, class_ids, pc_coord_cropped, pc):
    """:1008-1048.  rpointnet_masks (B, R, P, C), rois (B, R, 6), class_ids (B, R), pc_coord_cropped (B, R, P, 3) (the crop points in the
    coordinates of pc: points_cropping's unnormalised output), pc (B, N, 3) -> (B, R, N): for every point of the cloud inside ROI k, the
    value of k's selected mask at the nearest crop point; 0 outside the box.  The reference takes the argmin everywhere and multiplies
    by the box mask; for finite mask values that is the same number (up to the sign of a zero)."""
    if rpointnet_masks.dim() != 4 or pc_coord_cropped.dim() != 4 or tuple(rpointnet_masks.shape[:3]) != tuple(pc_coord_cropped.shape[:3]):
        raise ValueError("unmold_segmentation: rpointnet_masks %s and pc_coord_cropped %s must share (B, R, P)"
                         % (tuple(rpointnet_masks.shape), tuple(pc_coord_cropped.shape)))
    masks = select_segmentation(rpointnet_masks, class_ids)
    idx = nearest_in_sets(pc, pc_coord_cropped, rois)
    picked = torch.gather(masks, 2, idx.clamp(min=0).long())
    return torch.where(idx >= 0, picked, torch.zeros((), dtype=masks.dtype, device=masks.device))
