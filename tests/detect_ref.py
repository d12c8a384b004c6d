"""Restatements, in plain torch / numpy on the CPU, of the detection output stage of models/model_rpointnet.py -- the per-class NMS of
refine_detections (:855-901), refine_detections itself from the refined boxes on (:846-913), select_segmentation (:986-1006), the argmin and
the box mask of unmold_segmentation (:1008-1048) -- written from the reference's text for the tests of gspn_amd/detect.py, and the seeded
inputs those tests run on.  The per-class NMS is the literal loop: over the unique classes, roi_ref.nms_3d on the rows of each (pinned to the
reference's own function by golden/roi/nms3d_ref.npz), the intersection of index sets, top_k with the lower index first."""
import numpy as np
import torch

from tests import roi_ref as RR

# ---- the per-class NMS (:855-901) --------------------------------------------------------------------------------------------------


def class_nms_scene(boxes, scores, class_ids, max_per_class, max_output_size, iou_threshold, nms=None):
    """boxes (N, 6), scores (N,), class_ids (N,) -> the kept rows, at most max_output_size, in the order of top_k.  `nms`: a function
    with nms_3d's signature on numpy arrays (the generator of the golden file passes the reference's own); roi_ref.nms_3d otherwise."""
    keep = torch.nonzero(class_ids > 0)[:, 0]                                            # :847, ascending
    pre_ids, pre_scores, pre_rois = class_ids[keep], scores[keep], boxes[keep]
    nms_keep = []
    for c in np.unique(pre_ids.numpy()):                                                 # :861 (the order of the classes does not matter)
        ixs = torch.nonzero(pre_ids == int(c))[:, 0]
        if nms is None:
            ck = RR.nms_3d(pre_rois[ixs][None], pre_scores[ixs][None], -1, max_per_class, iou_threshold)[0]
        else:
            ck = torch.from_numpy(nms(pre_rois[ixs][None].numpy(), pre_scores[ixs][None].numpy(), -1, max_per_class, iou_threshold, float("-inf"))[0])
        ck = ck[ck > -1].long()                                                          # :874
        nms_keep.extend(keep[ixs[ck]].tolist())                                          # :877
    kept = sorted(set(keep.tolist()) & set(nms_keep))                                    # :893, a set: repeated picks collapse
    kept = torch.tensor(kept, dtype=torch.int64)
    order = torch.sort(-scores[kept], stable=True).indices[:max_output_size]             # :897-901, the lower index first among equals
    return kept[order]


def class_nms(boxes, scores, class_ids, max_per_class, max_output_size, iou_threshold, nms=None):
    """(B, N, 6), (B, N), (B, N) -> (B, max_output_size) int32, -1 padded"""
    out = -torch.ones((boxes.shape[0], max_output_size), dtype=torch.int32)
    for i in range(boxes.shape[0]):
        rows = class_nms_scene(boxes[i].float(), scores[i].float(), class_ids[i], max_per_class, max_output_size, iou_threshold, nms)
        out[i, :len(rows)] = rows.int()
    return out


def class_nms_one_pass(boxes, scores, class_ids, max_per_class, max_output_size, iou_threshold):
    """the formulation of the kernel: ONE pass over all candidates in score order; a pick suppresses within its class only, and its class
    is exhausted after max_per_class picks or after a pick that survives its own IoU test"""
    boxes, scores = boxes.float(), scores.float()
    thr, eps = torch.tensor(iou_threshold, dtype=torch.float32), torch.tensor(1e-8, dtype=torch.float32)
    out = -torch.ones((boxes.shape[0], max_output_size), dtype=torch.int32)
    for i in range(boxes.shape[0]):
        order = torch.sort(-scores[i], stable=True).indices
        live = order[class_ids[i][order] > 0]
        lo, hi = boxes[i, :, :3] - boxes[i, :, 3:] / 2, boxes[i, :, :3] + boxes[i, :, 3:] / 2
        vol = boxes[i, :, 3] * boxes[i, :, 4] * boxes[i, :, 5]
        picks = {}
        count = 0
        while len(live) > 0 and count < max_output_size:
            k = live[0]
            c = int(class_ids[i][k])
            out[i, count] = k
            count += 1
            picks[c] = picks.get(c, 0) + 1
            cube = torch.clamp(torch.minimum(hi[k], hi[live]) - torch.maximum(lo[k], lo[live]), min=0)
            inter = cube[:, 0] * cube[:, 1] * cube[:, 2]
            gone = (inter / (vol[live] + vol[k] - inter + eps)) > thr
            if not bool(gone[0]) or picks[c] >= max_per_class:
                gone = torch.ones_like(gone)
            live = live[~(gone & (class_ids[i][live] == c))]
    return out


def class_boxes(b, n, classes, seed, zero_volume=0, empty_scenes=()):
    """roi_ref.nms_boxes with a class in 0..classes per row (0: no candidate; about one row in classes + 1), `zero_volume` candidates
    per scene flattened on one axis, and the scenes of `empty_scenes` all of class 0"""
    boxes, scores = RR.nms_boxes(b, n, seed)
    g = torch.Generator().manual_seed(seed + 7)
    class_ids = torch.randint(0, classes + 1, (b, n), generator=g).int()
    for i in range(b):
        rows = torch.randperm(n, generator=g)[:zero_volume]
        boxes[i, rows, 3 + i % 3] = 0.0
        class_ids[i, rows] = torch.clamp(class_ids[i, rows], min=1)
        if i in empty_scenes:
            class_ids[i] = 0
    return boxes.contiguous(), scores.contiguous(), class_ids.contiguous()


# name -> (b, n, classes, seed, zero_volume, empty_scenes, max_per_class, max_output_size, iou_threshold)
CLASS_NMS_CASES = {
    "detect_384": (2, 384, 18, 41, 0, (), 100, 100, 0.1),
    "detect_zero_volume": (2, 384, 18, 42, 6, (), 100, 100, 0.1),
    "per_class_5": (2, 512, 3, 43, 0, (), 5, 100, 0.1),
    "few_classes_0.5": (2, 300, 2, 44, 3, (), 40, 64, 0.5),
    "empty_scene": (3, 200, 18, 45, 2, (1,), 100, 100, 0.1),
    "fewer_than_outputs": (1, 40, 4, 46, 0, (), 100, 100, 0.3),
}


def class_nms_case(name):
    b, n, classes, seed, zero_volume, empty, per_class, m, thr = CLASS_NMS_CASES[name]
    return class_boxes(b, n, classes, seed, zero_volume, empty) + (per_class, m, thr)


# ---- refine_detections (:846-913) from the refined boxes on ------------------------------------------------------------------------


def first_argmax(probs):
    """tf.argmax: the lowest column among equal maxima.  probs (..., C) -> (...) int32, and that probability"""
    top = probs.max(-1, keepdim=True).values
    ids = torch.from_numpy(np.argmax((probs == top).numpy(), axis=-1))                    # numpy's argmax takes the first True
    return ids.int(), torch.gather(probs, -1, ids.unsqueeze(-1)).squeeze(-1)


def refine_detections(refined, class_ids, class_scores, fb_prob, sem_prob, min_confidence, max_instances, iou_threshold):
    """refined (B, R, 6), class_ids (B, R) int32, class_scores, fb_prob, sem_prob (B, R) -> (B, max_instances, 8)"""
    b = refined.shape[0]
    out = torch.zeros((b, max_instances, 8), dtype=torch.float32)
    score = class_scores * fb_prob * sem_prob                                             # :859, left to right in fp32
    for i in range(b):
        ids = class_ids[i].clone()
        if min_confidence:
            ids[~(class_scores[i] >= torch.tensor(min_confidence, dtype=torch.float32))] = 0          # :849-853
        keep = class_nms_scene(refined[i], score[i], ids, max_instances, max_instances, iou_threshold)
        out[i, :len(keep)] = torch.cat((refined[i][keep], class_ids[i][keep].float()[:, None], class_scores[i][keep][:, None]), 1)
    return out


# ---- select_segmentation, unmold_segmentation --------------------------------------------------------------------------------------


def select_segmentation(masks, class_ids):
    """:986-1006 as written: reshape, transpose, gather_nd by (row, class).  (B, R, P, C), (B, R) -> (B, R, P)"""
    b, r, p, c = masks.shape
    flat = masks.reshape(-1, p, c).permute(0, 2, 1)
    return flat[torch.arange(b * r), class_ids.reshape(-1).long()].reshape(b, r, p)


def _first_argmin(q, s):
    """q (M, 3), s (P, 3) float32 numpy -> (M,) int32"""
    arg = np.empty(len(q), dtype=np.int32)
    for n0 in range(0, len(q), 2048):
        d = q[n0:n0 + 2048, None, :] - s[None, :, :]
        dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert dist.dtype == np.float32
        arg[n0:n0 + 2048] = np.argmin(dist, axis=1)                                       # numpy's argmin takes the first minimum
    return arg


def nearest_in_sets(query, sets, rois=None):
    """query (B, N, 3), sets (B, R, P, 3), rois (B, R, 6) or None -> (B, R, N) int32: first-index argmin of d0*d0 + d1*d1 + d2*d2 in
    float32; -1 outside the box (the inside test of :1042; the argmin of those queries is not computed, to keep the tests quick)"""
    b, n, _ = query.shape
    r = sets.shape[1]
    out = -torch.ones((b, r, n), dtype=torch.int32)
    for i in range(b):
        q = query[i].numpy().astype(np.float32)
        for k in range(r):
            s = sets[i, k].numpy().astype(np.float32)
            if rois is None:
                out[i, k] = torch.from_numpy(_first_argmin(q, s))
            else:
                members = RR.inside(rois[i, k:k + 1], query[i])[0]
                out[i, k][members] = torch.from_numpy(_first_argmin(q[members.numpy()], s))
    return out


def unmold_segmentation(masks, rois, class_ids, pc_coord_cropped, pc):
    """:1008-1048: the selected mask at the nearest crop point, times the box mask.  -> (B, R, N).  The product with a mask of 0 is a zero
    of either sign whatever the argmin, so the argmin is taken inside the boxes only."""
    sel = select_segmentation(masks, class_ids)
    idx = nearest_in_sets(pc, pc_coord_cropped, rois)
    inside = (idx >= 0).float()
    return torch.gather(sel, 2, idx.clamp(min=0).long()) * inside
