"""Restatements, in numpy on the CPU, of the lift of predictions to a scan's own vertices (gspn_amd/lift.py), written from
the definition for its tests:
  * nearest: the first minimum of the unfused float32 (dx*dx + dy*dy) + dz*dz, brute force;
  * vertex_tables: src (the scene point nearest to each vertex) and vert_fb (fb_prob[nearest seed, 1]);
  * lift: per detection the mask value at the crop point nearest to each vertex inside the box (float32 box test, bounds included),
    the three sums by math.fsum (every term is a float32 or a product of two, exact in double), the thresholded mask and its size;
  * literal: test.py:163-189 and :204 line for line with the vertices as the points -- the (R, V) float64 matrix group_label_pred, its
    products with the lifted tables -- for the rows it keeps;
  * scan_prediction: the whole stage for one scan from the six arrays of a scene, ordered by predict_ref.rank;
  * synthetic scans around a scene (tools/test.py --synthetic_vertices) are checked against the generator itself."""
import math

import numpy as np

from tests import predict_ref as PR


def nearest(q, pts, chunk=2048):
    """q (V, 3), pts (M, 3) float32 -> (V,) int32: np.argmin's first minimum of the float32 distance"""
    q, pts = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(pts, np.float32)
    out = np.empty(len(q), np.int32)
    for lo in range(0, len(q), chunk):
        d = q[lo:lo + chunk, None, :] - pts[None, :, :]
        dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert dist.dtype == np.float32
        out[lo:lo + chunk] = np.argmin(dist, axis=1)
    return out


def nearest_threads(q, pts, chunk=1024):
    """nearest() by torch's CPU kernels, which use every core: the same float32 operations one by one (torch fuses nothing in eager
    mode) and torch.argmin's first minimum.  For the sizes at which numpy takes too long for a test; tests/test_cpu_lift.py holds the two
    equal where both are quick."""
    import torch
    q, pts = torch.from_numpy(np.ascontiguousarray(q, np.float32)), torch.from_numpy(np.ascontiguousarray(pts, np.float32))
    px, py, pz = (pts[:, a].contiguous()[None] for a in range(3))
    out = torch.empty(len(q), dtype=torch.int64)
    for lo in range(0, len(q), chunk):
        c = q[lo:lo + chunk]
        d0, d1, d2 = c[:, 0:1] - px, c[:, 1:2] - py, c[:, 2:3] - pz
        out[lo:lo + chunk] = torch.argmin((d0 * d0 + d1 * d1) + d2 * d2, 1)
    return out.numpy().astype(np.int32)


def vertex_tables(verts, pc, pc_seed, fb_prob, search=nearest):
    """-> src (V,) int32, vert_fb (V,) float32"""
    return search(verts, pc), np.ascontiguousarray(fb_prob[search(verts, pc_seed), 1])


def inside(verts, box):
    """verts (V, 3), box (6,) float32 -> (V,) bool: v >= c - s / 2 and v <= c + s / 2 on every axis, in float32 (box_common.h's test)"""
    box = box.astype(np.float32)
    half = box[3:6] / np.float32(2.0)
    lo, hi = box[:3] - half, box[:3] + half
    assert lo.dtype == hi.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return np.all((verts >= lo) & (verts <= hi), -1)


def values(verts, crops, boxes, masks):
    """g (R, V) float32: masks[k][nearest crop point of k] inside box k, 0 outside; for every row, whatever its class"""
    r, v = masks.shape[0], verts.shape[0]
    g = np.zeros((r, v), np.float32)
    for k in range(r):
        members = np.nonzero(inside(verts, boxes[k]))[0]
        if len(members):
            g[k, members] = masks[k][nearest(verts[members], crops[k])]
    return g


def lift(verts, crops, boxes, masks, class_ids, src, sem_prob, vert_fb, mask_th=0.4):
    """the definition of gspn_lift_masks -> sem_conf, fb_conf (R,) float64 from correctly rounded sums, mask (R, V) uint8, mask_points
    (R,) int32; zeros in the rows whose class is outside [1, C); src clamped into [0, N)"""
    assert all(a.dtype == np.float32 for a in (verts, crops, boxes, masks, sem_prob, vert_fb))
    r, v = masks.shape[0], verts.shape[0]
    n, c = sem_prob.shape
    src = np.clip(src, 0, n - 1)
    g = values(verts, crops, boxes, masks)
    sem_conf, fb_conf = np.zeros(r), np.zeros(r)
    mask, points = np.zeros((r, v), np.uint8), np.zeros(r, np.int32)
    for k in range(r):
        cls = int(class_ids[k])
        if cls <= 0 or cls >= c:
            continue
        at = np.nonzero(g[k])[0]                                                                          # a zero adds nothing
        gd = g[k, at].astype(np.float64)
        s0 = math.fsum(gd.tolist())
        s1 = math.fsum((gd * sem_prob[src[at], cls].astype(np.float64)).tolist())                       # 24 x 24 bits: exact products
        s2 = math.fsum((gd * vert_fb[at].astype(np.float64)).tolist())
        sem_conf[k], fb_conf[k] = s1 / (1e-8 + s0), s2 / (1e-8 + s0)
        mask[k] = g[k].astype(np.float64) > mask_th
        points[k] = mask[k].sum()
    return sem_conf, fb_conf, mask, points


def literal(verts, crops, boxes, masks, class_ids, src, sem_prob, vert_fb, mask_th=0.4):
    """test.py:163-189 and :204 with the vertices as the points, for the rows of a class > 0 (the reference has dropped the others by
    then) -> rows, sem_conf, fb_conf (float64, numpy's own order of adding), group_label_pred (len(rows), V) int32"""
    rows = np.where(class_ids > 0)[0]
    n = sem_prob.shape[0]
    sem_class_prob, fb = sem_prob[np.clip(src, 0, n - 1)], vert_fb                                       # the tables on the vertices
    group_label_pred = np.zeros((len(rows), verts.shape[0]))                                            # :163, float64
    for j, k in enumerate(rows):
        sidx = nearest(verts, crops[k])                                                                 # :165-167, every vertex as the ball tree does
        group_label_pred[j, :] = masks[k][sidx]                                                         # :168
        roi_mask = np.logical_and(verts >= np.reshape(boxes[k, :3] - boxes[k, 3:6] / 2, [1, 3]),
                                  verts <= np.reshape(boxes[k, :3] + boxes[k, 3:6] / 2, [1, 3]))
        roi_mask = np.logical_and(np.logical_and(roi_mask[:, 0], roi_mask[:, 1]), roi_mask[:, 2]).astype(np.float32)
        group_label_pred[j, :] = np.multiply(group_label_pred[j, :], roi_mask)                          # :173
    sem_conf = np.matmul(group_label_pred, sem_class_prob)                                              # :178
    sem_conf = np.divide(sem_conf, 1e-8 + np.sum(group_label_pred, 1, keepdims=True))                   # :179
    sem_conf = sem_conf.reshape(-1)[class_ids[rows].astype(np.int32) + np.arange(len(rows)) * sem_conf.shape[1]]
    fb_conf = np.matmul(group_label_pred, fb)                                                           # :188
    fb_conf = np.divide(fb_conf, 1e-8 + np.sum(group_label_pred, 1))                                    # :189
    return rows, sem_conf, fb_conf, (group_label_pred > mask_th).astype(np.int32)                       # :204


def scan_prediction(verts, pc, masks, crops, det, logits, pc_seed, fb_prob, sem_conf_th=0.01, fb_conf_th=0.01, mask_th=0.4,
                    seg_label_map=PR.SEG_LABEL_MAP, tables=None):
    """The whole stage for one scan from the arrays of its scene (predict_ref.output_prediction's arguments, the vertices in front).
    tables: (sem_prob (N, C), src (V,), vert_fb (V,)) to use in place of numpy's softmax and the brute-force search (the device's own,
    where the sums are checked to double rounding).  -> a dict with the device's shapes without the leading 1: order, count, label_ids,
    confidence, score, and sem_conf, fb_conf, masks, mask_points in output order, src"""
    if tables is None:
        sem_prob = PR.point_tables(pc, logits, pc_seed, fb_prob)[0]
        src, vert_fb = vertex_tables(verts, pc, pc_seed, fb_prob)
    else:
        sem_prob, src, vert_fb = tables
    c = sem_prob.shape[1]
    cls = det[:, 6].astype(np.int32)
    sem_conf, fb_conf, mask, points = lift(verts, crops, np.ascontiguousarray(det[:, :6]), masks, cls, src, sem_prob, vert_fb, mask_th)
    order, count, label_ids, confidence, score = PR.rank(det[None, :, 7], cls[None], sem_conf[None], fb_conf[None], sem_conf_th, fb_conf_th,
                                                         np.asarray(seg_label_map)[:c])
    at = order[0]
    return dict(order=at, count=int(count[0]), label_ids=label_ids[0], confidence=confidence[0], score=score[0], sem_conf=sem_conf[at],
                fb_conf=fb_conf[at], masks=mask[at], mask_points=points[at], src=src)
