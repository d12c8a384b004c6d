"""Box arithmetic of GSPN's shape proposal stage (models/model_rpointnet.py) on the HIP kernels of csrc/spn_boxes.hip: box_shrink
(:529-551), the per-row bounding boxes behind bbox_ins_pred (:406-408) and pc_ins_center (:358), and spn_target_gen (:599-644) for a
whole batch.  Boxes are (centre x, y, z, size l, w, h), fp32.  No CPU fallback."""
import torch

from . import _lib as L


def box_shrink(box, pc):
    """:529-551.  box (B, S, 6), pc (B, N, 3) -> (B, S, 6): each box shrunk to the bounding box of the points inside it, plus 1e-3 on
    every size; six zeros for a box with no point inside or whose inside points are flat on an axis.  A point is inside when
    pc >= c - size/2 and pc <= c + size/2 on all three axes, both bounds in fp32 as written.  This is what the reference's gamma = 1e4
    formulation computes while |coordinate| < 5e3 (an outside point moved by gamma must stay outside every inside point); unlike it,
    nothing of size (B, S, N) is ever written.  The output carries no gradient (min / max of input points)."""
    box = L.need(box.detach(), torch.float32, 3, "box")
    pc = L.need(pc.detach(), torch.float32, 3, "pc")
    if box.shape[2] != 6 or pc.shape[2] != 3 or pc.shape[0] != box.shape[0]:
        raise ValueError("box_shrink: box must be (B, S, 6) and pc (B, N, 3), got %s and %s" % (tuple(box.shape), tuple(pc.shape)))
    b, s, _ = box.shape
    out = torch.empty_like(box)
    with torch.cuda.device(box.device):
        L.check(L.lib().gspn_box_shrink(b, s, pc.shape[1], L.ptr(box), L.ptr(pc), L.ptr(out), L.stream()), "box_shrink")
    return out


def points_bbox(pts, offset=None):
    """pts (..., M, 3), offset (..., 3) or None -> (..., 6): [(hi + lo)/2, hi - lo] with hi / lo the max / min over the M points of
    pts + offset.  Rounding is monotone, so adding the offset before or after the reduction gives the same bits as the reference's
    add-then-reduce.  The output carries no gradient and is returned detached: the reference only ever uses these boxes behind
    stop_gradient (spn_match, the detection targets) or computes them from input data (pc_ins)."""
    pts = L.need(pts.detach(), torch.float32, None, "pts")
    if pts.dim() < 3 or pts.shape[-1] != 3:
        raise ValueError("points_bbox: pts must be (..., M, 3), got %s" % (tuple(pts.shape),))
    lead, m = pts.shape[:-2], pts.shape[-2]
    rows = 1
    for d in lead:
        rows *= d
    if offset is not None:
        offset = L.need(offset.detach(), torch.float32, None, "offset")
        if tuple(offset.shape) != tuple(lead) + (3,):
            raise ValueError("points_bbox: offset must be %s, got %s" % (tuple(lead) + (3,), tuple(offset.shape)))
    out = torch.empty(tuple(lead) + (6,), dtype=torch.float32, device=pts.device)
    with torch.cuda.device(pts.device):
        L.check(L.lib().gspn_points_bbox(rows, m, L.ptr(pts), L.ptr(offset), L.ptr(out), L.stream()), "points_bbox")
    return out


def spn_target_gen_batch(proposals, proposal_seed_class_ids, gt_class_ids, gt_boxes):
    """:599-644 for the whole batch in one launch.  proposals (B, S, 6), proposal_seed_class_ids (B, S) (1 = foreground seed),
    gt_class_ids (B, G) (<= 0: padding, skipped in place), gt_boxes (B, G, 6) -> spn_match (B, S) int32: 1 positive, -1 negative,
    0 neutral.  No shape depends on the data, so the call can sit inside a captured step."""
    proposals = L.need(proposals.detach(), torch.float32, 3, "proposals")
    gt_boxes = L.need(gt_boxes.detach(), torch.float32, 3, "gt_boxes")
    seed_cls = L.need(proposal_seed_class_ids.detach().float(), torch.float32, 2, "proposal_seed_class_ids")
    gt_cls = L.need(gt_class_ids.detach().float(), torch.float32, 2, "gt_class_ids")
    b, s, _ = proposals.shape
    g = gt_boxes.shape[1]
    if proposals.shape[2] != 6 or tuple(gt_boxes.shape) != (b, g, 6) or tuple(seed_cls.shape) != (b, s) or tuple(gt_cls.shape) != (b, g):
        raise ValueError("spn_target_gen: expected proposals (B, S, 6), seed classes (B, S), gt classes (B, G), gt boxes (B, G, 6)")
    out = torch.empty((b, s), dtype=torch.int32, device=proposals.device)
    with torch.cuda.device(proposals.device):
        L.check(L.lib().gspn_spn_target_gen(b, s, g, L.ptr(proposals), L.ptr(seed_cls), L.ptr(gt_cls), L.ptr(gt_boxes), L.ptr(out), L.stream()),
                "spn_target_gen")
    return out
