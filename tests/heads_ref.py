"""Restatements, in plain torch on the CPU, for the tests of gspn_amd/heads.py: the first layer of the heads over the crop of
points_cropping (models/model_rpointnet.py:785-816 + the 1x1 convolution of :930 / :960) and the three R-PointNet losses (:1251-1323),
written from the reference's TensorFlow semantics -- tf.where / tf.gather / tf.gather_nd as real indexing and tf.cond as a Python `if`.
Everything runs in the dtype of its inputs; the tests hand in float64."""
import torch


def crop_rows(pc, pc_fea, pc_center, rois, idx, normalize=True):
    """the heads' input rows (B, R, P, C + 6) = concat(pc_fea[idx], (pc_center[idx] - centre) / size, (pc[idx] - centre) / size)"""
    b, r, p = idx.shape

    def take(x):
        i = idx.reshape(b, r * p, 1).long().expand(-1, -1, x.shape[2])
        return torch.gather(x, 1, i).reshape(b, r, p, x.shape[2])

    fea, cen, coord = take(pc_fea), take(pc_center), take(pc)
    centre = rois[:, :, :3].unsqueeze(2)
    coord, cen = coord - centre, cen - centre
    if normalize:
        rois = rois + (rois.sum(2, keepdim=True) == 0).to(rois.dtype)           # :812
        size = rois[:, :, 3:].unsqueeze(2)
        coord, cen = coord / size, cen / size
    return torch.cat((fea, cen, coord), -1)


def crop_linear(pc, pc_fea, pc_center, rois, idx, weights, biases, normalize=True):
    """gather, centre, divide, concat, . W + b"""
    return crop_rows(pc, pc_fea, pc_center, rois, idx, normalize) @ weights + biases


def crop_linear_case(b, n, c, r, p, cout, seed=0):
    """seeded inputs of crop_linear: the last ROI row of every scene is all zero with an index row of zeros, ROI 0 draws one point P times
    and every other row draws from a fifth of the points (duplicates)"""
    g = torch.Generator().manual_seed(seed)
    room = torch.tensor([8.0, 6.0, 3.0])
    pc = torch.rand(b, n, 3, generator=g) * room
    fea = torch.randn(b, n, c, generator=g)
    cen = pc + 0.1 * torch.randn(b, n, 3, generator=g)
    rois = torch.cat((torch.rand(b, r, 3, generator=g) * room, torch.rand(b, r, 3, generator=g) + 0.3), -1)
    rois[:, r - 1] = 0.0
    idx = torch.randint(0, max(n // 5, 2), (b, r, p), generator=g).int()
    idx[:, 0] = min(3, n - 1)
    idx[:, r - 1] = 0
    w = torch.randn(c + 6, cout, generator=g) / (c + 6) ** 0.5
    bias = torch.randn(cout, generator=g)
    return pc, fea, cen, rois, idx, w, bias


# ---- the losses ------------------------------------------------------------------------------------------------------------------------

def smooth_l1(y_true, y_pred):
    """:1223-1230 -> (loss, diff)"""
    diff = (y_true - y_pred).abs()
    less = (diff < 1.0).to(diff.dtype)
    return less * 0.5 * diff ** 2 + (1 - less) * (diff - 0.5), diff


def class_loss(logits, gt_class_ids, roi_valid_mask):
    """:1251-1262"""
    b, r, k = logits.shape
    ce = torch.nn.functional.cross_entropy(logits.reshape(-1, k), gt_class_ids.reshape(-1).long(), reduction='none').reshape(b, r)
    return (ce * roi_valid_mask).sum() / (roi_valid_mask.sum() + 1e-8)


def _selected(gt_class_ids, roi_valid_mask):
    """tf.where(valid > 0 and class > 0)[:, 0] (:1279, :1310)"""
    return torch.nonzero((roi_valid_mask.reshape(-1) > 0) & (gt_class_ids.reshape(-1) > 0))[:, 0]


def bbox_loss(gt_bbox, gt_class_ids, pred_bbox, roi_valid_mask, num_category):
    """:1264-1291 -> (loss, the smooth-L1 arguments of the selected rows)"""
    sel = _selected(gt_class_ids, roi_valid_mask)
    cls = gt_class_ids.reshape(-1).long()[sel]
    gt = gt_bbox.reshape(-1, 6)[sel]
    pred = pred_bbox.reshape(-1, num_category, 6)[sel, cls]
    if gt.numel() > 0:                                                              # tf.cond(tf.size(gt_bbox) > 0, ...)
        loss, diff = smooth_l1(gt, pred)
        return loss.sum(1).mean(0), diff
    return torch.zeros((), dtype=pred_bbox.dtype), torch.zeros(0, dtype=pred_bbox.dtype)


def mask_loss(gt_masks, gt_class_ids, pred_masks, roi_valid_mask, num_category, num_point_per_roi):
    """:1293-1323"""
    sel = _selected(gt_class_ids, roi_valid_mask)
    cls = gt_class_ids.reshape(-1).long()[sel]
    gt = gt_masks.reshape(-1, num_point_per_roi)[sel].to(pred_masks.dtype)
    pred = pred_masks.reshape(-1, num_point_per_roi, num_category).permute(0, 2, 1)[sel, cls]
    if gt.numel() > 0:
        return torch.nn.functional.binary_cross_entropy_with_logits(pred, gt, reduction='mean')
    return torch.zeros((), dtype=pred_masks.dtype)


def loss_case(kind, b=2, r=12, p=16, k=5, seed=0):
    """seeded end_points of get_rpointnet_loss.  kind: 'mixed' (positives first, then negatives, then zero padding, as
    detection_target_gen orders them), 'no_positive' (negatives and padding only) or 'all_padding' (every ROI row zero).
    Target deltas are placed so that no smooth-L1 argument of a selected row is near 1."""
    g = torch.Generator().manual_seed(seed)
    npos = {"mixed": (4, 3), "no_positive": (0, 0), "all_padding": (0, 0)}[kind]
    nneg = {"mixed": (5, 6), "no_positive": (7, 9), "all_padding": (0, 0)}[kind]
    rois = torch.zeros(b, r, 6)
    cls = torch.zeros(b, r, dtype=torch.int32)
    tbox = torch.zeros(b, r, 6)
    tmask = torch.zeros(b, r, p, dtype=torch.bool)
    pred_bbox = torch.randn(b, r, k, 6, generator=g)
    for i in range(b):
        live = npos[i] + nneg[i]
        rois[i, :live] = torch.cat((torch.rand(live, 3, generator=g) * 8 - 4, torch.rand(live, 3, generator=g) + 0.2), 1)
        cls[i, :npos[i]] = torch.randint(1, k, (npos[i],), generator=g).int()
        tmask[i, :npos[i]] = torch.rand(npos[i], p, generator=g) < 0.4
        # |target - prediction of the row's class| is either below 0.9 or above 1.1: both branches of smooth-L1, none on the kink
        d = torch.rand(npos[i], 6, generator=g) * 0.9
        far = torch.rand(npos[i], 6, generator=g) < 0.3
        d = torch.where(far, d + 1.1, d) * torch.where(torch.rand(npos[i], 6, generator=g) < 0.5, -1.0, 1.0)
        tbox[i, :npos[i]] = pred_bbox[i, torch.arange(npos[i]), cls[i, :npos[i]].long()] + d
    return {"rois": rois, "target_class_ids": cls, "target_bbox": tbox, "target_mask": tmask,
            "rpointnet_class_logits": torch.randn(b, r, k, generator=g) * 2, "rpointnet_bbox": pred_bbox,
            "rpointnet_mask": torch.randn(b, r, p, k, generator=g) * 3}
