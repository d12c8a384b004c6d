"""The ROI stage of models/model_rpointnet.py, from SPN's proposals to the inputs of the two heads, on the HIP kernels of csrc/roi.hip:
nms_3d (:436-466), the inside-point count and sample_points_within_box (:584-597), detection_target_gen (:647-747), mask_selection_gen
(:749-783), points_cropping (:785-816), box_refinement (:553) and apply_box_delta (:570).  Boxes are (centre x, y, z, size l, w, h), fp32.

Every shape is static, nothing reads a value back to the host and nothing of size (boxes, points) is written: the reference's numpy loops,
its tf.where / boolean_mask trims and the (B, N, NUM_GROUP) one-hot of group_label are replaced by index tensors with -1 for "nothing".
The chain nms_3d -> gather_selection -> detection_target_gen_batch -> points_cropping -> backward captures in a graph.CapturedStep.

Random numbers come from the stateless generator gspn_roi_rand32 (include/gspn_hip.h).  `seed` is a one-element int64 tensor on the
device, or a Python int (copied to the device, which a stream capture does not allow: pass a tensor there).  A captured step draws
afresh on every replay once the caller has added to that tensor.  The inference crops also take `scene_seeds`, a (B,) int64 device tensor
with a seed per scene: a scene then draws what it draws alone, whichever batch and slot it is run in (tester.py).  No CPU fallback."""
import torch

from . import _lib as L
from . import invlists
from .tf_grouping import group_point

__all__ = ["nms_3d", "box_point_count", "sample_points_in_boxes", "detection_target_select", "detection_target_gen_batch",
           "detection_target_gen", "mask_selection_gen_batch", "mask_selection_gen", "points_cropping", "box_refinement", "apply_box_delta",
           "seed_tensor", "scene_seed_tensor"]

MASK_SELECTION_MARGIN = 1e-3          # :764-765


def seed_tensor(seed, device):
    """the one-element int64 device tensor the kernels read their seed from"""
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.numel() != 1:
            raise ValueError("seed must be a one-element int64 tensor, got %s %s" % (seed.dtype, tuple(seed.shape)))
        if not seed.is_cuda:
            raise L.GspnHipError("seed is on %s: gspn_amd runs on ROCm devices only (no CPU fallback)" % seed.device)
        return seed.contiguous()
    return torch.tensor([int(seed)], dtype=torch.int64, device=device)


def scene_seed_tensor(scene_seeds, batched, what):
    """the (B,) int64 device tensor the per-scene form of the crop sampler reads its seeds from, one per scene of `batched` (B, ...).
    Checked before anything else, so that a tensor that does not fit raises ValueError wherever the others live."""
    if not isinstance(scene_seeds, torch.Tensor):
        raise TypeError("scene_seeds must be a torch.Tensor")
    b = batched.shape[0] if isinstance(batched, torch.Tensor) and batched.dim() else 0
    if scene_seeds.dtype != torch.int64 or scene_seeds.dim() != 1 or scene_seeds.shape[0] != int(b):
        raise ValueError("%s: scene_seeds must be a (B,) = (%d,) int64 tensor, got %s %s" % (what, b, scene_seeds.dtype, tuple(scene_seeds.shape)))
    if not scene_seeds.is_cuda:
        raise L.GspnHipError("scene_seeds is on %s: gspn_amd runs on ROCm devices only (no CPU fallback)" % scene_seeds.device)
    if not scene_seeds.is_contiguous():
        raise ValueError("%s: scene_seeds must be contiguous" % what)
    return scene_seeds.detach()


def _boxes_and_points(boxes, pc, what):
    boxes = L.need(boxes.detach(), torch.float32, 3, "boxes")
    pc = L.need(pc.detach(), torch.float32, 3, "pc")
    if boxes.shape[2] != 6 or pc.shape[2] != 3 or pc.shape[0] != boxes.shape[0]:
        raise ValueError("%s: boxes must be (B, S, 6) and pc (B, N, 3), got %s and %s" % (what, tuple(boxes.shape), tuple(pc.shape)))
    return boxes, pc


def nms_3d(boxes, scores, pre_nms_limit, max_output_size, iou_threshold=0.5, score_threshold=float('-inf')):
    """:436-466 on the device.  boxes (B, N, 6), scores (B, N) -> selected_indices (B, max_output_size) int32, -1 padded.  Bit-faithful to
    the reference's numpy loop: IoUs in its fp32 order, both thresholds rounded to fp32 as numpy does, and a picked box leaves only by its
    own IoU test, so a zero-volume box (self-IoU 0) is picked again until the output is full.  Among equal scores the lower index comes
    first (the reference's argsort is not stable and leaves that order open).  N <= 4096."""
    boxes = L.need(boxes.detach(), torch.float32, 3, "boxes")
    scores = L.need(scores.detach(), torch.float32, 2, "scores")
    b, n, _ = boxes.shape
    if boxes.shape[2] != 6 or tuple(scores.shape) != (b, n):
        raise ValueError("nms_3d: boxes must be (B, N, 6) and scores (B, N), got %s and %s" % (tuple(boxes.shape), tuple(scores.shape)))
    out = torch.empty((b, int(max_output_size)), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        L.check(L.lib().gspn_nms3d(b, n, int(pre_nms_limit), int(max_output_size), float(iou_threshold), float(score_threshold), L.ptr(boxes),
                                   L.ptr(scores), L.ptr(out), L.stream()), "nms_3d")
    return out


def box_point_count(boxes, pc, margin=0.0):
    """boxes (B, S, 6), pc (B, N, 3) -> (B, S) int32: the points with pc >= (c - s/2) - margin and pc <= (c + s/2) + margin on all axes
    (:673-676 with margin 0, :764-766 with 1e-3)."""
    boxes, pc = _boxes_and_points(boxes, pc, "box_point_count")
    b, s, _ = boxes.shape
    out = torch.empty((b, s), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        L.check(L.lib().gspn_box_point_count(b, s, pc.shape[1], float(margin), L.ptr(boxes), L.ptr(pc), L.ptr(out), L.stream()), "box_point_count")
    return out


def sample_points_in_boxes(boxes, pc, nsmp, seed, margin=0.0, scene_seeds=None):
    """sample_points_within_box (:584-597) from the boxes themselves; the reference's (boxes, points) mask matrix is never built.
    boxes (B, R, 6), pc (B, N, 3) -> (B, R, nsmp) int32: nsmp draws with replacement, uniform over the points inside each box (the test of
    box_point_count); a row of zeros for a box with no inside point and for an all-zero box.  N <= 32768.
    scene_seeds: None, or a contiguous (B,) int64 device tensor, one seed per scene (gspn_sample_points_in_boxes_seeds).  Row s is then
    what this call gives for scene s alone with the one seed scene_seeds[s] -- whichever batch and slot the scene is run in -- and `seed`
    is ignored."""
    if scene_seeds is not None:
        scene_seeds = scene_seed_tensor(scene_seeds, boxes, "sample_points_in_boxes")
    boxes, pc = _boxes_and_points(boxes, pc, "sample_points_in_boxes")
    b, r, _ = boxes.shape
    if scene_seeds is None:
        entry, seeds = L.lib().gspn_sample_points_in_boxes, seed_tensor(seed, boxes.device)
    else:
        entry, seeds = L.lib().gspn_sample_points_in_boxes_seeds, scene_seeds
    out = torch.empty((b, r, int(nsmp)), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        L.check(entry(b, r, pc.shape[1], int(nsmp), float(margin), L.ptr(seeds), L.ptr(boxes), L.ptr(pc), L.ptr(out), L.stream()),
                "sample_points_in_boxes")
    return out


def detection_target_select(proposals, count, gt_class_ids, gt_boxes, rois_per_image, positive_ratio, seed):
    """The decisions of detection_target_gen (:662-720) for the whole batch.  proposals (B, S, 6), count (B, S) int32 (box_point_count,
    margin 0), gt_class_ids (B, G), gt_boxes (B, G, 6) -> roi_src, roi_gt (B, rois_per_image) int32: the source proposal of each ROI row
    (-1: padding) and its ground-truth box in untrimmed numbering (-1: negative or padding).  Positives first, then negatives, then
    padding; see gspn_detection_target_select in include/gspn_hip.h.  S <= 1024."""
    proposals = L.need(proposals.detach(), torch.float32, 3, "proposals")
    gt_boxes = L.need(gt_boxes.detach(), torch.float32, 3, "gt_boxes")
    count = L.need(count, torch.int32, 2, "count")
    gt_cls = L.need(gt_class_ids.detach().float(), torch.float32, 2, "gt_class_ids")
    b, s, _ = proposals.shape
    g = gt_boxes.shape[1]
    if proposals.shape[2] != 6 or tuple(gt_boxes.shape) != (b, g, 6) or tuple(count.shape) != (b, s) or tuple(gt_cls.shape) != (b, g):
        raise ValueError("detection_target_select: expected proposals (B, S, 6), count (B, S), gt classes (B, G), gt boxes (B, G, 6)")
    r = int(rois_per_image)
    max_positive = int(r * positive_ratio)                                                      # :700-701
    inv_ratio = float(torch.tensor(1.0 / positive_ratio, dtype=torch.float32))                  # :705, the constant TF rounds to fp32
    seed = seed_tensor(seed, proposals.device)
    roi_src = torch.empty((b, r), dtype=torch.int32, device=proposals.device)
    roi_gt = torch.empty((b, r), dtype=torch.int32, device=proposals.device)
    with torch.cuda.device(proposals.device):
        L.check(L.lib().gspn_detection_target_select(b, s, g, r, max_positive, inv_ratio, L.ptr(seed), L.ptr(proposals), L.ptr(count), L.ptr(gt_cls),
                                                     L.ptr(gt_boxes), L.ptr(roi_src), L.ptr(roi_gt), L.stream()), "detection_target_select")
    return roi_src, roi_gt


def box_refinement(box, gt_box):
    """:553-568.  box, gt_box (..., 6) -> (..., 6) in the reference's [dz, dy, dx, dh, dw, dl] order."""
    box, gt_box = box.float(), gt_box.float()
    size = box[..., 3:] + 1e-8
    d = (gt_box[..., :3] - box[..., :3]) / size
    s = torch.log(gt_box[..., 3:] / size)
    return torch.cat((d.flip(-1), s.flip(-1)), -1)


def apply_box_delta(box, delta):
    """:570-582.  box, delta (..., 6), delta in box_refinement's order -> refined box (..., 6)."""
    delta = torch.cat((delta[..., :3].flip(-1), delta[..., 3:].flip(-1)), -1)
    return torch.cat((delta[..., :3] * box[..., 3:] + box[..., :3], torch.exp(delta[..., 3:]) * box[..., 3:]), -1)


_constants = {}


def _constant(values, device):
    """a small fp32 constant on the device, copied there once (a host-to-device copy has no place inside a captured step)"""
    key = (tuple(float(v) for v in values), device)
    if key not in _constants:
        _constants[key] = torch.tensor(key[0], dtype=torch.float32, device=device)
    return _constants[key]


def _take_rows(source, idx):
    """source (B, S, ...) gathered by idx (B, R) with -1 for "nothing" (rows of zeros there)"""
    i = idx.long().clamp(min=0)
    i = i.reshape(i.shape + (1,) * (source.dim() - 2)).expand(i.shape + tuple(source.shape[2:]))
    keep = (idx >= 0).reshape(idx.shape + (1,) * (source.dim() - 2))
    picked = torch.gather(source, 1, i)
    return torch.where(keep, picked, torch.zeros((), dtype=source.dtype, device=source.device))


def _detection_targets(spn_rois, gt_class_ids, gt_boxes, pc, config, seed):
    """what both forms of detection_target_gen share: everything but the mask look-up"""
    seed = seed_tensor(seed, spn_rois.device)
    count = box_point_count(spn_rois, pc)
    roi_src, roi_gt = detection_target_select(spn_rois, count, gt_class_ids, gt_boxes, config.TRAIN_ROIS_PER_IMAGE, config.ROI_POSITIVE_RATIO, seed)
    positive = roi_gt >= 0
    rois = _take_rows(spn_rois.detach(), roi_src)
    target_class_ids = _take_rows(gt_class_ids, roi_gt)
    roi_gt_boxes = _take_rows(gt_boxes, roi_gt)
    std = _constant(config.BBOX_STD_DEV, rois.device)
    ones = torch.ones((), dtype=torch.float32, device=rois.device)
    pos3 = positive.unsqueeze(-1)
    # the rows that are not positive go through box_refinement as unit boxes (no log of 0) and come out as zeros, the reference's padding
    target_bbox = torch.where(pos3, box_refinement(torch.where(pos3, rois, ones), torch.where(pos3, roi_gt_boxes, ones)) / std,
                              torch.zeros((), dtype=torch.float32, device=rois.device))
    positive_rois = torch.where(pos3, rois, torch.zeros((), dtype=torch.float32, device=rois.device))
    idx = sample_points_in_boxes(positive_rois, pc, config.NUM_POINT_INS_MASK, seed)         # all-zero boxes: rows of zeros
    return rois, target_class_ids, target_bbox, idx, roi_gt, positive


def detection_target_gen_batch(spn_rois, gt_class_ids, gt_boxes, group_label, pc, config, seed=0):
    """:647-747 for the whole batch (the reference's batch_slice, :1090-1094), with group_label (B, N) in place of its one-hot.
    spn_rois (B, S, 6) zero padded, gt_class_ids (B, G), gt_boxes (B, G, 6) zero padded, pc (B, N, 3) ->
      rois (B, R, 6), target_class_ids (B, R) (gt_class_ids' dtype), target_bbox (B, R, 6), target_mask_selection_idx (B, R, P) int32,
      target_mask (B, R, P) bool, R = TRAIN_ROIS_PER_IMAGE, P = NUM_POINT_INS_MASK; positives first, then negatives, then padding.
    Rows of negatives and padding are zero in the last three and in target_class_ids, padding rows in rois too.
    target_mask = group_label[idx] == roi_gt: column roi_gt of the one-hot, which is never built (a sampled point is inside its ROI, so
    the reference's `and positive_roi_masks`, :729, changes nothing)."""
    rois, target_class_ids, target_bbox, idx, roi_gt, positive = _detection_targets(spn_rois, gt_class_ids, gt_boxes, pc, config, seed)
    b, r, p = idx.shape
    labels = torch.gather(group_label, 1, idx.reshape(b, r * p).long()).reshape(b, r, p)
    target_mask = (labels == roi_gt.unsqueeze(-1).to(labels.dtype)) & positive.unsqueeze(-1)
    return rois, target_class_ids, target_bbox, idx, target_mask


def detection_target_gen(proposals, gt_class_ids, gt_boxes, gt_masks, pc, config, seed=0):
    """:647-747 with the reference's per-scene signature: proposals (S, 6), gt_class_ids (G,), gt_boxes (G, 6), gt_masks (N, G), pc (N, 3).
    A thin wrapper of the batch form; gt_masks is a general matrix here, so the mask is looked up as gt_masks[idx, roi_gt]."""
    rois, target_class_ids, target_bbox, idx, roi_gt, positive = _detection_targets(
        proposals.unsqueeze(0), gt_class_ids.unsqueeze(0), gt_boxes.unsqueeze(0), pc.unsqueeze(0), config, seed)
    masks = gt_masks[idx[0].long(), roi_gt[0].long().clamp(min=0).unsqueeze(-1)].bool() & positive[0].unsqueeze(-1)
    return rois[0], target_class_ids[0], target_bbox[0], idx[0], masks


def mask_selection_gen_batch(proposals, pc, num_rois, config, empty_removal=True, seed=0, scene_seeds=None):
    """:749-783 for the whole batch.  proposals (B, S, 6) zero padded, pc (B, N, 3) -> rois (B, num_rois, 6), mask_selection_idx
    (B, num_rois, NUM_POINT_INS_MASK) int32.  The kept rows -- not all-zero and, with empty_removal, holding a point within the 1e-3
    margin -- move to the front in their original order (a prefix sum and a scatter on (B, S), no nonzero), then nsmp points are drawn
    inside each with the same margin.  Rows past num_rois are dropped (the reference would return a longer tensor).
    scene_seeds: as in sample_points_in_boxes -- a seed per scene, `seed` ignored."""
    if scene_seeds is not None:
        scene_seeds = scene_seed_tensor(scene_seeds, proposals, "mask_selection_gen")
    proposals, pc = _boxes_and_points(proposals, pc, "mask_selection_gen")
    b, s, _ = proposals.shape
    num_rois = int(num_rois)
    keep = proposals.abs().sum(-1) != 0                                                   # trim_zeros_graph, :491
    if empty_removal:
        keep = keep & (box_point_count(proposals, pc, MASK_SELECTION_MARGIN) > 0)
    dest = torch.where(keep, torch.cumsum(keep.long(), 1) - 1, torch.full((), s, dtype=torch.int64, device=keep.device))
    src = torch.full((b, s + 1), -1, dtype=torch.int64, device=keep.device)
    src.scatter_(1, dest, torch.arange(s, device=keep.device).expand(b, s))               # the rows not kept all land in column s
    src = src[:, :min(s, num_rois)]
    if num_rois > s:
        src = torch.nn.functional.pad(src, (0, num_rois - s), value=-1)
    rois = _take_rows(proposals, src)
    idx = sample_points_in_boxes(rois, pc, config.NUM_POINT_INS_MASK, seed, MASK_SELECTION_MARGIN, scene_seeds)
    return rois, idx


def mask_selection_gen(proposals, pc, num_rois, config, empty_removal=True, seed=0):
    """:749-783 with the reference's per-scene signature: proposals (S, 6), pc (N, 3)."""
    rois, idx = mask_selection_gen_batch(proposals.unsqueeze(0), pc.unsqueeze(0), num_rois, config, empty_removal, seed)
    return rois[0], idx[0]


class _Lists:
    """the inverse lists of one index tensor, built on first use and shared by the gradients of everything gathered through it"""

    def __init__(self, idx, n):
        self.idx, self.n, self.lists = idx, n, None

    def get(self):
        if self.lists is None:
            self.lists = invlists.inverse_lists(self.idx.reshape(self.idx.shape[0], -1), self.n)
        return self.lists


def _crop_gather_grad(lists, grad_out):
    """grad_out (B, R, P, c) gathered through lists.idx (B, R, P) -> (B, n, c): the sum over the positions that name each point, in the
    fixed order of gspn_crop_gather_grad"""
    b, m, ns, c = grad_out.shape
    grad_out = grad_out.contiguous()
    order, offsets = lists.get()
    n, idx = lists.n, lists.idx
    g = torch.empty((b, n, c), dtype=torch.float32, device=grad_out.device)
    part = torch.empty(int(L.lib().gspn_crop_gather_grad_part_floats(b, m * ns, c)), dtype=torch.float32, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        L.check(L.lib().gspn_crop_gather_grad(b, n, c, m * ns, L.ptr(idx), L.ptr(order), L.ptr(offsets), L.ptr(grad_out), L.ptr(part), L.ptr(g),
                                              L.stream()), "points_cropping(grad)")
    return g


class _CropGather(torch.autograd.Function):
    """group_point whose gradient is gspn_crop_gather_grad at EVERY width: a fixed summation order (tf_grouping.group_point takes the atomic
    scatter-add below 16 channels), and the list of point 0 -- which the rows of zeros of negative and padding ROIs all name -- spread
    over the chip instead of walked by one wave"""

    @staticmethod
    def forward(ctx, points, idx, lists):
        ctx.lists = lists
        ctx.save_for_backward(idx)           # backward reads it again through `lists` (and builds the inverse lists from it on first use)
        return group_point(points, idx)

    @staticmethod
    def backward(ctx, grad_out):
        ctx.saved_tensors                    # raises if idx was modified in place since the forward pass
        return _crop_gather_grad(ctx.lists, grad_out), None, None


def points_cropping(pc, pc_fea, pc_center, rois, masks_selection_idx, num_rois, num_point_per_roi, normalize_crop_region=True):
    """:785-816.  pc (B, N, 3), pc_fea (B, N, C), pc_center (B, N, 3), rois (B, R, 6) zero padded, masks_selection_idx (B, R, P) int32 ->
    pc_fea_cropped (B, R, P, C), pc_center_cropped, pc_coord_cropped, pc_coord_cropped_unnormalized (B, R, P, 3): the three gathers, minus
    the ROI centre, divided by the ROI size (all-zero ROI rows turned into ones first, :812).  The gathers are group_point; their gradients
    are sums in a fixed order through ONE set of inverse lists (gspn_crop_gather_grad), so they are the same bits on every call."""
    idx = L.need(masks_selection_idx, torch.int32, 3, "masks_selection_idx")
    pc = L.need(pc, torch.float32, 3, "pc")
    pc_fea = L.need(pc_fea, torch.float32, 3, "pc_fea")
    pc_center = L.need(pc_center, torch.float32, 3, "pc_center")
    b, n, _ = pc.shape
    if tuple(idx.shape) != (b, int(num_rois), int(num_point_per_roi)) or tuple(rois.shape) != (b, int(num_rois), 6):
        raise ValueError("points_cropping: expected masks_selection_idx (B, %d, %d) and rois (B, %d, 6), got %s and %s"
                         % (num_rois, num_point_per_roi, num_rois, tuple(idx.shape), tuple(rois.shape)))
    if pc_fea.shape[:2] != pc.shape[:2] or pc_center.shape[:2] != pc.shape[:2]:
        raise ValueError("points_cropping: pc, pc_fea and pc_center must share (B, N)")
    lists = _Lists(idx, n)
    pc_fea_cropped = _CropGather.apply(pc_fea, idx, lists)
    pc_center_cropped = _CropGather.apply(pc_center, idx, lists)
    pc_coord_cropped_unnormalized = _CropGather.apply(pc, idx, lists)
    rois_center = rois[:, :, :3].unsqueeze(2)
    pc_coord_cropped = pc_coord_cropped_unnormalized - rois_center
    pc_center_cropped = pc_center_cropped - rois_center
    if normalize_crop_region:
        rois = rois + (rois.sum(2, keepdim=True) == 0).float()
        rois_size = rois[:, :, 3:].unsqueeze(2)
        pc_coord_cropped = pc_coord_cropped / rois_size
        pc_center_cropped = pc_center_cropped / rois_size
    return pc_fea_cropped, pc_center_cropped, pc_coord_cropped, pc_coord_cropped_unnormalized
