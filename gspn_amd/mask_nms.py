"""Mask NMS (ours: the reference stops at the network's points and removes duplicates on boxes alone): duplicate instance
masks suppressed by pairwise IoU.  A scene is R mask rows of V bytes in priority order, row 0 the best, any nonzero byte set.  With size[k]
the set bytes of row k and inter[i][j] the vertices set in both rows, row k of the first `count` rows is suppressed iff an earlier KEPT row
i with the same label (or any earlier kept row, without labels) has float64(inter[i][k]) > iou_th * float64(size[i] + size[k] - inter[i][k]):
one double multiply and a strict compare.  A suppressed row suppresses nobody and comes out all zero, with mask_points 0, so the writer and
the AP counts pass it over; every shape stays static.  gspn_mask_overlaps / gspn_mask_nms (csrc/mask_nms.hip): the bytes packed to 64-bit
words, a popcount Gram over them, integer atomics only, the same bits on every call.  No CPU fallback."""
import torch

from . import _lib as L
from ._args import _on_device, _out_like, _typed, _workspace, _ws_typed

__all__ = ["MASK_NMS_MAX_R", "MASK_NMS_MAX_V", "MASK_NMS_MAX_B", "mask_overlaps", "mask_nms"]

MASK_NMS_MAX_R = 1024               # GSPN_MASK_NMS_MAX_R of include/gspn_hip.h: scene_rank's limit
MASK_NMS_MAX_V = 1 << 24            # GSPN_MASK_NMS_MAX_V
MASK_NMS_MAX_B = 65535              # GSPN_MASK_NMS_MAX_B: the scenes are a grid dimension


def _iou_th(iou_th, what):
    iou_th = float(iou_th)
    if not 0.0 <= iou_th < 1.0:                                                     # a NaN fails both
        raise ValueError("%s: iou_th must lie in [0, 1), got %r" % (what, iou_th))
    return iou_th


def _scenes(masks, what):
    """masks (R, V) or (B, R, V) uint8 -> the 3-D view and whether a scene axis was added; ValueError for anything else or an empty input"""
    if not isinstance(masks, torch.Tensor):
        raise TypeError("masks must be a torch.Tensor")
    if masks.dim() not in (2, 3):
        raise ValueError("%s: masks must be (R, V) or (B, R, V), got shape %s" % (what, tuple(masks.shape)))
    single = masks.dim() == 2
    masks = _typed(masks, torch.uint8, None, "masks")
    if min(masks.shape) <= 0:
        raise ValueError("%s: empty input, masks %s" % (what, tuple(masks.shape)))
    return (masks.unsqueeze(0) if single else masks), single


def _limits(b, r, v, what):
    if r > MASK_NMS_MAX_R or v > MASK_NMS_MAX_V or b > MASK_NMS_MAX_B:
        raise NotImplementedError("%s: R <= %d, V <= %d and B <= %d (got %d, %d and %d)" % (what, MASK_NMS_MAX_R, MASK_NMS_MAX_V, MASK_NMS_MAX_B, r, v, b))


def mask_overlaps(masks, ws=None):
    """masks (R, V) or (B, R, V) uint8, any nonzero byte set; ws: a 16-byte aligned uint8 device tensor of at least
    gspn_mask_overlaps_ws_bytes(B, R, V) bytes (it need not be initialised; a caller that owns it can capture the call in a graph), or None
    -> sizes (R,) or (B, R) int32: the set bytes of each row; inter (R, R) or (B, R, R) int32: the vertices set in both rows, symmetric,
    sizes on its diagonal.  Raises ValueError for shapes, dtypes, an empty input or a short or misplaced ws, NotImplementedError for
    R > 1024, V > 2^24 or B > 65535, all before anything has run."""
    masks, single = _scenes(masks, "mask_overlaps")
    b, r, v = masks.shape
    ws = _ws_typed(ws)
    _limits(b, r, v, "mask_overlaps")
    masks, = _on_device(masks=masks)
    dev = masks.device
    ws = _workspace(ws, int(L.lib().gspn_mask_overlaps_ws_bytes(b, r, v)), dev, "mask_overlaps")
    sizes = torch.empty((b, r), dtype=torch.int32, device=dev)
    inter = torch.empty((b, r, r), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_mask_overlaps(b, r, v, L.ptr(masks), L.ptr(ws), L.ptr(sizes), L.ptr(inter), L.stream()), "mask_overlaps")
    return (sizes[0], inter[0]) if single else (sizes, inter)


def mask_nms(masks, count=None, labels=None, *, iou_th, out=None, ws=None):
    """masks (R, V) or (B, R, V) uint8 in priority order, row 0 the best; count: the live leading rows, a () or (B,) int32 device tensor
    (scene_rank's, as it is: nothing is read back) or None for all rows; labels (R,) or (B, R) int32, or None: with labels only rows of
    equal label suppress each other; iou_th: a Python float (a double) in [0, 1), no default; out: a uint8 device tensor shaped like
    masks, masks itself allowed, or None; ws: at least gspn_mask_nms_ws_bytes(B, R, V) bytes, or None
    -> out like masks, 0 and 1, a suppressed row all zero, every other row (those at or beyond count too) the normalised input;
       keep (R,) or (B, R) uint8: 1 for a kept live row, 0 for a suppressed one and for a row at or beyond count;
       mask_points (R,) or (B, R) int32: the set bytes of each row of out.
    Raises as mask_overlaps does, and ValueError for an iou_th outside [0, 1)."""
    masks, single = _scenes(masks, "mask_nms")
    b, r, v = masks.shape
    lead = () if single else (b,)
    if count is not None:
        count = _typed(count, torch.int32, len(lead), "count")
        if tuple(count.shape) != lead:
            raise ValueError("mask_nms: count must be %s, one per scene, got %s" % (lead, tuple(count.shape)))
        count = count.reshape(b)
    if labels is not None:
        labels = _typed(labels, torch.int32, len(lead) + 1, "labels")
        if tuple(labels.shape) != lead + (r,):
            raise ValueError("mask_nms: labels must be %s, one per row, got %s" % (lead + (r,), tuple(labels.shape)))
        labels = labels.reshape(b, r)
    iou_th = _iou_th(iou_th, "mask_nms")
    out = _out_like(out, lead + (r, v), None, "mask_nms")
    ws = _ws_typed(ws)
    _limits(b, r, v, "mask_nms")
    masks, = _on_device(masks=masks)
    dev = masks.device
    if count is None:
        count = torch.full((b,), r, dtype=torch.int32, device=dev)
    else:
        count, = _on_device(count=count)
    if labels is not None:
        labels, = _on_device(labels=labels)
    out = _out_like(out, lead + (r, v), dev, "mask_nms")
    ws = _workspace(ws, int(L.lib().gspn_mask_nms_ws_bytes(b, r, v)), dev, "mask_nms")
    keep = torch.empty(lead + (r,), dtype=torch.uint8, device=dev)
    mask_points = torch.empty(lead + (r,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_mask_nms(b, r, v, L.ptr(masks), L.ptr(count), L.ptr(labels), iou_th, L.ptr(ws),
                                      L.ptr(out), L.ptr(keep), L.ptr(mask_points), L.stream()), "mask_nms")
    return out, keep, mask_points
