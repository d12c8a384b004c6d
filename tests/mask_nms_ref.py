"""numpy restatement of mask NMS (gspn_amd/mask_nms.py): int64 counts, and the same double compare as the kernel --
float64(inter) > iou_th * float64(union), one multiply, strict.  Test infrastructure only."""
import numpy as np


def mask_overlaps_ref(masks):
    """masks (R, V), any nonzero byte set -> sizes (R,) int32, inter (R, R) int32 (counted in int64)"""
    m = (np.asarray(masks) != 0).astype(np.int64)
    inter = m @ m.T
    return np.diagonal(inter).astype(np.int32), inter.astype(np.int32)


def greedy_ref(sizes, inter, count=None, labels=None, iou_th=0.5):
    """the walk alone -> suppressed (R,) bool, live"""
    r = len(sizes)
    live = r if count is None else min(max(int(count), 0), r)
    th = np.float64(iou_th)
    sizes, inter = np.asarray(sizes, np.int64), np.asarray(inter, np.int64)
    supp = np.zeros(r, bool)
    for k in range(1, live):
        n = inter[:k, k]                                              # against every earlier row at once: the same compare, row by row
        above = n.astype(np.float64) > th * (sizes[:k] + sizes[k] - n).astype(np.float64)
        same = np.ones(k, bool) if labels is None else np.asarray(labels[:k]) == labels[k]
        supp[k] = bool((above & same & ~supp[:k]).any())
    return supp, live


def mask_nms_ref(masks, count=None, labels=None, iou_th=0.5):
    """one scene: masks (R, V) -> out (R, V) uint8, keep (R,) uint8, mask_points (R,) int32"""
    masks = np.asarray(masks)
    sizes, inter = mask_overlaps_ref(masks)
    supp, live = greedy_ref(sizes.astype(np.int64), inter.astype(np.int64), count, labels, iou_th)
    out = (masks != 0).astype(np.uint8)
    out[supp] = 0
    keep = np.zeros(masks.shape[0], np.uint8)
    keep[:live] = ~supp[:live]
    return out, keep, out.sum(1, dtype=np.int64).astype(np.int32)


def mask_nms_batch_ref(masks, count=None, labels=None, iou_th=0.5):
    """(B, R, V) with count (B,) and labels (B, R), either None -> the three outputs stacked"""
    parts = [mask_nms_ref(masks[s], None if count is None else count[s], None if labels is None else labels[s], iou_th) for s in range(len(masks))]
    return tuple(np.stack(p) for p in zip(*parts))
