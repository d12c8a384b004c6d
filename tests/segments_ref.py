"""The numpy restatement of DESIGN.md 4.23 (segment voting), in loops and np.bincount: what tests/test_cpu_segments.py pins on a
hand-written case and tests/test_gpu_*segments.py compare gspn_amd.segments against, bit for bit.  A plain module: no conftest, no plugin."""
import numpy as np


def segment_vote_ref(masks, seg, num_segments, vote_th=0.5):
    """masks (R, V) uint8, seg (V,) integers, S -> out (R, V) uint8 of 0 and 1, mask_points (R,) int32"""
    masks = np.asarray(masks)
    seg = np.asarray(seg).astype(np.int64)
    r, v = masks.shape
    s = int(num_segments)
    inside = (seg >= 0) & (seg < s)                                   # an id outside [0, S) never indexes anything
    ids = seg[inside]
    size = np.bincount(ids, minlength=s)[:s] if s else np.zeros(0, np.int64)
    out = np.zeros((r, v), np.uint8)
    for k in range(r):
        own = masks[k] != 0
        cnt = np.bincount(ids[own[inside]], minlength=s)[:s] if s else np.zeros(0, np.int64)
        bit = np.zeros(s, bool)
        for g in range(s):
            bit[g] = np.float64(cnt[g]) > np.float64(vote_th) * np.float64(size[g])          # one double multiply, a strict compare
        row = own.copy()                                              # an unsegmented vertex keeps its own byte, as 0 or 1
        row[inside] = bit[ids]
        out[k] = row
    return out, out.sum(1).astype(np.int32)


def segment_label_vote_ref(labels, seg, num_segments, num_classes):
    """labels (V,) integers, seg (V,) integers, S, C -> (V,) int32"""
    labels = np.asarray(labels).astype(np.int64)
    seg = np.asarray(seg).astype(np.int64)
    s, c = int(num_segments), int(num_classes)
    inside = (seg >= 0) & (seg < s)
    votes = inside & (labels >= 0) & (labels < c)                     # a label outside [0, C) does not vote
    cnt = np.bincount(seg[votes] * c + labels[votes], minlength=s * c)[:s * c].reshape(s, c)
    out = labels.copy()
    for i in range(labels.shape[0]):
        if inside[i]:
            row = cnt[seg[i]]
            if row.max() > 0:
                out[i] = int(np.argmax(row))                          # the first maximum: the lowest label among equal counts
    return out.astype(np.int32)


def fast_segment_vote_ref(masks, seg, num_segments, vote_th=0.5):
    """segment_vote_ref without the loop over the segments (the same float64 multiply and compare, elementwise), for the larger cases"""
    masks = np.asarray(masks)
    seg = np.asarray(seg).astype(np.int64)
    r, v = masks.shape
    s = int(num_segments)
    inside = (seg >= 0) & (seg < s)
    ids = seg[inside]
    size = np.bincount(ids, minlength=s)[:s].astype(np.float64) if s else np.zeros(0, np.float64)
    out = np.zeros((r, v), np.uint8)
    for k in range(r):
        own = masks[k] != 0
        if not own.any():
            continue
        cnt = np.bincount(ids[own[inside]], minlength=s)[:s].astype(np.float64) if s else np.zeros(0, np.float64)
        bit = cnt > np.float64(vote_th) * size
        row = own.copy()
        row[inside] = bit[ids]
        out[k] = row
    return out, out.sum(1).astype(np.int32)
