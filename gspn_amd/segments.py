"""Segment voting (ours: the reference stops at the network's points): a scan's per-vertex masks and labels snapped to the
segments of its mesh's over-segmentation, the `segIndices` ScanNet's ground truth is built from.  The vertices of a segment vote and the
whole segment takes the majority's value: a mask row sets segment g iff float64(set vertices of g) > vote_th * float64(vertices of g), one
double multiply and a strict compare; a label row takes the most frequent label in [0, C), the lowest among equal counts.  A vertex whose
segment id is outside [0, S) is unsegmented: it does not vote and keeps its own value.  With one vertex per segment both are the identity
(on masks: the normalisation of a nonzero byte to 1).  gspn_segment_vote / gspn_segment_label_vote (csrc/segments.hip): integer counts and
integer atomics only, the same bits on every call.  No CPU fallback."""
import torch

from . import _lib as L
from ._args import _on_device, _out_like, _typed, _workspace, _ws_typed

__all__ = ["SEGMENT_MAX_V", "SEGMENT_MAX_S", "SEGMENT_MAX_R", "SEGMENT_MAX_COUNTERS", "compact_segments", "segment_vote", "segment_label_vote"]

SEGMENT_MAX_V = 1 << 24             # GSPN_SEGMENT_VOTE_MAX_V of include/gspn_hip.h
SEGMENT_MAX_S = 1 << 24             # GSPN_SEGMENT_VOTE_MAX_S
SEGMENT_MAX_R = 65535               # the rows are a grid dimension
SEGMENT_MAX_COUNTERS = 1 << 28      # GSPN_SEGMENT_VOTE_MAX_COUNTERS: (R + 1) * S, or S * C


def compact_segments(ids):
    """Raw segment ids (V,), any integer dtype, on any device (ScanNet's are sparse; data_prep allows up to 2^26) -> (seg (V,) int32 on the
    same device, S): the S different non-negative ids numbered 0..S-1 in ascending order of id, every negative id -1.  torch.unique
    with return_inverse, and S read back once: eager, once per scan, not meant for a captured region."""
    if not isinstance(ids, torch.Tensor):
        raise TypeError("ids must be a torch.Tensor")
    if ids.dim() != 1 or ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
        raise ValueError("compact_segments: ids must be a 1-D integer tensor, got %s %s" % (tuple(ids.shape), ids.dtype))
    ids = ids.detach().long()
    values, inverse = torch.unique(ids.clamp(min=-1), return_inverse=True)          # ascending; the negatives, if any, are values[0] == -1
    shift = (values[:1] < 0).long().sum() if values.numel() else torch.zeros((), dtype=torch.long, device=ids.device)
    s = int(values.numel() - shift)                                                 # the one read-back
    return (inverse - shift).int().contiguous(), s


def _vote_th(vote_th, what):
    vote_th = float(vote_th)
    if not 0.0 <= vote_th < 1.0:                                                    # a NaN fails both
        raise ValueError("%s: vote_th must lie in [0, 1), got %r" % (what, vote_th))
    return vote_th


def _count(n, what, name):
    n = int(n)
    if n < 0:
        raise ValueError("%s: %s must not be negative, got %d" % (what, name, n))
    return n


def segment_vote(masks, seg, num_segments, vote_th=0.5, out=None, ws=None):
    """masks (R, V) uint8, any nonzero byte set; seg (V,) int32, compact ids (compact_segments), a value outside [0, num_segments)
    unsegmented; vote_th a Python float (a double) in [0, 1); out: a (R, V) uint8 device tensor to write, masks itself allowed, or None;
    ws: a 16-byte aligned uint8 device tensor of at least gspn_segment_vote_ws_bytes(R, V, S) bytes (it need not be initialised; a caller
    that owns it can capture the call in a graph), or None -> out (R, V) uint8 of 0 and 1, mask_points (R,) int32: the set bytes of each
    row.  Raises ValueError for shapes, dtypes, an empty input, a vote_th outside [0, 1) or a short or misplaced ws, NotImplementedError
    for V or S > 2^24, R > 65535 or (R + 1) * S > 2^28, all before anything has run."""
    masks = _typed(masks, torch.uint8, 2, "masks")
    seg = _typed(seg, torch.int32, 1, "seg")
    r, v = masks.shape
    if tuple(seg.shape) != (v,):
        raise ValueError("segment_vote: expected masks (R, V) and seg (V,), got %s and %s" % (tuple(masks.shape), tuple(seg.shape)))
    if min(r, v) <= 0:
        raise ValueError("segment_vote: empty input, masks %s" % (tuple(masks.shape),))
    s = _count(num_segments, "segment_vote", "num_segments")
    vote_th = _vote_th(vote_th, "segment_vote")
    out = _out_like(out, (r, v), None, "segment_vote")
    ws = _ws_typed(ws)
    if v > SEGMENT_MAX_V or s > SEGMENT_MAX_S or r > SEGMENT_MAX_R or (r + 1) * s > SEGMENT_MAX_COUNTERS:
        raise NotImplementedError("segment_vote: V <= %d, S <= %d, R <= %d and (R + 1) * S <= %d (got %d, %d and %d)"
                                  % (SEGMENT_MAX_V, SEGMENT_MAX_S, SEGMENT_MAX_R, SEGMENT_MAX_COUNTERS, v, s, r))
    masks, seg = _on_device(masks=masks, seg=seg)
    dev = masks.device
    out = _out_like(out, (r, v), dev, "segment_vote")
    ws = _workspace(ws, int(L.lib().gspn_segment_vote_ws_bytes(r, v, s)), dev, "segment_vote")
    mask_points = torch.empty((r,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_segment_vote(r, v, s, L.ptr(masks), L.ptr(seg), vote_th, L.ptr(ws), L.ptr(out), L.ptr(mask_points), L.stream()),
                "segment_vote")
    return out, mask_points


def segment_label_vote(labels, seg, num_segments, num_classes, ws=None):
    """labels (V,) int32; seg (V,) int32 as in segment_vote; ws: at least gspn_segment_label_vote_ws_bytes(V, S, C) bytes, or None
    -> (V,) int32: the label in [0, num_classes) that most vertices of the vertex's segment hold, the lowest among equal counts; a label
    outside [0, num_classes) does not vote; an unsegmented vertex, or one in a segment where nobody voted, keeps its own label.  Raises as
    segment_vote does; NotImplementedError for V or S > 2^24 or S * C > 2^28."""
    labels = _typed(labels, torch.int32, 1, "labels")
    seg = _typed(seg, torch.int32, 1, "seg")
    v = labels.shape[0]
    if tuple(seg.shape) != (v,):
        raise ValueError("segment_label_vote: expected labels (V,) and seg (V,), got %s and %s" % (tuple(labels.shape), tuple(seg.shape)))
    if v <= 0:
        raise ValueError("segment_label_vote: empty input, labels %s" % (tuple(labels.shape),))
    s = _count(num_segments, "segment_label_vote", "num_segments")
    c = int(num_classes)
    if c < 1:
        raise ValueError("segment_label_vote: num_classes must be positive, got %d" % c)
    ws = _ws_typed(ws)
    if v > SEGMENT_MAX_V or s > SEGMENT_MAX_S or s * c > SEGMENT_MAX_COUNTERS:
        raise NotImplementedError("segment_label_vote: V <= %d, S <= %d and S * C <= %d (got %d, %d and C = %d)"
                                  % (SEGMENT_MAX_V, SEGMENT_MAX_S, SEGMENT_MAX_COUNTERS, v, s, c))
    labels, seg = _on_device(labels=labels, seg=seg)
    dev = labels.device
    ws = _workspace(ws, int(L.lib().gspn_segment_label_vote_ws_bytes(v, s, c)), dev, "segment_label_vote")
    out = torch.empty((v,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_segment_label_vote(v, s, c, L.ptr(labels), L.ptr(seg), L.ptr(ws), L.ptr(out), L.stream()), "segment_label_vote")
    return out
