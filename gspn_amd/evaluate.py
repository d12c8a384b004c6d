"""Instance AP evaluation: what the ScanNet benchmark's evaluate_semantic_instance step (the step the reference runs after test.py:221-222)
computes from the files of write_predictions / write_ground_truth, or from scene_predictions' tensors before they are written, on the HIP
kernels of csrc/evaluate.hip.  The definition is DESIGN.md 4.18.

The only large part of the metric is the overlap counting: R x G intersections of N-point masks per scene.  gspn_instance_overlaps counts them
from the (B, R, N) uint8 masks scene_predictions leaves on the device; gspn_instance_match runs the greedy matching per (scene, threshold,
class) and leaves, per prediction row, how many (true, confidence) and (false, confidence) records it contributes.  Those are small static-shape
integer tensors: InstanceAP keeps them on the device, batch after batch, and reads nothing back until compute(), which makes one transfer and
runs the precision / recall curve in float64 numpy.

instance_overlaps and instance_match run under torch.no_grad(); every shape is static and nothing reads a value back to the host, so they
capture in a graph.CapturedStep behind scene_predictions.  The readers and write_result_file are host IO in plain Python.  No CPU fallback for
the compute."""
import os
import warnings

import numpy as np
import torch

from . import _lib as L
from ._args import _on_device, _typed
from .predict import SCANNET_LABEL_MAP

__all__ = ["DEFAULT_OVERLAPS", "MIN_REGION_SIZE", "INSTANCE_MAX_G", "INSTANCE_MAX_CG", "INSTANCE_MATCH_MAX_R", "SCANNET_CLASS_NAMES",
           "instance_overlaps", "instance_match", "classes_from_label_ids", "InstanceAP", "average_precision", "read_predictions",
           "read_ground_truth", "evaluate_files", "write_result_file"]

DEFAULT_OVERLAPS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)          # the benchmark's thresholds, float64, built by its own expression
MIN_REGION_SIZE = 100
INSTANCE_MAX_G = 4096         # GSPN_INSTANCE_MAX_G of include/gspn_hip.h: one LDS bin per group
INSTANCE_MAX_CG = 8192        # GSPN_INSTANCE_MAX_CG: one LDS bin per (class, group)
INSTANCE_MATCH_MAX_R = 1024   # GSPN_INSTANCE_MATCH_MAX_R: the per-row state of one (scene, threshold, class) sits in LDS
SCANNET_CLASS_NAMES = ("cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter", "desk", "curtain",
                       "refrigerator", "shower curtain", "toilet", "sink", "bathtub", "otherfurniture")          # classes 1..18 of SCANNET_LABEL_MAP

_tables = {}


def _cached(kind, values, device, make):
    """a small constant as a device tensor, copied there once (a host-to-device copy has no place inside a captured step)"""
    key = (kind, values, device)
    if key not in _tables:
        _tables[key] = make()
    return _tables[key]


def _threshold_tensor(thresholds, device):
    values = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if values.size == 0 or np.isnan(values).any():
        raise ValueError("thresholds must be a non-empty sequence without NaN, got %r" % (thresholds,))
    return _cached("th", values.tobytes(), device, lambda: torch.from_numpy(values.copy()).to(device))


def instance_overlaps(masks, pred_class, seg_label, group_label, num_class, ngroup):
    """The counts of the metric for every prediction row of every scene.  masks (B, R, N) uint8 (a byte that is not 0 is a set point),
    pred_class (B, R) int32, seg_label, group_label (B, N) int32, num_class = C and ngroup = G Python integers
    -> inter (B, R, G), void_count (B, R), pred_count (B, R), gt_count (B, C, G), all int32.  A point is void when its seg label is outside
    [1, C) or its group label outside [0, G).  For a row k of class s in [1, C): inter[k, g] = its set points with seg == s and group == g,
    void_count[k] = its set points that are void, pred_count[k] = its set points; a row of another class gets zeros.  gt_count[s, g] = the
    scene's points that are not void with seg == s and group == g.  masks may be any view with contiguous strides: its rows need no alignment.
    Raises NotImplementedError for G > 4096 or C * G > 8192, before anything has run."""
    masks = _typed(masks, torch.uint8, 3, "masks")
    pred_class = _typed(pred_class, torch.int32, 2, "pred_class")
    seg_label = _typed(seg_label, torch.int32, 2, "seg_label")
    group_label = _typed(group_label, torch.int32, 2, "group_label")
    b, r, n = masks.shape
    if tuple(pred_class.shape) != (b, r) or tuple(seg_label.shape) != (b, n) or tuple(group_label.shape) != (b, n):
        raise ValueError("instance_overlaps: expected masks (B, R, N), pred_class (B, R), seg_label and group_label (B, N), got %s, %s, %s and %s"
                         % (tuple(masks.shape), tuple(pred_class.shape), tuple(seg_label.shape), tuple(group_label.shape)))
    c, g = int(num_class), int(ngroup)
    if min(b, r, n) <= 0 or c <= 0 or g <= 0:
        raise ValueError("instance_overlaps: empty input, masks %s, num_class %d, ngroup %d" % (tuple(masks.shape), c, g))
    if g > INSTANCE_MAX_G or c * g > INSTANCE_MAX_CG:
        raise NotImplementedError("instance_overlaps: ngroup <= %d and num_class * ngroup <= %d (got %d and %d)"
                                  % (INSTANCE_MAX_G, INSTANCE_MAX_CG, g, c * g))
    masks, pred_class, seg_label, group_label = _on_device(masks=masks, pred_class=pred_class, seg_label=seg_label, group_label=group_label)
    dev = masks.device
    with torch.no_grad():
        inter = torch.empty((b, r, g), dtype=torch.int32, device=dev)
        void_count = torch.empty((b, r), dtype=torch.int32, device=dev)
        pred_count = torch.empty((b, r), dtype=torch.int32, device=dev)
        gt_count = torch.empty((b, c, g), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().gspn_instance_overlaps(b, r, n, c, g, L.ptr(masks), L.ptr(pred_class), L.ptr(seg_label), L.ptr(group_label), L.ptr(inter),
                                                   L.ptr(void_count), L.ptr(pred_count), L.ptr(gt_count), L.stream()), "instance_overlaps")
    return inter, void_count, pred_count, gt_count


def instance_match(inter, void_count, pred_count, pred_class, confidence, count, gt_count, thresholds=DEFAULT_OVERLAPS,
                   min_region=MIN_REGION_SIZE):
    """The matching of DESIGN.md 4.18 for every (scene, threshold, class).  inter (B, R, G), void_count, pred_count (B, R), gt_count (B, C, G)
    int32: instance_overlaps'; pred_class (B, R) int32; confidence (B, R) float32; count (B,) int32: the rows k < count are a scene's
    predictions; thresholds: T doubles (a sequence, or a float64 device tensor); min_region a Python integer
    -> n_true, n_false (B, T, R) int32: the (true = 1, confidence[k]) and (true = 0, confidence[k]) records row k contributes at each threshold;
    hard_fn (B, T, C) int32: the eligible gts without a match; n_gt, n_pred (B, C) int32: the eligible gts and the valid rows of each class.
    Raises NotImplementedError for R > 1024 or min_region < 1, before anything has run."""
    inter = _typed(inter, torch.int32, 3, "inter")
    void_count = _typed(void_count, torch.int32, 2, "void_count")
    pred_count = _typed(pred_count, torch.int32, 2, "pred_count")
    pred_class = _typed(pred_class, torch.int32, 2, "pred_class")
    confidence = _typed(confidence, torch.float32, 2, "confidence")
    count = _typed(count, torch.int32, 1, "count")
    gt_count = _typed(gt_count, torch.int32, 3, "gt_count")
    b, r, g = inter.shape
    c = gt_count.shape[1]
    if (not (tuple(void_count.shape) == tuple(pred_count.shape) == tuple(pred_class.shape) == tuple(confidence.shape) == (b, r))
            or tuple(count.shape) != (b,) or tuple(gt_count.shape) != (b, c, g)):
        raise ValueError("instance_match: expected inter (B, R, G), void_count, pred_count, pred_class and confidence (B, R), count (B,) and "
                         "gt_count (B, C, G), got %s, %s, %s, %s, %s, %s and %s"
                         % tuple(tuple(t.shape) for t in (inter, void_count, pred_count, pred_class, confidence, count, gt_count)))
    if min(b, r, g, c) <= 0:
        raise ValueError("instance_match: empty input, inter %s, gt_count %s" % (tuple(inter.shape), tuple(gt_count.shape)))
    if isinstance(thresholds, torch.Tensor):
        thresholds = _typed(thresholds, torch.float64, 1, "thresholds")
        if thresholds.shape[0] <= 0:
            raise ValueError("instance_match: no threshold")
    else:
        np_thresholds = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        if np_thresholds.size == 0 or np.isnan(np_thresholds).any():
            raise ValueError("instance_match: thresholds must be a non-empty sequence without NaN, got %r" % (thresholds,))
    min_region = int(min_region)
    if r > INSTANCE_MATCH_MAX_R or min_region < 1:
        raise NotImplementedError("instance_match: R <= %d and min_region >= 1 (got %d and %d)" % (INSTANCE_MATCH_MAX_R, r, min_region))
    inter, void_count, pred_count, pred_class, confidence, count, gt_count = _on_device(
        inter=inter, void_count=void_count, pred_count=pred_count, pred_class=pred_class, confidence=confidence, count=count, gt_count=gt_count)
    dev = inter.device
    thresholds = _on_device(thresholds=thresholds)[0] if isinstance(thresholds, torch.Tensor) else _threshold_tensor(thresholds, dev)
    t = thresholds.shape[0]
    with torch.no_grad():
        n_true = torch.empty((b, t, r), dtype=torch.int32, device=dev)
        n_false = torch.empty((b, t, r), dtype=torch.int32, device=dev)
        hard_fn = torch.empty((b, t, c), dtype=torch.int32, device=dev)
        n_gt = torch.empty((b, c), dtype=torch.int32, device=dev)
        n_pred = torch.empty((b, c), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().gspn_instance_match(b, r, c, g, t, min_region, L.ptr(inter), L.ptr(void_count), L.ptr(pred_count), L.ptr(pred_class),
                                                L.ptr(confidence), L.ptr(count), L.ptr(gt_count), L.ptr(thresholds), L.ptr(n_true), L.ptr(n_false),
                                                L.ptr(hard_fn), L.ptr(n_gt), L.ptr(n_pred), L.stream()), "instance_match")
    return n_true, n_false, hard_fn, n_gt, n_pred


def _inverse_map(label_map):
    """label id -> class for the classes 1..C-1 of label_map (class 0's id is the id of no class)"""
    table = [int(v) for v in (label_map.tolist() if hasattr(label_map, "tolist") else label_map)]
    if len(table) < 1 or min(table) < 0:
        raise ValueError("label_map must hold one non-negative label id per class, got %r" % (table,))
    inverse = {}
    for s in range(1, len(table)):
        if table[s] in inverse or table[s] == table[0]:
            raise ValueError("label_map must give every class its own label id, got %r" % (table,))
        inverse[table[s]] = s
    return table, inverse


def classes_from_label_ids(label_ids, label_map=SCANNET_LABEL_MAP):
    """The inverse of label_map on the device: label_ids int32 of any shape -> the class s in [1, C) with label_map[s] == id, and 0 for every id
    the map does not hold (label_map[0] included).  The dense table of max(label_map) + 1 entries is copied to the device once."""
    label_ids = _typed(label_ids, torch.int32, None, "label_ids")
    table, inverse = _inverse_map(label_map)
    label_ids = _on_device(label_ids=label_ids)[0]
    size = max(table) + 1

    def make():
        dense = torch.zeros(size, dtype=torch.int32)
        for label, s in inverse.items():
            dense[label] = s
        return dense.to(label_ids.device)

    dense = _cached("inv", tuple(table), label_ids.device, make)
    with torch.no_grad():
        inside = (label_ids >= 0) & (label_ids < size)
        return torch.where(inside, dense[label_ids.clamp(0, size - 1).long()], torch.zeros_like(label_ids))


def average_precision(y_true, y_score, hard_false_negatives):
    """The benchmark's precision / recall curve for one (class, threshold): y_true (0 or 1) and y_score, one entry per record, and the number
    of gts that no record stands for -> AP, a float.  float64 numpy throughout; host only.  No record at all gives 0."""
    y_true = np.asarray(y_true, dtype=np.float64).reshape(-1)
    y_score = np.asarray(y_score, dtype=np.float64).reshape(-1)
    if y_true.shape != y_score.shape:
        raise ValueError("average_precision: one score per record, got %d and %d" % (y_true.size, y_score.size))
    order = np.argsort(y_score, kind="stable")
    score_sorted, true_sorted = y_score[order], y_true[order]
    cumsum = np.cumsum(true_sorted)
    _, starts = np.unique(score_sorted, return_index=True)
    n = len(score_sorted)
    total_true = cumsum[-1] if n else 0.0
    precision = np.zeros(len(starts) + 1)
    recall = np.zeros(len(starts) + 1)
    for at, i in enumerate(starts):
        cum = cumsum[i - 1] if i > 0 else 0.0
        tp = total_true - cum
        fp = n - i - tp
        fn = cum + hard_false_negatives
        precision[at] = float(tp) / (tp + fp)
        recall[at] = float(tp) / (tp + fn) if tp + fn > 0 else 0.0
    precision[-1] = 1.0                                                            # the artificial last point
    recall[-1] = 0.0
    stepped = np.concatenate(([recall[0]], recall, [0.0]))
    widths = np.convolve(stepped, [-0.5, 0, 0.5], "valid")
    return float(np.dot(precision, widths))


_FIELDS = ("n_true", "n_false", "hard_fn", "n_gt", "n_pred", "pred_class", "confidence")


class InstanceAP:
    """AP / AP50 / AP25 of an evaluation pass, accumulated on the device.

        metric = InstanceAP(num_class=19)
        for each batch:  metric.add_predictions(scene_predictions(end_points, pc), seg_label, group_label, ngroup)
        result = metric.compute()        # the one transfer

    add / add_predictions launch the two kernels and keep their small outputs (a few (B, T, R) and (B, T, C) int32 tensors) on the device; they
    return that batch's outputs as a dict.  Inside a captured step the dict's tensors belong to the graph and every replay overwrites them: clone
    them after a replay and hand the clones to add_counts.  num_class = C counts class 0, the class of no instance."""

    def __init__(self, num_class, overlaps=DEFAULT_OVERLAPS, min_region_size=MIN_REGION_SIZE, label_map=SCANNET_LABEL_MAP, class_names=None):
        self.num_class = int(num_class)
        if self.num_class < 2:
            raise ValueError("InstanceAP: needs class 0 and at least one class of instances, got num_class = %d" % self.num_class)
        self.overlaps = np.array(overlaps, dtype=np.float64).reshape(-1)
        if self.overlaps.size == 0 or np.isnan(self.overlaps).any():
            raise ValueError("InstanceAP: overlaps must be a non-empty sequence without NaN")
        self.min_region_size = int(min_region_size)
        if self.min_region_size < 1:
            raise NotImplementedError("InstanceAP: min_region_size >= 1 (got %d)" % self.min_region_size)
        self.label_map = None
        if label_map is not None:
            self.label_map, _ = _inverse_map(label_map)
            if len(self.label_map) != self.num_class:
                raise ValueError("InstanceAP: label_map must have one entry per class, %d, got %d" % (self.num_class, len(self.label_map)))
        if class_names is None:
            same = self.label_map is not None and tuple(self.label_map) == tuple(SCANNET_LABEL_MAP)
            class_names = SCANNET_CLASS_NAMES if same else tuple("class_%d" % s for s in range(1, self.num_class))
        self.class_names = tuple(str(v) for v in class_names)
        if len(self.class_names) != self.num_class - 1:
            raise ValueError("InstanceAP: one name per class 1..C-1, %d, got %d" % (self.num_class - 1, len(self.class_names)))
        self._batches = []

    def reset(self):
        self._batches = []

    def add(self, masks, pred_class, confidence, count, seg_label, group_label, ngroup):
        """one batch: masks (B, R, N) uint8, pred_class (B, R) int32, confidence (B, R) float32, count (B,) int32, seg_label, group_label (B, N)
        int32, ngroup a Python integer (every group label below it) -> this batch's outputs of instance_match, kept for compute()"""
        inter, void_count, pred_count, gt_count = instance_overlaps(masks, pred_class, seg_label, group_label, self.num_class, ngroup)
        n_true, n_false, hard_fn, n_gt, n_pred = instance_match(inter, void_count, pred_count, pred_class, confidence, count, gt_count,
                                                                self.overlaps, self.min_region_size)
        return self.add_counts({"n_true": n_true, "n_false": n_false, "hard_fn": hard_fn, "n_gt": n_gt, "n_pred": n_pred,
                                "pred_class": pred_class.detach().clone(), "confidence": confidence.detach().clone()})       # the caller may reuse its buffers

    def add_predictions(self, pred, seg_label, group_label, ngroup):
        """one batch of scene_predictions' result, as it is: its label ids go back to classes through label_map on the device"""
        for k in ("masks", "label_ids", "confidence", "count"):
            if k not in pred:
                raise ValueError("InstanceAP.add_predictions: pred has no %r (pass scene_predictions' result)" % k)
        if self.label_map is None:
            raise ValueError("InstanceAP.add_predictions: needs the label_map the predictions were made with")
        return self.add(pred["masks"], classes_from_label_ids(pred["label_ids"], self.label_map), pred["confidence"], pred["count"], seg_label,
                        group_label, ngroup)

    def add_counts(self, batch):
        """a batch's outputs as add returned them (or clones of them)"""
        t, c = len(self.overlaps), self.num_class
        b, r = batch["pred_class"].shape
        want = {"n_true": (b, t, r), "n_false": (b, t, r), "hard_fn": (b, t, c), "n_gt": (b, c), "n_pred": (b, c), "pred_class": (b, r),
                "confidence": (b, r)}
        for k in _FIELDS:
            dtype = torch.float32 if k == "confidence" else torch.int32
            if tuple(_typed(batch[k], dtype, None, k).shape) != want[k]:
                raise ValueError("InstanceAP.add_counts: %s must be %s, got %s" % (k, want[k], tuple(batch[k].shape)))
        batch = {k: batch[k] for k in _FIELDS}
        self._batches.append(batch)
        return batch

    def _records(self):
        """one transfer of everything kept -> per batch, the fields as numpy arrays"""
        if not self._batches:
            return []
        with torch.no_grad():
            flat = torch.cat([batch[k].contiguous().view(torch.int32).reshape(-1) for batch in self._batches for k in _FIELDS]).cpu().numpy()
        out, at = [], 0
        for batch in self._batches:
            fields = {}
            for k in _FIELDS:
                size = batch[k].numel()
                part = flat[at:at + size].reshape(tuple(batch[k].shape))
                fields[k] = part.view(np.float32) if k == "confidence" else part
                at += size
            out.append(fields)
        return out

    def compute(self):
        """-> {"overlaps": (T,) float64, "ap": (C - 1, T) float64 (row s - 1 is class s; nan where the class has no gt),
        "class_names", "class_ids", "classes": {name: {"ap", "ap50%", "ap25%"}}, "all_ap", "all_ap_50%", "all_ap_25%"}"""
        t, c = len(self.overlaps), self.num_class
        batches = self._records()
        has_gt, has_pred = np.zeros(c, bool), np.zeros(c, bool)
        hard = np.zeros((t, c), np.int64)
        for f in batches:
            has_gt |= (f["n_gt"] > 0).any(0)
            has_pred |= (f["n_pred"] > 0).any(0)
            hard += f["hard_fn"].sum(0)
        ap = np.full((c - 1, t), np.nan)
        for s in range(1, c):
            if not has_gt[s]:
                continue
            if not has_pred[s]:
                ap[s - 1] = 0.0
                continue
            for ti in range(t):
                y_true, y_score = [], []
                for f in batches:
                    rows = f["pred_class"] == s                                    # (B, R)
                    conf = f["confidence"][rows].astype(np.float64)
                    for flag, counts in ((1.0, f["n_true"][:, ti][rows]), (0.0, f["n_false"][:, ti][rows])):
                        y_score.append(np.repeat(conf, counts))
                        y_true.append(np.full(int(counts.sum()), flag))
                ap[s - 1, ti] = average_precision(np.concatenate(y_true), np.concatenate(y_score), int(hard[ti, s]))
        o50 = np.isclose(self.overlaps, 0.5)
        o25 = np.isclose(self.overlaps, 0.25)
        rest = ~o25
        label_ids = self.label_map if self.label_map is not None else list(range(c))

        def mean(values, over_classes):
            if values.size == 0:
                return float("nan")
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)                    # a mean over nothing but nan is nan, said once here
                return float(np.nanmean(values)) if over_classes else float(np.average(values))

        classes = {name: {"ap": mean(ap[i, rest], False), "ap50%": mean(ap[i, o50], False), "ap25%": mean(ap[i, o25], False)}
                   for i, name in enumerate(self.class_names)}
        return {"overlaps": self.overlaps.copy(), "ap": ap, "class_names": list(self.class_names), "class_ids": [int(v) for v in label_ids[1:]],
                "classes": classes, "all_ap": mean(ap[:, rest], True), "all_ap_50%": mean(ap[:, o50], True), "all_ap_25%": mean(ap[:, o25], True)}


# ---- host IO: the readers of what predict.write_predictions / write_ground_truth write, plain Python ------------------------------------------

def _read_ids(path):
    with open(path) as f:
        return [int(line) for line in f.read().split()]


def read_predictions(pred_dir, scan, n):
    """<pred_dir>/<scan>.txt and the mask files it names, for a scene of n points -> masks (K, n) uint8, label_ids (K,) int32, confidence (K,)
    float32, in the file's order.  Raises ValueError on a line that does not have three fields or a mask that does not have n entries."""
    masks, labels, confidence = [], [], []
    with open(os.path.join(pred_dir, scan + ".txt")) as f:
        lines = [line for line in f.read().splitlines() if line.strip()]
    for line in lines:
        parts = line.rsplit(None, 2)
        if len(parts) != 3:
            raise ValueError("read_predictions: %s.txt: expected '<mask file> <label id> <confidence>', got %r" % (scan, line))
        mask = _read_ids(os.path.join(pred_dir, parts[0]))
        if len(mask) != n:
            raise ValueError("read_predictions: %s has %d entries, the scene has %d points" % (parts[0], len(mask), n))
        masks.append(np.asarray(mask, dtype=np.int64) != 0)
        labels.append(int(parts[1]))
        confidence.append(float(parts[2]))
    return (np.array(masks, dtype=np.uint8).reshape(len(masks), n), np.array(labels, dtype=np.int32), np.array(confidence, dtype=np.float32))


def read_ground_truth(gt_dir, scan, label_map=SCANNET_LABEL_MAP):
    """<gt_dir>/<scan>.txt, one id = label id * 1000 + group per point -> seg_label, group_label (N,) int32, the classes of label_map.  An id
    below 1000 is a point of no class (class 0, with its group).  Raises ValueError on a label id the map does not hold."""
    table, inverse = _inverse_map(label_map)
    inverse = dict(inverse)
    inverse[0] = 0
    inverse[table[0]] = 0
    ids = np.asarray(_read_ids(os.path.join(gt_dir, scan + ".txt")), dtype=np.int64)
    if ids.size and ids.min() < 0:
        raise ValueError("read_ground_truth: %s.txt holds a negative id" % scan)
    labels, group = ids // 1000, ids % 1000
    unknown = sorted(set(labels.tolist()) - set(inverse))
    if unknown:
        raise ValueError("read_ground_truth: %s.txt holds label ids the label map does not: %r" % (scan, unknown))
    seg = np.zeros(ids.shape, dtype=np.int32)
    for label, s in inverse.items():
        seg[labels == label] = s
    return seg, group.astype(np.int32)


def evaluate_files(pred_dir, gt_dir, scans, overlaps=DEFAULT_OVERLAPS, min_region_size=MIN_REGION_SIZE, label_map=SCANNET_LABEL_MAP,
                   class_names=None, device="cuda"):
    """The evaluation over files: for every scan, <gt_dir>/<scan>.txt and <pred_dir>/<scan>.txt with its masks go to the device, one scene per
    add -> InstanceAP.compute().  Raises ValueError on a label id of a prediction that the map does not hold."""
    table, inverse = _inverse_map(label_map)
    metric = InstanceAP(len(table), overlaps, min_region_size, label_map, class_names)
    device = torch.device(device)
    for scan in scans:
        seg, group = read_ground_truth(gt_dir, scan, label_map)
        n = seg.shape[0]
        masks, labels, confidence = read_predictions(pred_dir, scan, n)
        unknown = sorted(set(labels.tolist()) - set(inverse))
        if unknown:
            raise ValueError("evaluate_files: %s.txt predicts label ids the label map does not hold: %r" % (scan, unknown))
        k = masks.shape[0]
        if k == 0:                                                                # a scene without a prediction: one row beyond count
            masks, labels, confidence = np.zeros((1, n), np.uint8), np.zeros(1, np.int32), np.zeros(1, np.float32)
        pred_class = np.array([inverse.get(int(v), 0) for v in labels], dtype=np.int32)
        metric.add(torch.from_numpy(masks).unsqueeze(0).to(device), torch.from_numpy(pred_class).unsqueeze(0).to(device),
                   torch.from_numpy(confidence).unsqueeze(0).to(device), torch.tensor([k], dtype=torch.int32, device=device),
                   torch.from_numpy(seg).unsqueeze(0).to(device), torch.from_numpy(group).unsqueeze(0).to(device), int(group.max()) + 1 if n else 1)
    return metric.compute()


def write_result_file(path, result):
    """the benchmark's result file: a header and one line 'class,class id,ap,ap50,ap25' per class"""
    with open(path, "w") as f:
        f.write(",".join(("class", "class id", "ap", "ap50", "ap25")) + "\n")
        for name, label in zip(result["class_names"], result["class_ids"]):
            v = result["classes"][name]
            f.write(",".join(str(x) for x in (name, label, v["ap"], v["ap50%"], v["ap25%"])) + "\n")
