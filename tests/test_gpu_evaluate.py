"""GPU tests of gspn_amd/evaluate.py on the kernels of csrc/evaluate.hip.  The oracle is the plain dict-and-loop restatement of the metric in
this file (DESIGN.md 4.18 has the definition): ref_overlaps counts point by point, ref_match walks gts and rows as the benchmark's script
does, ref_average_precision is the curve, ref_evaluate puts them together.  Every count is compared as an exact integer; AP values within
1e-12 with nan in the same places."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

THRESHOLDS = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
T50, T25 = 0, 9                                                                     # where 0.5 and 0.25 sit in THRESHOLDS


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------------

def ref_overlaps(masks, cls, seg, group, c, g):
    """one scene: masks (R, N), cls (R,), seg, group (N,) -> inter (R, G), void (R,), size (R,), gt (C, G) as Python lists"""
    r, n = masks.shape
    inter = [[0] * g for _ in range(r)]
    void, size = [0] * r, [0] * r
    gt = [[0] * g for _ in range(c)]
    is_void = [not (1 <= int(seg[j]) < c and 0 <= int(group[j]) < g) for j in range(n)]
    for j in range(n):
        if not is_void[j]:
            gt[int(seg[j])][int(group[j])] += 1
    for k in range(r):
        if not 1 <= int(cls[k]) < c:
            continue
        for j in np.nonzero(masks[k])[0].tolist():
            size[k] += 1
            if is_void[j]:
                void[k] += 1
            elif int(seg[j]) == int(cls[k]):
                inter[k][int(group[j])] += 1
    return inter, void, size, gt


def iou_of(inter, gt_points, pred_points):
    return np.float64(inter) / np.float64(gt_points + pred_points - inter)


def ref_match(inter, void, size, gt, cls, conf, count, c, g, thresholds, min_region):
    """one scene -> n_true, n_false [t][k], hard [t][s], n_gt [s], n_pred [s]"""
    r = len(cls)
    valid = [k < count and 1 <= int(cls[k]) < c and size[k] >= min_region for k in range(r)]
    n_true = [[0] * r for _ in thresholds]
    n_false = [[0] * r for _ in thresholds]
    hard = [[0] * c for _ in thresholds]
    n_gt = [sum(1 for j in range(g) if s >= 1 and gt[s][j] >= min_region) for s in range(c)]
    n_pred = [sum(1 for k in range(r) if valid[k] and int(cls[k]) == s) for s in range(c)]
    for ti, th in enumerate(thresholds):
        for s in range(1, c):
            rows = [k for k in range(r) if valid[k] and int(cls[k]) == s]
            visited = {k: False for k in rows}
            for j in range(g):
                if gt[s][j] < min_region:
                    continue
                events = []
                for k in rows:
                    if inter[k][j] <= 0 or visited[k]:
                        continue
                    if iou_of(inter[k][j], gt[s][j], size[k]) > th:
                        events.append(k)
                        if len(events) == 1:
                            visited[k] = True
                if not events:
                    hard[ti][s] += 1
                    continue
                holder = events[0]
                for k in events[1:]:
                    if np.float32(conf[k]) > np.float32(conf[holder]):
                        holder = k
                for k in events:
                    (n_true if k == holder else n_false)[ti][k] += 1
            for k in rows:
                if any(inter[k][j] > 0 and iou_of(inter[k][j], gt[s][j], size[k]) > th for j in range(g)):
                    continue
                ignore = void[k] + sum(inter[k][j] for j in range(g) if gt[s][j] < min_region)
                if np.float64(ignore) / np.float64(size[k]) <= th:
                    n_false[ti][k] += 1
    return n_true, n_false, hard, n_gt, n_pred


def ref_average_precision(records, hard_fn):
    """records: a list of (true, score)"""
    y_true = np.array([t for t, _ in records], dtype=np.float64)
    y_score = np.array([s for _, s in records], dtype=np.float64)
    order = np.argsort(y_score)
    y_score, y_true = y_score[order], y_true[order]
    cumsum = np.cumsum(y_true)
    _, starts = np.unique(y_score, return_index=True)
    n = len(y_score)
    total = cumsum[-1] if n else 0.0
    precision, recall = [], []
    for i in starts:
        cum = cumsum[i - 1] if i > 0 else 0.0
        tp = total - cum
        fp = n - i - tp
        fn = cum + hard_fn
        precision.append(tp / (tp + fp))
        recall.append(tp / (tp + fn))
    precision.append(1.0)
    recall.append(0.0)
    stepped = np.array([recall[0]] + recall + [0.0])
    return float(np.dot(np.array(precision), np.convolve(stepped, [-0.5, 0, 0.5], "valid")))


def ref_evaluate(scenes, c, thresholds, min_region):
    """scenes: dicts of masks (R, N), cls, conf (R,), count, seg, group (N,), g -> (ap (C-1, T), all_ap, all_ap_50, all_ap_25)"""
    records = {(ti, s): [] for ti in range(len(thresholds)) for s in range(1, c)}
    hard = {key: 0 for key in records}
    has_gt, has_pred = [False] * c, [False] * c
    for sc in scenes:
        inter, void, size, gt = ref_overlaps(sc["masks"], sc["cls"], sc["seg"], sc["group"], c, sc["g"])
        n_true, n_false, hard_fn, n_gt, n_pred = ref_match(inter, void, size, gt, sc["cls"], sc["conf"], sc["count"], c, sc["g"], thresholds, min_region)
        for s in range(1, c):
            has_gt[s] |= n_gt[s] > 0
            has_pred[s] |= n_pred[s] > 0
            for ti in range(len(thresholds)):
                hard[ti, s] += hard_fn[ti][s]
                for k in range(len(sc["cls"])):
                    if int(sc["cls"][k]) == s:
                        score = float(np.float32(sc["conf"][k]))
                        records[ti, s] += [(1, score)] * n_true[ti][k] + [(0, score)] * n_false[ti][k]
    ap = np.full((c - 1, len(thresholds)), np.nan)
    for (ti, s), rec in records.items():
        if has_gt[s] and has_pred[s]:
            ap[s - 1, ti] = ref_average_precision(rec, hard[ti, s])
        elif has_gt[s]:
            ap[s - 1, ti] = 0.0
    o25 = np.isclose(thresholds, 0.25)
    o50 = np.isclose(thresholds, 0.5)
    return ap, np.nanmean(ap[:, ~o25]), np.nanmean(ap[:, o50]), np.nanmean(ap[:, o25])


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------

def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def batch_tensors(scenes):
    """scenes of one (R, N) -> the arguments of InstanceAP.add, without ngroup"""
    return (dev(np.stack([s["masks"] for s in scenes]), torch.uint8), dev(np.stack([s["cls"] for s in scenes]), torch.int32),
            dev(np.stack([s["conf"] for s in scenes]), torch.float32), dev(np.array([s["count"] for s in scenes]), torch.int32),
            dev(np.stack([s["seg"] for s in scenes]), torch.int32), dev(np.stack([s["group"] for s in scenes]), torch.int32))


def check_counts(scenes, c, g, thresholds, min_region):
    """instance_overlaps and instance_match on the batch against the oracle, scene by scene; -> the oracle's per-scene results"""
    from gspn_amd.evaluate import instance_match, instance_overlaps
    masks, cls, conf, count, seg, group = batch_tensors(scenes)
    inter, void, size, gt = instance_overlaps(masks, cls, seg, group, c, g)
    got = instance_match(inter, void, size, cls, conf, count, gt, thresholds, min_region)
    assert inter.dtype == void.dtype == size.dtype == gt.dtype == torch.int32 and all(t.dtype == torch.int32 for t in got)
    names = ("n_true", "n_false", "hard_fn", "n_gt", "n_pred")
    want_all = []
    for i, sc in enumerate(scenes):
        w_inter, w_void, w_size, w_gt = ref_overlaps(sc["masks"], sc["cls"], sc["seg"], sc["group"], c, g)
        assert inter[i].tolist() == w_inter and void[i].tolist() == w_void and size[i].tolist() == w_size and gt[i].tolist() == w_gt, i
        want = ref_match(w_inter, w_void, w_size, w_gt, sc["cls"], sc["conf"], sc["count"], c, g, thresholds, min_region)
        for name, have, w in zip(names, got, want):
            assert have[i].tolist() == w, (i, name, have[i].tolist(), w)
        want_all.append(dict(zip(names, want)))
    return want_all


def random_scene(rng, n, r, c, g, lo, hi, confidences=(1.0, 0.97, 0.5, 0.5, 0.25)):
    """blocks of lo..hi points, each of one (class, group); predictions are noisy copies of blocks; a few labels out of range"""
    seg, group = np.zeros(n, np.int32), np.zeros(n, np.int32)
    blocks, pos = [], 0
    while pos < n:
        stop = min(n, pos + int(rng.integers(lo, hi + 1)))
        s, j = int(rng.integers(0, c)), len(blocks) % g
        seg[pos:stop], group[pos:stop] = s, j
        blocks.append((pos, stop, s))
        pos = stop
    for value, into in ((-1, seg), (c, seg), (-1, group), (g, group)):
        into[rng.integers(0, n, 2)] = value
    masks = np.zeros((r, n), np.uint8)
    cls = np.zeros(r, np.int32)
    for k in range(r):
        a, b, s = blocks[int(rng.integers(0, len(blocks)))]
        cls[k] = s if s > 0 and rng.random() < 0.8 else int(rng.integers(0, c + 1))
        keep = (1.0, 0.9, 0.6, 0.3)[int(rng.integers(0, 4))]
        masks[k, a:b] = rng.random(b - a) < keep
        extra = int(rng.integers(0, 3)) * (b - a) // 2                              # none, half a block or a whole block more, behind it
        masks[k, b:min(n, b + extra)] = 1
    perm = rng.permutation(n)
    return {"masks": np.ascontiguousarray(masks[:, perm]), "cls": cls, "conf": rng.choice(np.array(confidences, np.float32), r),
            "count": r - int(rng.integers(0, min(3, r))), "seg": seg[perm], "group": group[perm], "g": g}


# ---- 1. instance_overlaps ------------------------------------------------------------------------------------------------------------------

def overlap_inputs(b, r, n, c, g, seed):
    rng = np.random.default_rng(seed)
    masks = (rng.random((b, r, n)) < np.where(np.arange(r) % 2 == 0, 0.01, 0.5)[None, :, None]).astype(np.uint8)
    cls = rng.integers(1, c, (b, r)).astype(np.int32)
    if r >= 5:                                                                      # row 1 stays a half-full row of a valid class
        masks[:, 0] = 0
        masks[:, 4] = 1
        cls[:, 2] = 0
        cls[:, 3] = c
    else:                                                                           # one row per scene: all ones, about 1 %, none
        masks[0] = 1
        masks[-1] = 0
    seg = rng.integers(-1, c + 1, (b, n)).astype(np.int32)                          # below 0 and at C: void
    group = rng.integers(-1, g + 1, (b, n)).astype(np.int32)
    return masks, cls, seg, group


@pytest.mark.parametrize("shape", [(2, 5, 1003, 4, 7), (1, 37, 4099, 19, 100), (3, 1, 257, 2, 1)])
def test_instance_overlaps_against_the_loops(shape):
    from gspn_amd.evaluate import instance_overlaps
    b, r, n, c, g = shape
    masks, cls, seg, group = overlap_inputs(*shape, seed=sum(shape))
    assert (seg < 0).any() and (seg >= c).any() and (group < 0).any() and (group >= g).any()
    args = (dev(cls, torch.int32), dev(seg, torch.int32), dev(group, torch.int32), c, g)
    got = instance_overlaps(dev(masks, torch.uint8), *args)
    shifted = torch.empty(b * r * n + 1, dtype=torch.uint8, device="cuda")[1:].view(b, r, n)      # its storage starts one byte into an allocation
    shifted.copy_(torch.from_numpy(masks))
    assert shifted.data_ptr() % 16 == 1 and shifted.is_contiguous()
    again = instance_overlaps(shifted, *args)
    seen_void = False
    for i in range(b):
        want = ref_overlaps(masks[i], cls[i], seg[i], group[i], c, g)
        for have, other, w in zip(got, again, want):
            assert have[i].tolist() == w and other[i].tolist() == w
        seen_void |= any(want[1])
        if r >= 5:
            assert want[2][0] == 0 and want[2][4] == n and want[2][2] == 0 and want[2][3] == 0          # the empty row, the full row, classes 0 and C
            assert 0.4 * n < want[2][1] < 0.6 * n
    assert seen_void


def test_instance_overlaps_limits():
    from gspn_amd.evaluate import instance_overlaps
    masks, cls, seg, group = overlap_inputs(1, 2, 300, 2, 4096, seed=3)
    t = (dev(masks, torch.uint8), dev(cls, torch.int32), dev(seg, torch.int32), dev(group, torch.int32))
    got = instance_overlaps(*t, 2, 4096)
    want = ref_overlaps(masks[0], cls[0], seg[0], group[0], 2, 4096)
    for have, w in zip(got, want):
        assert have[0].tolist() == w
    with pytest.raises(NotImplementedError):
        instance_overlaps(*t, 2, 4097)
    with pytest.raises(NotImplementedError):
        instance_overlaps(*t, 3, 2731)                                              # C * G = 8193


# ---- 2. instance_match ---------------------------------------------------------------------------------------------------------------------

N_HAND, R_HAND, C_HAND, G_HAND = 40, 3, 4, 4


def hand_scene(gts, preds, count=None):
    """gts: (class, group, start, stop); preds: (class, confidence, [(start, stop), ...]); unlabelled points are void"""
    seg, group = np.zeros(N_HAND, np.int32), np.zeros(N_HAND, np.int32)
    for s, j, a, b in gts:
        seg[a:b], group[a:b] = s, j
    masks, cls, conf = np.zeros((R_HAND, N_HAND), np.uint8), np.zeros(R_HAND, np.int32), np.zeros(R_HAND, np.float32)
    for k, (s, cf, spans) in enumerate(preds):
        cls[k], conf[k] = s, cf
        for a, b in spans:
            masks[k, a:b] = 1
    return {"masks": masks, "cls": cls, "conf": conf, "count": len(preds) if count is None else count, "seg": seg, "group": group, "g": G_HAND}


HAND = {
    # both rows cover the gt; the first is visited, the second has the higher confidence and holds the match
    "duplicate": hand_scene([(1, 1, 0, 10)], [(1, 0.5, [(0, 10)]), (1, 0.9, [(0, 10)])]),
    # row 1 is a later event of gt A (row 0 is visited there) and the only event of gt B: an event of two gts at 0.25
    "two_gts": hand_scene([(1, 0, 0, 10), (1, 1, 10, 20)], [(1, 0.9, [(0, 10)]), (1, 0.8, [(0, 20)])]),
    # the one row is visited by gt A, so gt B finds nothing at 0.25
    "visited": hand_scene([(1, 0, 0, 10), (1, 1, 10, 20)], [(1, 0.9, [(0, 20)])]),
    # 5 of the gt's 5 points and 5 points of another class: iou = 5 / 10
    "iou_at_th": hand_scene([(1, 0, 0, 5), (2, 1, 5, 15)], [(1, 0.9, [(0, 10)])]),
    # 5 void + 5 of class 2, and 6 void + 4 of class 2, both predicted as class 1, which has no gt
    "ignore_at_th": hand_scene([(2, 1, 0, 10)], [(1, 0.9, [(0, 5), (20, 25)]), (1, 0.9, [(0, 4), (20, 26)])]),
    # 2 points of a 4-point gt + 2 void + 1 of class 2: ignore = 4 / 5, without the small gt it would be 2 / 5
    "small_gt": hand_scene([(1, 0, 0, 4), (2, 1, 10, 20)], [(1, 0.9, [(0, 2), (10, 11), (30, 32)])]),
    # a 4-point prediction inside a 10-point gt
    "small_pred": hand_scene([(1, 0, 0, 10)], [(1, 0.9, [(0, 4)])]),
    # count = 1: the perfect rows 1 and 2 are not predictions
    "beyond_count": hand_scene([(1, 0, 0, 10)], [(2, 0.9, [(20, 30)]), (1, 0.9, [(0, 10)]), (1, 0.9, [(0, 10)])], count=1),
    # equal confidences: the lower row holds the match
    "equal_conf": hand_scene([(1, 2, 0, 10)], [(1, 0.5, [(0, 10)]), (1, 0.5, [(0, 10)])]),
    # class 3 has a gt and no prediction, class 2 a prediction and no gt
    "converse": hand_scene([(3, 0, 0, 10)], [(2, 0.9, [(0, 10)])]),
}


def test_instance_match_constructed_scenes():
    names = list(HAND)
    want = dict(zip(names, check_counts([HAND[k] for k in names], C_HAND, G_HAND, THRESHOLDS, 5)))
    every = range(len(THRESHOLDS))
    w = want["duplicate"]
    assert all(w["n_true"][t] == [0, 1, 0] and w["n_false"][t] == [1, 0, 0] and w["hard_fn"][t][1] == 0 for t in every)
    w = want["two_gts"]
    assert w["n_true"][T25] == [1, 1, 0] and w["n_false"][T25] == [0, 1, 0] and w["hard_fn"][T25][1] == 0
    assert w["n_true"][T50] == [1, 0, 0] and w["n_false"][T50] == [0, 1, 0] and w["hard_fn"][T50][1] == 1
    w = want["visited"]
    assert w["n_true"][T25] == [1, 0, 0] and w["hard_fn"][T25][1] == 1 and w["hard_fn"][T50][1] == 2 and w["n_false"][T50] == [1, 0, 0]
    w = want["iou_at_th"]
    assert w["n_true"][T50] == [0, 0, 0] and w["hard_fn"][T50][1] == 1 and w["n_false"][T50] == [1, 0, 0] and w["n_true"][T25] == [1, 0, 0]
    w = want["ignore_at_th"]
    assert w["n_false"][T50] == [1, 0, 0] and w["n_false"][T25] == [0, 0, 0] and w["n_gt"][1] == 0 and w["n_pred"][1] == 2
    w = want["small_gt"]
    assert w["n_false"][T50] == [0, 0, 0] and w["n_gt"][1] == 0 and w["n_pred"][1] == 1 and w["hard_fn"][T50][1] == 0
    w = want["small_pred"]
    assert all(w["hard_fn"][t][1] == 1 and w["n_true"][t] == [0, 0, 0] and w["n_false"][t] == [0, 0, 0] for t in every) and w["n_pred"][1] == 0
    w = want["beyond_count"]
    assert all(w["hard_fn"][t][1] == 1 and w["n_true"][t] == [0, 0, 0] for t in every) and w["n_pred"] == [0, 0, 1, 0]
    w = want["equal_conf"]
    assert all(w["n_true"][t] == [1, 0, 0] and w["n_false"][t] == [0, 1, 0] for t in every) and w["n_gt"][1] == 1
    w = want["converse"]
    assert w["n_gt"] == [0, 0, 0, 1] and w["n_pred"] == [0, 0, 1, 0] and w["hard_fn"][T50][3] == 1 and w["n_false"][T50] == [1, 0, 0]
    assert want["duplicate"]["n_gt"][1] == 1 and want["two_gts"]["n_gt"][1] == 2                   # group 0 under a valid class is a gt


@pytest.mark.parametrize("r", [1, 63, 64, 65, 130])
def test_instance_match_random_scenes(r):
    rng = np.random.default_rng(100 + r)
    want = check_counts([random_scene(rng, 600, r, 4, 9, 4, 40) for _ in range(4)], 4, 9, THRESHOLDS, 5)
    if r > 1:
        assert sum(sum(map(sum, w["n_true"])) for w in want) > 0 and sum(sum(map(sum, w["n_false"])) for w in want) > 0
        assert sum(sum(map(sum, w["hard_fn"])) for w in want) > 0


def test_instance_match_at_1024_rows_and_the_limit():
    from gspn_amd.evaluate import instance_match
    rng = np.random.default_rng(1024)
    want = check_counts([random_scene(rng, 1500, 1024, 3, 12, 20, 60)], 3, 12, THRESHOLDS[[0, 5, 9]], 5)
    assert max(map(max, want[0]["n_true"])) >= 1 and sum(map(sum, want[0]["n_false"])) > 0
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        instance_match(z(1, 1025, 2), z(1, 1025), z(1, 1025), z(1, 1025), torch.zeros(1, 1025, device="cuda"), z(1), z(1, 2, 2))
    with pytest.raises(NotImplementedError):
        instance_match(z(1, 4, 2), z(1, 4), z(1, 4), z(1, 4), torch.zeros(1, 4, device="cuda"), z(1), z(1, 2, 2), min_region=0)


# ---- 3. InstanceAP -------------------------------------------------------------------------------------------------------------------------

C_AP, G_AP = 5, 12
AP_MAP = (0, 3, 4, 5, 7)                                                           # class -> label id


@pytest.fixture(scope="module")
def ap_scenes():
    rng = np.random.default_rng(77)
    scenes = [random_scene(rng, 3000, 12, C_AP, G_AP, 60, 330, confidences=(1.0, 0.97, 0.75, 0.5, 0.5, 0.125)) for _ in range(6)]
    gts = preds = 0
    for sc in scenes:
        _, _, size, gt = ref_overlaps(sc["masks"], sc["cls"], sc["seg"], sc["group"], C_AP, G_AP)
        gts += sum(v >= 100 for row in gt[1:] for v in row)
        preds += sum(size[k] >= 100 for k in range(sc["count"]))
    assert gts >= 10 and preds >= 10
    return scenes, ref_evaluate(scenes, C_AP, THRESHOLDS, 100)


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(np.abs(a - b)[~np.isnan(a)] <= 1e-12))


def test_instance_ap_against_the_restated_evaluator(ap_scenes):
    from gspn_amd.evaluate import InstanceAP
    scenes, (ap, all_ap, all_50, all_25) = ap_scenes
    assert np.isfinite(ap).any() and 0 < all_ap < 1 and 0 < all_25 < 1
    metric = InstanceAP(C_AP, label_map=AP_MAP)
    for at in (0, 2, 4):
        metric.add(*batch_tensors(scenes[at:at + 2]), G_AP)
    got = metric.compute()
    assert same(got["ap"], ap) and same(got["all_ap"], all_ap) and same(got["all_ap_50%"], all_50) and same(got["all_ap_25%"], all_25)
    assert got["class_ids"] == [3, 4, 5, 7] and got["class_names"] == ["class_1", "class_2", "class_3", "class_4"]
    o25 = np.isclose(THRESHOLDS, 0.25)
    for i, name in enumerate(got["class_names"]):
        v = got["classes"][name]
        assert same(v["ap"], np.average(ap[i, ~o25])) and same(v["ap50%"], ap[i, T50]) and same(v["ap25%"], ap[i, T25])
    whole = InstanceAP(C_AP, label_map=AP_MAP)
    whole.add(*batch_tensors(scenes), G_AP)
    one = whole.compute()
    assert np.array_equal(one["ap"], got["ap"], equal_nan=True) and one["all_ap"] == got["all_ap"]
    metric.reset()
    metric.add(*batch_tensors(scenes[:2]), G_AP)
    assert same(metric.compute()["ap"], ref_evaluate(scenes[:2], C_AP, THRESHOLDS, 100)[0])


# ---- 4. perfect predictions ----------------------------------------------------------------------------------------------------------------

def test_perfect_predictions_score_one_and_empty_ones_zero():
    from gspn_amd.evaluate import InstanceAP
    n, c, g = 1200, 5, 8
    seg, group = np.zeros((2, n), np.int32), np.zeros((2, n), np.int32)
    blocks = [(0, 0, 150, 1, 0), (0, 150, 400, 2, 1), (0, 400, 450, 2, 2), (1, 100, 300, 1, 3), (1, 300, 420, 4, 0)]      # scene, start, stop, class, group
    masks, cls = np.zeros((2, 3, n), np.uint8), np.zeros((2, 3), np.int32)
    rows = [0, 0]
    for i, a, b, s, j in blocks:
        seg[i, a:b], group[i, a:b] = s, j
        if b - a >= 100:                                                            # the 50-point gt of class 2 is not eligible and gets no prediction
            masks[i, rows[i], a:b], cls[i, rows[i]] = 1, s
            rows[i] += 1
    labels = (dev(seg, torch.int32), dev(group, torch.int32), g)
    conf, count = torch.ones(2, 3, device="cuda"), dev(np.array(rows), torch.int32)
    metric = InstanceAP(c, label_map=None)
    metric.add(dev(masks, torch.uint8), dev(cls, torch.int32), conf, count, *labels)
    got = metric.compute()
    assert np.array_equal(got["ap"][[0, 1, 3]], np.ones((3, 10))) and np.isnan(got["ap"][2]).all()
    assert got["all_ap"] == 1.0 and got["all_ap_50%"] == 1.0 and got["all_ap_25%"] == 1.0
    metric.reset()
    metric.add(torch.zeros(2, 3, n, dtype=torch.uint8, device="cuda"), dev(cls, torch.int32), conf, count, *labels)
    got = metric.compute()
    assert np.array_equal(got["ap"][[0, 1, 3]], np.zeros((3, 10))) and np.isnan(got["ap"][2]).all() and got["all_ap"] == 0.0


# ---- 5. the captured chain -----------------------------------------------------------------------------------------------------------------

def test_chain_captured_behind_scene_predictions_and_replayed_on_new_inputs():
    from gspn_amd.evaluate import InstanceAP, classes_from_label_ids
    from gspn_amd.graph import CapturedStep
    from gspn_amd.predict import SCANNET_LABEL_MAP, scene_predictions
    from tests import predict_ref as PR
    shape = (2, 7, 3001, 64, 19)
    b, r, n, _, c = shape
    g = 6
    rng = np.random.default_rng(9)
    inputs = []
    for seed in (51, 52):
        pc, ep = PR.stage_inputs(*shape, seed=seed, ladder=False)
        inputs.append((pc, ep, torch.from_numpy(rng.integers(0, c, (b, n)).astype(np.int32)), torch.from_numpy(rng.integers(0, g, (b, n)).astype(np.int32))))
    pc, ep = inputs[0][0].cuda(), {k: v.cuda() for k, v in inputs[0][1].items()}
    seg, group = inputs[0][2].cuda(), inputs[0][3].cuda()
    captured, st = InstanceAP(c, min_region_size=5), {}
    step = CapturedStep(lambda: st.update(out=captured.add_predictions(scene_predictions(ep, pc), seg, group, g)))
    captured.reset()                                                                # the warm-up runs and the capture itself added three batches
    eager = InstanceAP(c, min_region_size=5)
    for new_pc, new_ep, new_seg, new_group in (inputs[1], inputs[0]):
        pc.copy_(new_pc)
        seg.copy_(new_seg)
        group.copy_(new_group)
        for k, v in new_ep.items():
            ep[k].copy_(v)
        step.replay()
        torch.cuda.synchronize()
        replayed = captured.add_counts({k: v.clone() for k, v in st["out"].items()})
        pred = scene_predictions({k: v.cuda() for k, v in new_ep.items()}, new_pc.cuda())              # eager, on fresh tensors
        want = eager.add_predictions(pred, new_seg.cuda(), new_group.cuda(), g)
        for k, w in want.items():
            assert torch.equal(replayed[k], w), k
        assert torch.equal(want["pred_class"], classes_from_label_ids(pred["label_ids"], SCANNET_LABEL_MAP))
        assert bool(((want["pred_class"] > 0) == (pred["label_ids"] > 0)).all()) and int(want["n_pred"].sum()) > 0
    a, e = captured.compute(), eager.compute()
    assert np.array_equal(a["ap"], e["ap"], equal_nan=True) and np.isfinite(a["ap"]).any()


# ---- 6. the file round trip ------------------------------------------------------------------------------------------------------------------

def test_files_give_what_the_tensors_give(ap_scenes, tmp_path):
    from gspn_amd.evaluate import InstanceAP, evaluate_files
    from gspn_amd.predict import write_ground_truth, write_predictions
    scenes = [dict(sc) for sc in ap_scenes[0][:3]]
    for sc in scenes:                                                               # the exporter writes rows of a class only: the others go behind count
        ok = np.array([k < sc["count"] and 1 <= sc["cls"][k] < C_AP for k in range(12)])
        order = np.concatenate((np.nonzero(ok)[0], np.nonzero(~ok)[0]))
        sc["masks"], sc["cls"], sc["conf"], sc["count"] = sc["masks"][order].copy(), sc["cls"][order], sc["conf"][order], int(ok.sum())
    scenes[0]["masks"][1] = 0                                                       # an empty mask: skipped by the exporter, the numbering goes on
    masks, cls, conf, count, seg, group = batch_tensors(scenes)
    seg = seg.clamp(0, C_AP - 1)                                                    # the exporter has no id for a label out of range
    group = group.clamp(0, G_AP - 1)
    metric = InstanceAP(C_AP, label_map=AP_MAP)
    metric.add(masks, cls, conf, count, seg, group, G_AP)
    want = metric.compute()
    table = torch.tensor(AP_MAP, dtype=torch.int32, device="cuda")
    pred = {"masks": masks, "label_ids": table[cls.clamp(0, C_AP - 1).long()], "confidence": conf, "count": count, "mask_points": masks.sum(-1).int()}
    scans = ["scene%04d_00" % i for i in range(3)]
    written = 0
    for i, scan in enumerate(scans):
        written += write_predictions(str(tmp_path / "pred"), scan, pred, i)
        write_ground_truth(str(tmp_path / "gt"), scan, seg[i], group[i], label_map=AP_MAP)
    assert written == int(count.sum()) - 1 and not os.path.exists(str(tmp_path / "pred" / "pred_mask" / "scene0000_00_1.txt"))
    got = evaluate_files(str(tmp_path / "pred"), str(tmp_path / "gt"), scans, label_map=AP_MAP)
    assert np.array_equal(got["ap"], want["ap"], equal_nan=True) and np.isfinite(got["ap"]).any()
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert got[k] == want[k]
    assert got["classes"] == want["classes"] or all(same(list(got["classes"][n].values()), list(want["classes"][n].values())) for n in got["classes"])
