"""GPU tests of the segment vote through the layers above it, on the three synthetic scenes of 4096 points, scans of 9000
vertices and batch size of 2 that tests/test_gpu_tester_vertices.py uses: lift.scan_predictions with segments against lift_masks ->
segment_vote -> scene_rank composed by hand, singleton segments against the call without segments, and Tester.run_vertices with and
without 'segments' -- the run without, made before any segmented run, is what a later run without must reproduce byte for byte."""
import os

import numpy as np
import pytest
import torch

from tests import segments_ref as ref
from tests import test_gpu_inference as TI
from tests.test_gpu_tester import plant_boxes, read_tree, same_result
from tests.test_gpu_tester_vertices import ARGV, BATCH, SCENES, V, tool

pytestmark = pytest.mark.gpu

CELL, VOTE_TH = 0.25, 0.5
SHARED = ("order", "count", "label_ids", "confidence", "sem_conf", "fb_conf", "score", "masks", "mask_points", "src")


def hand_composition(t, lift, s, scan):
    """scan_predictions with segments, step by step -> (its dict, sem_label by the numpy restatement)"""
    from gspn_amd.lift import lift_masks, vertex_tables
    from gspn_amd.predict import scene_rank
    from gspn_amd.segments import compact_segments, segment_vote
    th = t.thresholds
    xyz = torch.as_tensor(scan["xyz"]).cuda()
    seg, nseg = compact_segments(torch.as_tensor(scan["segments"]).cuda())
    det, logits = lift["detections"][s], lift["sem_class_logits"]
    src, vert_fb = vertex_tables(xyz, t.buf["pc"][s], lift["pc_seed"][s], lift["fb_prob"][s])
    sem_prob = torch.softmax(logits[s:s + 1], -1)[0]
    class_ids = det[:, 6].int()
    sem_conf, fb_conf, mask, points = lift_masks(xyz, lift["pc_coord_cropped_final_unnormalized"][s], det[:, :6], lift["rpointnet_mask_selected"][s],
                                                 class_ids, src, sem_prob, vert_fb, th["mask_th"])
    mask, points = segment_vote(mask, seg, nseg, VOTE_TH)
    order, count, label_ids, confidence, score = scene_rank(det[None, :, 7], class_ids[None], sem_conf[None], fb_conf[None], th["sem_conf_th"],
                                                            th["fb_conf_th"], t.label_map)
    at = order[0].long()
    pred = {"order": order, "count": count, "label_ids": label_ids, "confidence": confidence, "sem_conf": sem_conf[at][None],
            "fb_conf": fb_conf[at][None], "score": score, "masks": mask[at][None], "mask_points": points[at][None], "src": src}
    own = np.argmax(logits[s].cpu().numpy()[src.cpu().numpy()], axis=-1)                                # np.argmax: the first maximum
    sem_label = ref.segment_label_vote_ref(own, seg.cpu().numpy(), nseg, logits.shape[2])
    return {k: v.clone() for k, v in pred.items()}, sem_label


class Driver:
    """one Tester over the tool's synthetic scenes.  run_vertices without segments comes first, before any segmented run; then, batch by
    batch as run_vertices forms them, scan_predictions with segments beside the composition by hand, whose files are written; then
    run_vertices with segments.  Computed once, shared, left unchanged.

    A freshly initialised semantic head says class 0 at every point, which would make every statement about labels hold trivially: for
    the segmented part the step's outputs pass through `planted`, which puts seeded random logits in the place of sem_class_logits
    (several classes win, segments hold mixed votes and ties).  The runs without segments see the step's own outputs."""

    def __init__(self, root):
        from gspn_amd.lift import scan_predictions
        from gspn_amd.predict import SCANNET_LABEL_MAP, mean_iou, write_predictions
        from gspn_amd.segments import compact_segments
        from gspn_amd.tester import Tester
        from gspn_amd.train import DeviceDataset
        self.tool = tool()
        args = self.tool.parse(ARGV)
        cache = self.tool.synthetic_cache(args)
        self.label_map = SCANNET_LABEL_MAP[:TI.NCAT]
        data = DeviceDataset(*[cache[k].cuda() for k in self.tool.CACHE_KEYS], is_augment=False, permute_points=False)
        t = self.tester = Tester(TI.small_config(), data, batch_size=BATCH, seed=TI.STORE_SEED, label_map=self.label_map, vote_th=VOTE_TH)
        plant_boxes(t.store)
        self.plain = self.tool.synthetic_vertices(cache, V, args.seed)
        self.segmented = self.tool.synthetic_vertices(cache, V, args.seed, CELL)
        self.before = os.path.join(root, "before")
        self.before_result = t.run_vertices(self.before, self.plain)

        step_outputs = t._outputs

        def planted(idx):
            out = dict(step_outputs(idx))
            lift = dict(out["lift"])
            gen = torch.Generator(device="cuda").manual_seed(1000 + idx[0])
            lift["sem_class_logits"] = torch.randn(lift["sem_class_logits"].shape, generator=gen, device="cuda") * 3.0
            out["lift"] = lift
            return out

        t._outputs = planted

        self.hand_dir = os.path.join(root, "hand")
        os.makedirs(self.hand_dir)
        self.pairs = []                                               # per scene: scan_predictions' dict, the hand's, the hand's labels, the labels before the vote
        self.identity = []                                            # per scene: scan_predictions with singleton segments, and without any
        inter = torch.zeros(TI.NCAT - 1, dtype=torch.int64, device="cuda")
        union = torch.zeros(TI.NCAT - 1, dtype=torch.int64, device="cuda")
        for lo in range(0, SCENES, BATCH):
            idx = list(range(lo, min(lo + BATCH, SCENES)))
            lift = planted(idx)["lift"]
            for s, k in enumerate(idx):
                scan = self.segmented(k)
                xyz = torch.as_tensor(scan["xyz"]).cuda()
                seg, nseg = compact_segments(torch.as_tensor(scan["segments"]).cuda())
                kw = dict(pc=t.buf["pc"], label_map=t.label_map, **t.thresholds)
                got = scan_predictions(lift, s, xyz, segments=seg, num_segments=nseg, vote_th=VOTE_TH, **kw)
                hand, labels = hand_composition(t, lift, s, scan)
                own = np.argmax(lift["sem_class_logits"][s].cpu().numpy()[got["src"].cpu().numpy()], axis=-1)        # the labels before the vote
                self.pairs.append(({n: v.clone() for n, v in got.items()}, hand, labels, own))
                write_predictions(self.hand_dir, t.scans[k], hand, 0)
                single = scan_predictions(lift, s, xyz, segments=torch.arange(V, dtype=torch.int32, device="cuda"), num_segments=V, **kw)
                self.identity.append(({n: v.clone() for n, v in single.items()}, {n: v.clone() for n, v in scan_predictions(lift, s, xyz, **kw).items()}))
                truth = np.asarray(scan["seg_label"])
                for c in range(1, TI.NCAT):
                    inter[c - 1] += int(((labels == c) & (truth == c)).sum())
                    union[c - 1] += int(((labels == c) | (truth == c)).sum())
        self.hand_iou = float(mean_iou(inter, union))
        self.voted = os.path.join(root, "voted")
        self.voted_result = t.run_vertices(self.voted, self.segmented)
        del t._outputs                                                # the step's own outputs again


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return Driver(str(tmp_path_factory.mktemp("run_vertices_segments")))


def test_scan_predictions_with_segments_is_the_composition_by_hand(driver):
    changed = 0
    for got, hand, labels, own in driver.pairs:
        assert set(got) == set(SHARED) | {"sem_label"}
        for k in SHARED:
            assert got[k].dtype == hand[k].dtype and torch.equal(got[k], hand[k]), k
        assert got["sem_label"].dtype == torch.int32 and np.array_equal(got["sem_label"].cpu().numpy(), labels)
        assert np.unique(labels).size > 1 and 0 < int((own != labels).sum()) < V                  # a vote that has something to decide
        assert torch.equal(got["mask_points"][0], got["masks"][0].sum(1).int())
    for (got, _, _, _), (_, plain) in zip(driver.pairs, driver.identity):
        for k in ("order", "count", "label_ids", "confidence", "sem_conf", "fb_conf", "score", "src"):
            assert torch.equal(got[k], plain[k]), k                   # the vote touches the hard masks and nothing else
        changed += int((got["masks"] != plain["masks"]).sum())
    assert changed > 0                                                # and it does touch them: the case is not vacuous


def test_singleton_segments_give_the_predictions_without_segments(driver):
    for single, plain in driver.identity:
        assert set(plain) == set(SHARED) and set(single) == set(SHARED) | {"sem_label"}
        for k in SHARED:
            assert single[k].dtype == plain[k].dtype and torch.equal(single[k], plain[k]), k


def test_run_vertices_with_segments_writes_the_files_of_the_composition(driver):
    from gspn_amd import tester as T
    from gspn_amd.evaluate import evaluate_files
    t = driver.tester
    voted, hand, before = read_tree(os.path.join(driver.voted, "pred_vertices")), read_tree(driver.hand_dir), read_tree(driver.before)
    assert sorted(k for k in voted if k != T.RESULT_FILE) == sorted(hand) and all(voted[k] == hand[k] for k in hand)
    gt = read_tree(os.path.join(driver.voted, "gt_vertices"))
    assert all(gt[k] == before[os.path.join("gt_vertices", k)] for k in gt) and len(gt) == SCENES
    masks = [k for k in hand if k.startswith("pred_mask")]
    assert masks and all(hand[k].count(b"\n") == V for k in masks)
    assert any(hand[k] != before.get(os.path.join("pred_vertices", k)) for k in masks)                  # the vote changed something
    result = driver.voted_result
    figures = {k: v for k, v in result.items() if k != "iou"}
    assert same_result(figures, evaluate_files(os.path.join(driver.voted, "pred_vertices"), os.path.join(driver.voted, "gt_vertices"), t.scans,
                                               label_map=driver.label_map))
    assert result["iou"] == driver.hand_iou and 0.0 < result["iou"] < 1.0                               # the IoU counts come from the voted labels
    print("voted: AP %.4f mean IoU %.4f; not voted: AP %.4f mean IoU %.4f" % (result["all_ap"], result["iou"], driver.before_result["all_ap"],
                                                                           driver.before_result["iou"]))


def test_a_scan_without_segments_goes_the_old_way(driver, tmp_path):
    t = driver.tester
    again = t.run_vertices(str(tmp_path / "after"), driver.plain)     # after the segmented runs, on the same tester
    a, w = read_tree(str(tmp_path / "after")), read_tree(driver.before)
    assert sorted(a) == sorted(w) and all(a[k] == w[k] for k in w) and same_result(again, driver.before_result)
    with pytest.raises(ValueError, match="must name the segment of each of its %d vertices" % V):
        t.run_vertices(None, lambda k: dict(driver.segmented(k), segments=driver.segmented(k)["segments"][:100]))
    with pytest.raises(ValueError, match=r"vote_th must lie in \[0, 1\)"):
        from gspn_amd.tester import Tester
        Tester(TI.small_config(), t.data, batch_size=BATCH, seed=TI.STORE_SEED, label_map=driver.label_map, vote_th=1.0)


def test_the_tool_runs_with_segments(driver, tmp_path, capsys):
    from gspn_amd.train import save_variables
    path = save_variables(str(tmp_path / "model.ckpt"), driver.tester.store)
    out = str(tmp_path / "eva")
    argv = ARGV + ["--segments", "--segment_cell", str(CELL), "--vote_th", str(VOTE_TH), "--model_path", path, "--out", out]
    a = driver.tool.parse(argv)
    assert a.segments and (a.vote_th, a.segment_cell) == (VOTE_TH, CELL)
    result = driver.tool.main(argv)
    assert "AP: " in capsys.readouterr().out and set(result) == set(driver.voted_result) and 0.0 <= result["iou"] <= 1.0
    tree = read_tree(out)
    assert {k.split(os.sep)[0] for k in tree} == {"pred_vertices", "gt_vertices"}
    masks = [k for k in tree if k.startswith(os.path.join("pred_vertices", "pred_mask"))]
    assert all(tree[k].count(b"\n") == V and set(tree[k]) <= set(b"01\n") for k in masks)
