"""GPU tests of mask NMS through the layers above it, on the three synthetic scenes of 4096 points, scans of 9000 vertices
and batch size of 2 that tests/test_gpu_tester_vertices.py uses.  A freshly initialised network rarely detects one object twice, so the
step's outputs pass through `doubled`, which copies every even detection row -- box, class, score, crop and mask values -- onto the odd
row behind it: every detection then has an exact duplicate that the box NMS did not see.  scan_predictions and scene_predictions with
mask_nms_th=None against the calls without the argument, with a threshold against mask_nms applied by hand and against the numpy
restatement, and Tester.run_vertices with and without the threshold."""
import os

import numpy as np
import pytest
import torch

from tests import mask_nms_ref as ref
from tests import test_gpu_inference as TI
from tests.test_gpu_tester import plant_boxes, read_tree, same_result
from tests.test_gpu_tester_vertices import ARGV, BATCH, SCENES, V, tool

pytestmark = pytest.mark.gpu

TH, CELL = 0.5, 0.25
SHARED = ("order", "count", "label_ids", "confidence", "sem_conf", "fb_conf", "score", "masks", "mask_points")
DOUBLED = ("detections", "rpointnet_mask_selected", "pc_coord_cropped_final_unnormalized")


def clones(d):
    return {k: v.clone() for k, v in d.items()}


def by_hand(pred):
    """mask_nms applied to a prediction dict from outside -> the dict scan_predictions / scene_predictions must return with the threshold"""
    from gspn_amd.mask_nms import mask_nms
    out = clones(pred)
    out["masks"], out["keep"], out["mask_points"] = mask_nms(pred["masks"].clone(), pred["count"], pred["label_ids"], iou_th=TH)
    return out


class Driver:
    """one Tester(mask_nms_th=TH) over the tool's synthetic scenes, seeing the doubled outputs; its run without the stage is made with the
    attribute set to None for that run.  Computed once, shared, left unchanged."""

    def __init__(self, root):
        from gspn_amd.evaluate import InstanceAP
        from gspn_amd.lift import scan_predictions
        from gspn_amd.predict import SCANNET_LABEL_MAP, scene_predictions
        from gspn_amd.segments import compact_segments
        from gspn_amd.tester import Tester
        from gspn_amd.train import DeviceDataset
        self.tool = tool()
        args = self.tool.parse(ARGV)
        cache = self.tool.synthetic_cache(args)
        self.label_map = SCANNET_LABEL_MAP[:TI.NCAT]
        data = DeviceDataset(*[cache[k].cuda() for k in self.tool.CACHE_KEYS], is_augment=False, permute_points=False)
        self.scans = self.tool.synthetic_vertices(cache, V, args.seed, CELL)
        t = self.tester = Tester(TI.small_config(), data, batch_size=BATCH, seed=TI.STORE_SEED, label_map=self.label_map, mask_nms_th=TH)
        assert t.mask_nms_th == TH
        plant_boxes(t.store)
        t._outputs = self.doubled(t._outputs)
        self.scene, self.scan, self.voted = [], [], []                # per batch / per scene: (without the argument, with None, with TH)
        metric = InstanceAP(TI.NCAT, label_map=self.label_map)
        for lo in range(0, SCENES, BATCH):
            idx = list(range(lo, min(lo + BATCH, SCENES)))
            lift = t._outputs(idx)["lift"]
            kw = dict(label_map=t.label_map, **t.thresholds)
            self.scene.append(tuple(clones(scene_predictions(lift, t.buf["pc"], **kw, **extra)) for extra in ({}, dict(mask_nms_th=None), dict(mask_nms_th=TH))))
            for s, k in enumerate(idx):
                scan = self.scans(k)
                xyz = torch.as_tensor(scan["xyz"]).cuda()
                seg, nseg = compact_segments(torch.as_tensor(scan["segments"]).cuda())
                kw = dict(pc=t.buf["pc"], label_map=t.label_map, **t.thresholds)
                trio = tuple(clones(scan_predictions(lift, s, xyz, **kw, **extra)) for extra in ({}, dict(mask_nms_th=None), dict(mask_nms_th=TH)))
                self.scan.append(trio)
                self.voted.append(tuple(clones(scan_predictions(lift, s, xyz, segments=seg, num_segments=nseg, **kw, **extra))
                                        for extra in ({}, dict(mask_nms_th=TH))))
                group = torch.as_tensor(scan["group_label"]).cuda().int()
                metric.add_predictions(by_hand(trio[0]), torch.as_tensor(scan["seg_label"]).cuda().int()[None], group[None], max(int(group.max()), 0) + 1)
        self.hand_result = metric.compute()
        plain = lambda k: {n: v for n, v in self.scans(k).items() if n != "segments"}          # noqa: E731
        self.dirs = {name: os.path.join(root, name) for name in ("nms", "plain")}
        self.results = {"nms": t.run_vertices(self.dirs["nms"], plain)}
        t.mask_nms_th = None
        self.results["plain"] = t.run_vertices(self.dirs["plain"], plain)
        t.mask_nms_th = TH

    @staticmethod
    def doubled(step_outputs):
        def outputs(idx):
            out = dict(step_outputs(idx))
            lift = dict(out["lift"])
            for k in DOUBLED:
                t = lift[k].clone()
                pairs = t.shape[1] // 2
                t[:, 1:2 * pairs:2] = t[:, 0:2 * pairs:2]
                lift[k] = t
            out["lift"] = lift
            return out
        return outputs


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return Driver(str(tmp_path_factory.mktemp("run_vertices_mask_nms")))


def test_none_leaves_the_keys_and_the_bits(driver):
    for without, none, _ in driver.scene:
        assert set(without) == set(none) == set(SHARED)
        assert all(without[k].dtype == none[k].dtype and torch.equal(without[k], none[k]) for k in SHARED)
    for without, none, _ in driver.scan:
        assert set(without) == set(none) == set(SHARED) | {"src"}
        assert all(without[k].dtype == none[k].dtype and torch.equal(without[k], none[k]) for k in without)


def check(plain, got, extra):
    """got = plain with mask_nms applied by hand, and by the numpy restatement"""
    hand = by_hand(plain)
    assert set(got) == set(hand) == set(SHARED) | {"keep"} | extra
    for k in hand:
        assert got[k].dtype == hand[k].dtype and torch.equal(got[k], hand[k]), k
    for k in set(SHARED) - {"masks", "mask_points"}:
        assert torch.equal(got[k], plain[k]), k                       # the confidences, the order, the score and the count are not touched
    want = ref.mask_nms_batch_ref(plain["masks"].cpu().numpy(), plain["count"].cpu().numpy(), plain["label_ids"].cpu().numpy(), TH)
    for k, w in zip(("masks", "keep", "mask_points"), want):
        assert np.array_equal(got[k].cpu().numpy(), w), k
    assert got["keep"].dtype == torch.uint8 and torch.equal(got["mask_points"], got["masks"].sum(-1).int())
    return int(plain["count"].sum()) - int(got["keep"].sum())


def test_a_threshold_is_mask_nms_on_the_rows_in_output_order(driver):
    gone = sum(check(plain, got, set()) for plain, _, got in driver.scene)
    gone += sum(check(plain, got, {"src"}) for plain, _, got in driver.scan)
    gone += sum(check(plain, got, {"src", "sem_label"}) for plain, got in driver.voted)            # behind the segment vote
    assert gone > 0                                                   # the doubled detections were found: the case is not vacuous


def test_run_vertices_with_a_threshold_writes_fewer_files_and_their_figures(driver):
    from gspn_amd import tester as T
    from gspn_amd.evaluate import evaluate_files
    trees = {name: read_tree(os.path.join(driver.dirs[name], "pred_vertices")) for name in driver.dirs}
    masks = {name: sorted(k for k in trees[name] if k.startswith("pred_mask")) for name in trees}
    assert 0 < len(masks["nms"]) < len(masks["plain"])
    kept = sum(int(got["keep"].sum()) for _, _, got in driver.scan)   # one file per kept row that is not empty
    written = sum(int(((got["keep"] != 0) & (got["mask_points"] > 0)).sum()) for _, _, got in driver.scan)
    assert len(masks["nms"]) == written <= kept
    assert all(trees["nms"][k].count(b"\n") == V and b"1" in trees["nms"][k] for k in masks["nms"])
    gt = {name: read_tree(os.path.join(driver.dirs[name], "gt_vertices")) for name in driver.dirs}
    assert gt["nms"] == gt["plain"] and len(gt["nms"]) == SCENES
    result, t = driver.results["nms"], driver.tester
    figures = {k: v for k, v in result.items() if k != "iou"}
    assert same_result(figures, driver.hand_result)                   # InstanceAP on the masks mask_nms leaves by hand
    assert same_result(figures, evaluate_files(os.path.join(driver.dirs["nms"], "pred_vertices"), os.path.join(driver.dirs["nms"], "gt_vertices"),
                                               t.scans, label_map=driver.label_map))
    assert result["iou"] == driver.results["plain"]["iou"]            # the semantic labels are not the stage's business
    assert T.RESULT_FILE in trees["nms"]
    print("per vertex, doubled detections: AP %.4f with mask NMS at %.2f (%d files), %.4f without (%d files)"
          % (result["all_ap"], TH, len(masks["nms"]), driver.results["plain"]["all_ap"], len(masks["plain"])))


def test_the_tester_checks_its_threshold_and_the_tool_runs_with_it(driver, tmp_path, capsys):
    from gspn_amd.tester import Tester
    from gspn_amd.train import save_variables
    t = driver.tester
    for th in (1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match=r"mask_nms_th must lie in \[0, 1\)"):
            Tester(TI.small_config(), t.data, batch_size=BATCH, seed=TI.STORE_SEED, label_map=driver.label_map, mask_nms_th=th)
    path = save_variables(str(tmp_path / "model.ckpt"), t.store)
    out = str(tmp_path / "eva")
    argv = ARGV + ["--segments", "--segment_cell", str(CELL), "--mask_nms", str(TH), "--model_path", path, "--out", out]
    assert driver.tool.parse(argv).mask_nms == TH
    result = driver.tool.main(argv)
    assert "AP: " in capsys.readouterr().out and set(result) == set(driver.results["nms"]) and 0.0 <= result["iou"] <= 1.0
    tree = read_tree(out)
    assert {k.split(os.sep)[0] for k in tree} == {"pred_vertices", "gt_vertices"}
