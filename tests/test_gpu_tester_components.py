"""GPU tests of mask components through the layers above them, on the three synthetic scenes of 4096 points, scans of 9000
vertices and batch size of 2 that tests/test_gpu_tester_vertices.py uses, with synth.scan_faces as each scan's mesh.  scan_predictions
without the arguments against the call with faces=None, with them against component_filter applied by hand -- the filter works row by
row, so filtering the rows in output order is filtering them before the order; with mask NMS the hand-made order is filter, then NMS --
and against the numpy restatement, with and without segments; and Tester.run_vertices with and without 'faces'."""
import os

import numpy as np
import pytest
import torch

from tests import components_ref as ref
from tests import test_gpu_inference as TI
from tests.test_gpu_tester import plant_boxes, read_tree, same_result
from tests.test_gpu_tester_vertices import ARGV, BATCH, SCENES, V, tool

pytestmark = pytest.mark.gpu

MIN, SHARE, TH, CELL = 30, 0.25, 0.5, 0.25
SHARED = ("order", "count", "label_ids", "confidence", "sem_conf", "fb_conf", "score", "masks", "mask_points")


def clones(d):
    return {k: v.clone() for k, v in d.items()}


def by_hand(pred, faces, nms=False):
    """component_filter, and then mask_nms, applied to a prediction dict from outside"""
    from gspn_amd.components import component_filter
    from gspn_amd.mask_nms import mask_nms
    out = clones(pred)
    m, points, ncomp, nkept = component_filter(pred["masks"][0].clone(), faces, min_vertices=MIN, min_share=SHARE)
    out["masks"], out["mask_points"], out["components"], out["components_kept"] = m[None], points[None], ncomp[None], nkept[None]
    if nms:
        out["masks"], out["keep"], out["mask_points"] = mask_nms(out["masks"], pred["count"], pred["label_ids"], iou_th=TH)
    return out


class Driver:
    """one Tester(min_component=MIN, min_component_share=SHARE) over the tool's synthetic scenes.  Computed once, shared, left unchanged."""

    def __init__(self, root):
        from gspn_amd.components import mesh_faces
        from gspn_amd.evaluate import InstanceAP
        from gspn_amd.lift import scan_predictions
        from gspn_amd.predict import SCANNET_LABEL_MAP
        from gspn_amd.segments import compact_segments
        from gspn_amd.tester import Tester
        from gspn_amd.train import DeviceDataset
        self.tool = tool()
        args = self.tool.parse(ARGV)
        cache = self.tool.synthetic_cache(args)
        self.label_map = SCANNET_LABEL_MAP[:TI.NCAT]
        data = DeviceDataset(*[cache[k].cuda() for k in self.tool.CACHE_KEYS], is_augment=False, permute_points=False)
        self.scans = self.tool.synthetic_vertices(cache, V, args.seed, CELL, CELL)
        t = self.tester = Tester(TI.small_config(), data, batch_size=BATCH, seed=TI.STORE_SEED, label_map=self.label_map, min_component=MIN,
                                 min_component_share=SHARE)
        assert (t.min_component, t.min_component_share) == (MIN, SHARE)
        plant_boxes(t.store)
        self.plain, self.none, self.cleaned, self.both, self.voted, self.faces = [], [], [], [], [], []
        metric = InstanceAP(TI.NCAT, label_map=self.label_map)
        for lo in range(0, SCENES, BATCH):
            idx = list(range(lo, min(lo + BATCH, SCENES)))
            lift = t._outputs(idx)["lift"]
            for s, k in enumerate(idx):
                scan = self.scans(k)
                xyz = torch.as_tensor(scan["xyz"]).cuda()
                faces = mesh_faces(scan["faces"], V)
                seg, nseg = compact_segments(torch.as_tensor(scan["segments"]).cuda())
                kw = dict(pc=t.buf["pc"], label_map=t.label_map, **t.thresholds)
                stage = dict(faces=faces, min_component=MIN, min_component_share=SHARE)
                self.faces.append(faces)
                self.plain.append(clones(scan_predictions(lift, s, xyz, **kw)))
                self.none.append(clones(scan_predictions(lift, s, xyz, faces=None, min_component=None, **kw)))
                self.cleaned.append(clones(scan_predictions(lift, s, xyz, **kw, **stage)))
                self.both.append(clones(scan_predictions(lift, s, xyz, mask_nms_th=TH, **kw, **stage)))
                self.voted.append(tuple(clones(scan_predictions(lift, s, xyz, segments=seg, num_segments=nseg, **kw, **extra)) for extra in ({}, stage)))
                group = torch.as_tensor(scan["group_label"]).cuda().int()
                metric.add_predictions(by_hand(self.plain[-1], faces), torch.as_tensor(scan["seg_label"]).cuda().int()[None], group[None],
                                       max(int(group.max()), 0) + 1)
        self.hand_result = metric.compute()
        no_segments = lambda k: {n: v for n, v in self.scans(k).items() if n != "segments"}            # noqa: E731
        no_faces = lambda k: {n: v for n, v in self.scans(k).items() if n not in ("segments", "faces")}    # noqa: E731
        self.dirs = {name: os.path.join(root, name) for name in ("cleaned", "plain", "off")}
        self.results = {"cleaned": t.run_vertices(self.dirs["cleaned"], no_segments), "plain": t.run_vertices(self.dirs["plain"], no_faces)}
        t.min_component = None
        self.results["off"] = t.run_vertices(self.dirs["off"], no_segments)        # faces, but the tester was not asked
        t.min_component = MIN


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return Driver(str(tmp_path_factory.mktemp("run_vertices_components")))


def test_without_the_arguments_the_keys_and_the_bits_are_the_parent_s(driver):
    for plain, none in zip(driver.plain, driver.none):
        assert set(plain) == set(none) == set(SHARED) | {"src"}
        assert all(plain[k].dtype == none[k].dtype and torch.equal(plain[k], none[k]) for k in plain)


def check(plain, got, faces, extra, nms=False):
    hand = by_hand(plain, faces, nms)
    assert set(got) == set(hand) == set(SHARED) | {"components", "components_kept"} | extra
    for k in hand:
        assert got[k].dtype == hand[k].dtype and got[k].shape == hand[k].shape and torch.equal(got[k], hand[k]), k
    for k in set(SHARED) - {"masks", "mask_points"}:
        assert torch.equal(got[k], plain[k]), k                       # the confidences, the order, the score and the count are not touched
    assert got["components"].dtype == got["components_kept"].dtype == torch.int32 and got["components"].shape == got["count"].shape + plain["masks"].shape[1:2]
    assert bool((got["components"] >= 0).all())
    if not nms:
        want = ref.component_filter_ref(plain["masks"][0].cpu().numpy(), faces.cpu().numpy(), MIN, SHARE)
        for k, w in zip(("masks", "mask_points", "components", "components_kept"), want):
            assert np.array_equal(got[k][0].cpu().numpy(), w), k
        assert torch.equal(got["mask_points"], got["masks"].sum(-1).int())
    return int(plain["mask_points"].sum()) - int(got["mask_points"].sum())


def test_the_arguments_are_component_filter_before_the_order_and_before_mask_nms(driver):
    gone = sum(check(p, g, f, {"src"}) for p, g, f in zip(driver.plain, driver.cleaned, driver.faces))
    assert gone > 0                                                   # vertices were dropped: the case is not vacuous
    gone = sum(check(p, g, f, {"src", "sem_label"}) for (p, g), f in zip(driver.voted, driver.faces))          # behind the segment vote
    assert gone > 0
    for p, g, f in zip(driver.plain, driver.both, driver.faces):      # mask NMS sees the cleaned rows
        check(p, g, f, {"src", "keep"}, nms=True)


def test_run_vertices_cleans_the_scans_that_bring_faces(driver):
    from gspn_amd.evaluate import evaluate_files
    trees = {name: read_tree(os.path.join(driver.dirs[name], "pred_vertices")) for name in driver.dirs}
    assert trees["plain"] == trees["off"] and trees["cleaned"] != trees["plain"]          # no 'faces', or no min_component: as it always went
    assert same_result(driver.results["plain"], driver.results["off"])
    result, t = driver.results["cleaned"], driver.tester
    figures = {k: v for k, v in result.items() if k != "iou"}
    assert same_result(figures, driver.hand_result)                   # InstanceAP on the masks component_filter leaves by hand
    assert same_result(figures, evaluate_files(os.path.join(driver.dirs["cleaned"], "pred_vertices"), os.path.join(driver.dirs["cleaned"], "gt_vertices"),
                                               t.scans, label_map=driver.label_map))
    assert result["iou"] == driver.results["plain"]["iou"]            # the semantic labels are not the stage's business
    ones = {name: sum(v.count(b"1") for k, v in trees[name].items() if k.startswith("pred_mask")) for name in trees}
    assert ones["cleaned"] == sum(int(g["mask_points"][0, :int(g["count"])].sum()) for g in driver.cleaned) < ones["plain"]
    print("per vertex: AP %.4f behind the component filter (%d, %.2f), %.4f without" % (result["all_ap"], MIN, SHARE, driver.results["plain"]["all_ap"]))


def test_the_tester_checks_its_parameters_and_the_tool_runs_with_them(driver, tmp_path, capsys):
    from gspn_amd.tester import Tester
    from gspn_amd.train import save_variables
    t = driver.tester
    for kw in (dict(min_component=0), dict(min_component=1.5), dict(min_component=1, min_component_share=1.5),
               dict(min_component=1, min_component_share=float("nan"))):
        with pytest.raises(ValueError, match="Tester: min_"):
            Tester(TI.small_config(), t.data, batch_size=BATCH, seed=TI.STORE_SEED, label_map=driver.label_map, **kw)
    path = save_variables(str(tmp_path / "model.ckpt"), t.store)
    out = str(tmp_path / "eva")
    argv = ARGV + ["--segments", "--segment_cell", str(CELL), "--components", str(MIN), "--component_share", str(SHARE), "--model_path", path, "--out", out]
    result = driver.tool.main(argv)
    assert "AP: " in capsys.readouterr().out and set(result) == set(driver.results["cleaned"]) and 0.0 <= result["iou"] <= 1.0
    assert {k.split(os.sep)[0] for k in read_tree(out)} == {"pred_vertices", "gt_vertices"}
