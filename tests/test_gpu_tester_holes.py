"""GPU tests of mask holes through the layers above them, on the three synthetic scenes of 4096 points, scans of 9000
vertices and batch size of 2 that tests/test_gpu_tester_vertices.py uses.  The soft masks of the untrained network lie above the mask
threshold throughout, so a lifted row is every vertex of its planted box and has no unset vertex inside its own box: nothing to fill.
The driver here therefore knocks three in ten of the soft mask values out behind the network (punched), which leaves clusters of unset
vertices inside the rows, and the mesh is chunk_faces, short paths through vertices that lie close together, on which such rows enclose
many small gaps.  scan_predictions
without the arguments against the call with max_hole=None, with them against hole_fill applied by hand -- the fill works row by row, so
filling the rows in output order is filling them before the order; with the component filter and mask NMS the hand-made order is filter,
fill, NMS -- and against the numpy restatement; and Tester.run_vertices with and without 'faces'."""
import os

import numpy as np
import pytest
import torch

from tests import holes_ref as ref
from tests import test_gpu_inference as TI
from tests.test_gpu_tester import plant_boxes, read_tree, same_result
from tests.test_gpu_tester_vertices import ARGV, BATCH, SCENES, V, tool

pytestmark = pytest.mark.gpu

HOLE, HSHARE, MIN, SHARE, TH, CELL = 8, 0.5, 2, 0.0, 0.5, 0.25
SHARED = ("order", "count", "label_ids", "confidence", "sem_conf", "fb_conf", "score", "masks", "mask_points")


def clones(d):
    return {k: v.clone() for k, v in d.items()}


def chunk_faces(xyz):
    """(V, 3) -> faces: the vertices ordered by their cell of 0.1 and cut into chunks of 3 to 10, one path through each chunk"""
    cell = np.floor(np.asarray(xyz, np.float64) / 0.1).astype(np.int64)
    order = np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))
    faces, at, k = [], 0, 0
    while at < order.size - 1:
        n = 3 + k % 8
        part = order[at:at + n]
        faces.append(np.stack((part[:-1], part[1:], part[1:]), axis=1))
        at, k = at + n, k + 1
    return np.concatenate(faces).astype(np.int32)


def punched(outputs):
    """the step's outputs with three in ten of the soft mask values set to 0 and the others to 1, by a seeded draw; nothing else changed"""
    lift = dict(outputs["lift"])
    m = lift["rpointnet_mask_selected"]
    keep = (torch.rand(m.shape, generator=torch.Generator().manual_seed(5)) < 0.7).to(m.device)
    lift["rpointnet_mask_selected"] = keep.to(m.dtype)
    return dict(outputs, lift=lift)


def by_hand(pred, faces, xyz, filtered=False, nms=False):
    """component_filter, then hole_fill, then mask_nms, applied to a prediction dict from outside"""
    from gspn_amd.components import component_filter
    from gspn_amd.holes import hole_fill
    from gspn_amd.mask_nms import mask_nms
    out = clones(pred)
    m = pred["masks"][0].clone()
    if filtered:
        m, _, ncomp, nkept = component_filter(m, faces, min_vertices=MIN, min_share=SHARE)
        out["components"], out["components_kept"] = ncomp[None], nkept[None]
    m, points, nholes, nfilled = hole_fill(m, faces, xyz, max_vertices=HOLE, max_share=HSHARE)
    out["masks"], out["mask_points"], out["holes"], out["holes_filled"] = m[None], points[None], nholes[None], nfilled[None]
    if nms:
        out["masks"], out["keep"], out["mask_points"] = mask_nms(out["masks"], pred["count"], pred["label_ids"], iou_th=TH)
    return out


class Driver:
    """one Tester(max_hole=HOLE, max_hole_share=HSHARE) over the tool's synthetic scenes.  Computed once, shared, left unchanged."""

    def __init__(self, root):
        from gspn_amd.components import mesh_faces
        from gspn_amd.evaluate import InstanceAP
        from gspn_amd.lift import scan_predictions
        from gspn_amd.predict import SCANNET_LABEL_MAP
        from gspn_amd.tester import Tester
        from gspn_amd.train import DeviceDataset
        self.tool = tool()
        args = self.tool.parse(ARGV)
        cache = self.tool.synthetic_cache(args)
        self.label_map = SCANNET_LABEL_MAP[:TI.NCAT]
        data = DeviceDataset(*[cache[k].cuda() for k in self.tool.CACHE_KEYS], is_augment=False, permute_points=False)
        drawn = self.tool.synthetic_vertices(cache, V, args.seed)
        self.scans = lambda k: dict(drawn(k), faces=chunk_faces(drawn(k)["xyz"]))                      # noqa: E731
        t = self.tester = Tester(TI.small_config(), data, batch_size=BATCH, seed=TI.STORE_SEED, label_map=self.label_map, max_hole=HOLE,
                                 max_hole_share=HSHARE)
        assert (t.max_hole, t.max_hole_share, t.min_component) == (HOLE, HSHARE, None)
        plant_boxes(t.store)
        outputs = t._outputs
        t._outputs = lambda idx: punched(outputs(idx))                 # run_vertices and the calls below see the same rows
        self.plain, self.none, self.filled, self.all, self.faces, self.xyz = [], [], [], [], [], []
        metric = InstanceAP(TI.NCAT, label_map=self.label_map)
        for lo in range(0, SCENES, BATCH):
            idx = list(range(lo, min(lo + BATCH, SCENES)))
            lift = t._outputs(idx)["lift"]
            for s, k in enumerate(idx):
                scan = self.scans(k)
                xyz = torch.as_tensor(scan["xyz"]).cuda()
                faces = mesh_faces(scan["faces"], V)
                kw = dict(pc=t.buf["pc"], label_map=t.label_map, **t.thresholds)
                stage = dict(faces=faces, max_hole=HOLE, max_hole_share=HSHARE)
                self.faces.append(faces)
                self.xyz.append(xyz)
                self.plain.append(clones(scan_predictions(lift, s, xyz, **kw)))
                self.none.append(clones(scan_predictions(lift, s, xyz, faces=None, max_hole=None, **kw)))
                self.filled.append(clones(scan_predictions(lift, s, xyz, **kw, **stage)))
                self.all.append(clones(scan_predictions(lift, s, xyz, mask_nms_th=TH, min_component=MIN, min_component_share=SHARE, **kw, **stage)))
                group = torch.as_tensor(scan["group_label"]).cuda().int()
                metric.add_predictions(by_hand(self.plain[-1], faces, xyz), torch.as_tensor(scan["seg_label"]).cuda().int()[None], group[None],
                                       max(int(group.max()), 0) + 1)
        self.hand_result = metric.compute()
        no_faces = lambda k: {n: v for n, v in self.scans(k).items() if n != "faces"}                  # noqa: E731
        self.dirs = {name: os.path.join(root, name) for name in ("filled", "plain", "off")}
        self.results = {"filled": t.run_vertices(self.dirs["filled"], self.scans), "plain": t.run_vertices(self.dirs["plain"], no_faces)}
        t.max_hole = None
        self.results["off"] = t.run_vertices(self.dirs["off"], self.scans)         # faces, but the tester was not asked
        t.max_hole = HOLE


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return Driver(str(tmp_path_factory.mktemp("run_vertices_holes")))


def test_without_the_arguments_the_keys_and_the_bits_are_the_parent_s(driver):
    for plain, none in zip(driver.plain, driver.none):
        assert set(plain) == set(none) == set(SHARED) | {"src"}
        assert all(plain[k].dtype == none[k].dtype and torch.equal(plain[k], none[k]) for k in plain)


def check(plain, got, faces, xyz, extra, **stages):
    hand = by_hand(plain, faces, xyz, **stages)
    assert set(got) == set(hand) == set(SHARED) | {"holes", "holes_filled"} | extra
    for k in hand:
        assert got[k].dtype == hand[k].dtype and got[k].shape == hand[k].shape and torch.equal(got[k], hand[k]), k
    for k in set(SHARED) - {"masks", "mask_points"}:
        assert torch.equal(got[k], plain[k]), k                       # the confidences, the order, the score and the count are not touched
    assert got["holes"].dtype == got["holes_filled"].dtype == torch.int32 and got["holes"].shape == got["count"].shape + plain["masks"].shape[1:2]
    assert bool((got["holes"] >= 0).all())
    if not stages:
        want = ref.hole_fill_ref(plain["masks"][0].cpu().numpy(), faces.cpu().numpy(), xyz.cpu().numpy(), HOLE, HSHARE)
        for k, w in zip(("masks", "mask_points", "holes", "holes_filled"), want):
            assert np.array_equal(got[k][0].cpu().numpy(), w), k
        assert torch.equal(got["mask_points"], got["masks"].sum(-1).int())
    return int(got["holes_filled"].sum())


def test_the_arguments_are_hole_fill_behind_the_filter_before_the_order_and_before_mask_nms(driver):
    added = sum(check(p, g, f, x, {"src"}) for p, g, f, x in zip(driver.plain, driver.filled, driver.faces, driver.xyz))
    assert added > 0                                                  # vertices were filled: the case is not vacuous
    for p, g, f, x in zip(driver.plain, driver.all, driver.faces, driver.xyz):     # components -> holes -> mask NMS
        check(p, g, f, x, {"src", "keep", "components", "components_kept"}, filtered=True, nms=True)
    # the order matters on these scans: filling first and filtering then gives other rows somewhere
    from gspn_amd.components import component_filter
    from gspn_amd.holes import hole_fill
    differs = 0
    for p, f, x in zip(driver.plain, driver.faces, driver.xyz):
        m = p["masks"][0]
        a = hole_fill(component_filter(m, f, min_vertices=MIN, min_share=SHARE)[0], f, x, max_vertices=HOLE, max_share=HSHARE)[0]
        b = component_filter(hole_fill(m, f, x, max_vertices=HOLE, max_share=HSHARE)[0], f, min_vertices=MIN, min_share=SHARE)[0]
        differs += int((a != b).sum())
    print("filter then fill against fill then filter: %d vertices differ" % differs)


def test_run_vertices_fills_the_scans_that_bring_faces(driver):
    from gspn_amd.evaluate import evaluate_files
    trees = {name: read_tree(os.path.join(driver.dirs[name], "pred_vertices")) for name in driver.dirs}
    assert trees["plain"] == trees["off"] and trees["filled"] != trees["plain"]           # no 'faces', or no max_hole: as it always went
    assert same_result(driver.results["plain"], driver.results["off"])
    result, t = driver.results["filled"], driver.tester
    figures = {k: v for k, v in result.items() if k != "iou"}
    assert same_result(figures, driver.hand_result)                   # InstanceAP on the masks hole_fill leaves by hand
    assert same_result(figures, evaluate_files(os.path.join(driver.dirs["filled"], "pred_vertices"), os.path.join(driver.dirs["filled"], "gt_vertices"),
                                               t.scans, label_map=driver.label_map))
    assert result["iou"] == driver.results["plain"]["iou"]            # the semantic labels are not the stage's business
    ones = {name: sum(v.count(b"1") for k, v in trees[name].items() if k.startswith("pred_mask")) for name in trees}
    assert ones["filled"] == sum(int(g["mask_points"][0, :int(g["count"])].sum()) for g in driver.filled) > ones["plain"]
    print("per vertex: AP %.4f behind the hole fill (%d, %.2f), %.4f without" % (result["all_ap"], HOLE, HSHARE, driver.results["plain"]["all_ap"]))


def test_the_tester_checks_its_parameters_and_the_tool_runs_with_them(driver, tmp_path, capsys):
    from gspn_amd.tester import Tester
    from gspn_amd.train import save_variables
    t = driver.tester
    for kw in (dict(max_hole=-1), dict(max_hole=1.5), dict(max_hole=1, max_hole_share=1.5), dict(max_hole=1, max_hole_share=float("nan"))):
        with pytest.raises(ValueError, match="Tester: max_"):
            Tester(TI.small_config(), t.data, batch_size=BATCH, seed=TI.STORE_SEED, label_map=driver.label_map, **kw)
    path = save_variables(str(tmp_path / "model.ckpt"), t.store)
    out = str(tmp_path / "eva")
    argv = ARGV + ["--holes", str(HOLE), "--hole_share", str(HSHARE), "--segment_cell", str(CELL), "--model_path", path, "--out", out]
    result = driver.tool.main(argv)
    assert "AP: " in capsys.readouterr().out and set(result) == set(driver.results["filled"]) and 0.0 <= result["iou"] <= 1.0
    assert {k.split(os.sep)[0] for k in read_tree(out)} == {"pred_vertices", "gt_vertices"}
