"""GPU tests of Tester.run_vertices and the vertex flags of tools/test.py, on three synthetic scenes of 4096 points with
synthetic scans of 9000 vertices around them and a batch size of 2 -- a short last batch: one line per vertex in every file written, the
figures against evaluate_files on those files, run()'s own outputs and the variable store untouched by the call, the scene's own points as
the scan giving run()'s files byte for byte, and the tool end to end."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_inference as TI
from tests.test_gpu_tester import plant_boxes, read_tree, same_result, same_store, snapshot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES, BATCH, V = 3, 2, 9000
ARGV = ["--synthetic", str(SCENES), "--num_point", "4096", "--num_point_ins", "512", "--num_category", str(TI.NCAT), "--num_sample", str(TI.NSMP),
        "--num_group", str(TI.NGROUP), "--batch_size", str(BATCH), "--seed", str(TI.STORE_SEED), "--synthetic_vertices", str(V)]


def tool():
    spec = importlib.util.spec_from_file_location("tools_test", os.path.join(ROOT, "tools", "test.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class Driver:
    """one Tester over the tool's synthetic scenes, run() once before anything else: computed once, shared, left unchanged"""

    def __init__(self, root):
        from gspn_amd.predict import SCANNET_LABEL_MAP
        from gspn_amd.tester import Tester
        from gspn_amd.train import DeviceDataset
        self.tool = tool()
        self.args = self.tool.parse(ARGV)
        self.cache = self.tool.synthetic_cache(self.args)
        self.label_map = SCANNET_LABEL_MAP[:TI.NCAT]
        data = DeviceDataset(*[self.cache[k].cuda() for k in self.tool.CACHE_KEYS], is_augment=False, permute_points=False)
        self.tester = Tester(TI.small_config(), data, batch_size=BATCH, seed=TI.STORE_SEED, label_map=self.label_map)
        plant_boxes(self.tester.store)
        self.vertices = self.tool.synthetic_vertices(self.cache, V, self.args.seed)
        self.first = os.path.join(root, "first")
        self.result = self.tester.run(out_dir=self.first)
        self.store = snapshot(self.tester.store)
        self.out = os.path.join(root, "vertices")
        self.vertex_result = self.tester.run_vertices(self.out, self.vertices)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return Driver(str(tmp_path_factory.mktemp("run_vertices")))


def lines(data):
    return data.count(b"\n")


def test_run_vertices_writes_one_line_per_vertex_and_the_figures_of_its_files(driver):
    from gspn_amd import tester as T
    from gspn_amd.evaluate import evaluate_files
    t = driver.tester
    tree = read_tree(driver.out)
    pred_dir, gt_dir = os.path.join(driver.out, "pred_vertices"), os.path.join(driver.out, "gt_vertices")
    assert {k.split(os.sep)[0] for k in tree} == {"pred_vertices", "gt_vertices"}
    for scan in t.scans:                                                            # every scene once, the filled slot of the last batch never
        assert lines(tree[os.path.join("gt_vertices", scan + ".txt")]) == V
        assert os.path.join("pred_vertices", scan + ".txt") in tree
    masks = [k for k in tree if k.startswith(os.path.join("pred_vertices", "pred_mask"))]
    assert len(masks) > 0 and all(lines(tree[k]) == V and set(tree[k]) <= set(b"01\n") for k in masks)
    named = sum(lines(tree[os.path.join("pred_vertices", scan + ".txt")]) for scan in t.scans)
    assert named == len(masks) and len(tree) == 2 * SCENES + len(masks) + 1
    result_file = tree[os.path.join("pred_vertices", T.RESULT_FILE)]
    assert result_file.startswith(b"class,class id,ap,ap50,ap25\n") and lines(result_file) == TI.NCAT
    # the ground truth is the generator's
    for k, scan in enumerate(t.scans):
        labels = driver.vertices(k)
        want = "".join("%d\n" % (driver.label_map[s] * 1000 + g) for s, g in zip(labels["seg_label"].tolist(), labels["group_label"].tolist()))
        assert tree[os.path.join("gt_vertices", scan + ".txt")] == want.encode()
    result = driver.vertex_result
    figures = {k: v for k, v in result.items() if k != "iou"}
    assert same_result(figures, evaluate_files(pred_dir, gt_dir, t.scans, label_map=driver.label_map))
    assert 0.0 <= result["iou"] <= 1.0
    # the added vertices take part: some mask has a set byte past the scene's points
    n = 4096
    assert any(b"1" in tree[k].split(b"\n", n)[n] for k in masks)
    ap = result["ap"]
    print("per vertex: AP %.4f AP50 %.4f AP25 %.4f, mean IoU %.4f; per point: AP %.4f, mean IoU %.4f; %d masks of %d lines"
          % (result["all_ap"], result["all_ap_50%"], result["all_ap_25%"], result["iou"], driver.result["all_ap"], driver.result["iou"], len(masks), V))
    assert not np.isnan(ap).all()


def test_run_and_the_variables_are_left_as_they_were(driver, tmp_path):
    t = driver.tester
    assert same_store(t.store, driver.store)                                       # bit-identical across run_vertices
    again = t.run(out_dir=str(tmp_path / "second"))
    a, w = read_tree(str(tmp_path / "second")), read_tree(driver.first)
    assert sorted(a) == sorted(w) and all(a[k] == w[k] for k in w) and same_result(again, driver.result)
    assert same_store(t.store, driver.store)
    pred, batch = t.predict([2])                                                    # predict's return value keeps its keys
    assert set(pred) == {"order", "count", "label_ids", "confidence", "sem_conf", "fb_conf", "score", "masks", "mask_points"}
    assert "lift" not in batch and pred["masks"].shape[0] == 1


def test_the_scene_s_own_points_as_the_scan_give_run_s_files(driver, tmp_path):
    t = driver.tester
    cache = driver.cache
    assert all(len(np.unique(cache["pc"][k].numpy(), axis=0)) == 4096 for k in range(SCENES))           # pairwise distinct: src is the identity
    own = lambda k: {"xyz": cache["pc"][k], "seg_label": cache["seg_label"][k], "group_label": cache["group_label"][k]}        # noqa: E731
    result = t.run_vertices(str(tmp_path / "own"), own)
    a, w = read_tree(str(tmp_path / "own")), read_tree(driver.first)
    rename = lambda k: k.replace("pred_vertices", "pred", 1).replace("gt_vertices", "gt", 1)            # noqa: E731
    assert sorted(rename(k) for k in a) == sorted(w) and all(a[k] == w[rename(k)] for k in a)
    assert same_result(result, driver.result)                                       # AP and the mean IoU of sem_class_logits[src]
    # files only, and the rule on labels
    assert t.run_vertices(str(tmp_path / "files_only"), lambda k: {"xyz": cache["pc"][k]}, evaluate=False) is None
    files = read_tree(str(tmp_path / "files_only"))
    assert sorted(files) == sorted(k for k in a if k.startswith("pred_vertices") and not k.endswith("evaluation.txt"))
    assert all(files[k] == a[k] for k in files)
    with pytest.raises(ValueError, match="has no 'seg_label' and 'group_label'"):
        t.run_vertices(None, lambda k: {"xyz": cache["pc"][k]})
    with pytest.raises(ValueError, match="must label each of its 4096 vertices"):
        t.run_vertices(None, lambda k: dict(own(k), seg_label=cache["seg_label"][k][:100]))


def test_the_tool_prints_the_per_vertex_figures(driver, tmp_path, capsys):
    from gspn_amd.train import save_variables
    a = driver.args
    assert (a.synthetic_vertices, a.mesh_path, a.label_path, a.batch_size) == (V, None, None, BATCH)
    path = save_variables(str(tmp_path / "model.ckpt"), driver.tester.store)
    out = str(tmp_path / "eva")
    result = driver.tool.main(ARGV + ["--no_files", "--model_path", path, "--out", out])
    printed = capsys.readouterr().out
    assert "AP: " in printed and "mean IoU: " in printed and not os.path.exists(out)                   # --no_files: the figures only
    assert set(driver.vertex_result) == set(result) and 0.0 <= result["iou"] <= 1.0
