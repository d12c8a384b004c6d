"""GPU tests of the test driver: gspn_sample_points_in_boxes_seeds (csrc/roi.hip) bit for bit against the one-seed entry run on each scene
alone and against the restated generator of tests/roi_ref.py, the crops of rpointnet_inference independent of a scene's slot once it has a
seed of its own, and gspn_amd/tester.py -- predict against the parts chained by hand, captured and eager, run's files against the exporters
of tests/predict_ref.py and its figures against evaluate_files, an InstanceAP fed by hand and the IoU loop, and restore.

Every comparison is exact: both sides run the same kernels on the same inputs, or compare integers and bytes.  The driver runs at the sizes
of tests/test_gpu_inference.py (small_config) on a synthetic cache of 5 scenes with the sizes of tests/test_gpu_train.py's datasets(), two
scenes per step, so the last batch is short."""
import functools
import os

import numpy as np
import pytest
import torch

from gspn_amd import synth, tf_util
from tests import predict_ref as PR
from tests import roi_ref as RR
from tests import test_gpu_heads as TH
from tests import test_gpu_inference as TI
from tests import test_gpu_spn_net as TS
from tests import test_gpu_train as TT
from tests.test_gpu_modules import fresh_store

pytestmark = pytest.mark.gpu

ROOM = torch.tensor(RR.ROOM)
GOLD = 0x9E3779B97F4A7C15


def dev_seeds(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device="cuda")


def as_int64(v):
    """v modulo 2^64 as the signed word the kernels read"""
    v %= 1 << 64
    return v - (1 << 64) if v >= (1 << 63) else v


# ---- 1. the sampler's per-scene seeds -------------------------------------------------------------------------------------------------

NSMP, MARGIN = 64, 1e-3
SEEDS = (42, -7, (1 << 40) + 3)


def sampler_case(b, r, n, seed):
    """a random cloud per scene and, over the r boxes of the b scenes in turn: a box over most of the room, a box holding no point, a box
    of a few points (fewer than NSMP), an all-zero row, a random box"""
    g = torch.Generator().manual_seed(seed)
    pc = torch.rand(b, n, 3, generator=g) * ROOM
    box = torch.zeros(b, r, 6)
    for i in range(b):
        for k in range(r):
            kind = (i * r + k) % 5
            if kind == 0:
                box[i, k] = torch.cat((ROOM / 2, ROOM * 0.8))
            elif kind == 1:
                box[i, k] = torch.tensor([100.0, 100.0, 100.0, 1.0, 1.0, 1.0])
            elif kind == 2:
                near = pc[i, (pc[i] - pc[i, 7]).square().sum(-1).argsort()[:4]]                  # point 7 and its three nearest
                box[i, k] = torch.cat(((near.max(0).values + near.min(0).values) / 2, near.max(0).values - near.min(0).values + 0.01))
            elif kind == 4:
                box[i, k] = torch.cat((torch.rand(3, generator=g) * ROOM, torch.rand(3, generator=g) * 1.5 + 0.5))
    return box.contiguous(), pc.contiguous()


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("r", [1, 5])
def test_sampler_per_scene_seeds_bit_for_bit(r, n):
    from gspn_amd.graph import CapturedStep
    from gspn_amd.rpointnet import sample_points_in_boxes
    b = 3
    box, pc = sampler_case(b, r, n, 100 * r + n)
    cnt = RR.box_point_count(box, pc, MARGIN).reshape(-1)
    kinds = torch.arange(b * r) % 5
    assert bool((cnt[kinds == 0] >= NSMP).all()) and not cnt[kinds == 1].any() and not cnt[kinds == 3].any()      # full, no point, all-zero
    assert bool(((cnt[kinds == 2] >= 4) & (cnt[kinds == 2] < NSMP)).all()) and int((kinds == 2).sum()) >= 1        # fewer points than draws
    bx, p = box.cuda(), pc.cuda()
    seeds = dev_seeds(SEEDS)
    got = sample_points_in_boxes(bx, p, NSMP, 0, MARGIN, scene_seeds=seeds)
    assert got.dtype == torch.int32 and tuple(got.shape) == (b, r, NSMP)
    assert torch.equal(sample_points_in_boxes(bx, p, NSMP, 12345, MARGIN, scene_seeds=seeds), got)                # seed is ignored
    for s in range(b):
        alone = sample_points_in_boxes(bx[s:s + 1], p[s:s + 1], NSMP, dev_seeds(SEEDS[s:s + 1]), MARGIN)
        assert torch.equal(got[s:s + 1], alone), s                                                               # the scene alone with its seed
        assert torch.equal(got[s].cpu(), RR.sample_points_in_boxes(box[s:s + 1], pc[s:s + 1], NSMP, SEEDS[s], MARGIN)[0]), s
    zero = (cnt == 0).reshape(b, r)
    assert not got.cpu()[zero].any()
    # two scenes with the same points and boxes and different seeds
    same = sample_points_in_boxes(bx[:1].expand(b, r, 6).contiguous(), p[:1].expand(b, n, 3).contiguous(), NSMP, 0, MARGIN, scene_seeds=seeds)
    assert torch.equal(same[0], got[0])
    assert not torch.equal(same[0, 0], same[1, 0]) and not torch.equal(same[1, 0], same[2, 0]) and not torch.equal(same[0, 0], same[2, 0])
    # the one-seed entry is what it was: slot s of a batch draws from the stream (seed, s), which is the stream (seed + s * GOLD, 0) of
    # a scene alone (include/gspn_hip.h: the state is mix(seed + GOLD * (scene + 1)))
    shared = 42
    old = sample_points_in_boxes(bx, p, NSMP, dev_seeds([shared]), MARGIN)
    assert torch.equal(old.cpu(), RR.sample_points_in_boxes(box, pc, NSMP, shared, MARGIN))
    for s in range(b):
        alone = sample_points_in_boxes(bx[s:s + 1], p[s:s + 1], NSMP, dev_seeds([as_int64(shared + s * GOLD)]), MARGIN)
        assert torch.equal(old[s:s + 1], alone), s
    assert torch.equal(old[0], got[0]) and not torch.equal(old[2], got[2])                                        # SEEDS[0] is the shared seed
    assert torch.equal(sample_points_in_boxes(bx, p, NSMP, 0, MARGIN, scene_seeds=dev_seeds([as_int64(shared + s * GOLD) for s in range(b)])), old)
    # a captured call reads the seeds on the device
    st = {}

    def step():
        st["out"] = sample_points_in_boxes(bx, p, NSMP, 0, MARGIN, scene_seeds=seeds)

    cap = CapturedStep(step)
    cap.replay()
    torch.cuda.synchronize()
    assert torch.equal(st["out"], got)
    moved = (SEEDS[2], SEEDS[0] + 1, SEEDS[1])
    seeds.copy_(dev_seeds(moved))
    cap.replay()
    torch.cuda.synchronize()
    replayed = st["out"].clone()
    assert torch.equal(replayed, sample_points_in_boxes(bx, p, NSMP, 0, MARGIN, scene_seeds=dev_seeds(moved)))
    assert not torch.equal(replayed, got)


def test_sampler_per_scene_seeds_rejects_what_the_one_seed_entry_rejects():
    from gspn_amd.rpointnet import sample_points_in_boxes
    box = torch.ones(2, 3, 6, device="cuda")
    with pytest.raises(NotImplementedError):
        sample_points_in_boxes(box, torch.zeros(2, 32769, 3, device="cuda"), 4, 0, scene_seeds=dev_seeds([1, 2]))
    with pytest.raises(ValueError):
        sample_points_in_boxes(box, torch.zeros(2, 8, 3, device="cuda"), 4, 0, scene_seeds=dev_seeds([1, 2, 3]))
    with pytest.raises(ValueError):
        sample_points_in_boxes(box, torch.zeros(2, 8, 3, device="cuda"), 4, 0, scene_seeds=dev_seeds([1, 2]).int())
    with pytest.raises(ValueError):
        sample_points_in_boxes(box, torch.zeros(2, 8, 3, device="cuda"), 4, 0, scene_seeds=dev_seeds([1, 0, 2])[::2])      # not contiguous


# ---- 2. slot independence --------------------------------------------------------------------------------------------------------------

def several_points(idx):
    """idx (R, P) -> (R,) bool: the rows that name more than one point"""
    return (idx != idx[:, :1]).any(-1)


def test_crops_do_not_depend_on_the_slot_with_scene_seeds():
    """a batch [A, B] and the batch [B, A]: with a seed per scene a scene's crop indices are equal wherever its ROIs are equal bit for
    bit; with one seed for the batch they are not, which is what the driver could not live with"""
    from gspn_amd.rpointnet import rpointnet_inference
    sc, cfg = TS.scene(), TI.small_config()
    flipped = {k: v.flip(0).contiguous() for k, v in sc.items()}
    fresh_store(TI.STORE_SEED)
    seeds = dev_seeds([11, 22])
    ab = rpointnet_inference(*TI.scene_args(sc), cfg, scene_seeds=seeds)
    ba = rpointnet_inference(*TI.scene_args(flipped), cfg, scene_seeds=seeds.flip(0).contiguous())
    one = dev_seeds([TI.SEED])
    ab_one = rpointnet_inference(*TI.scene_args(sc), cfg, seed=one)
    ba_one = rpointnet_inference(*TI.scene_args(flipped), cfg, seed=one)
    for rois, idx in (("rois", "mask_selection_idx"), ("rois_final", "mask_selection_idx_final")):
        for scene in (0, 1):
            same = (ab[rois][scene] == ba[rois][1 - scene]).all(-1) & (ab[rois][scene].abs().sum(-1) != 0)
            print("%s, scene %d: %d of %d ROIs equal bit for bit in both slots" % (rois, scene, int(same.sum()), same.numel()))
            assert bool(same.any()), (rois, scene)
            assert torch.equal(ab[idx][scene][same], ba[idx][1 - scene][same]), (idx, scene)
            several = several_points(ab[idx][scene]) & same
            assert bool(several.any()), (rois, scene)
            if rois == "rois_final":
                # with one seed the first crops differ with the slot, the heads then see other points and the detections differ: no
                # ROI is left to compare row by row
                assert not torch.equal(ab_one[idx][scene], ba_one[idx][1 - scene]), (idx, scene)
                continue
            same_one = (ab_one[rois][scene] == ba_one[rois][1 - scene]).all(-1) & (ab_one[rois][scene].abs().sum(-1) != 0)
            several_one = several_points(ab_one[idx][scene]) & same_one
            assert bool(several_one.any()), (rois, scene)
            assert not torch.equal(ab_one[idx][scene][several_one], ba_one[idx][1 - scene][several_one]), (idx, scene)
    # in its own slot, scene 0 of the batch [A, B] with one seed is scene A with that seed
    again = rpointnet_inference(*TI.scene_args(sc), cfg, scene_seeds=dev_seeds([TI.SEED, as_int64(TI.SEED + GOLD)]))
    assert torch.equal(again["mask_selection_idx"], ab_one["mask_selection_idx"])


# ---- the driver --------------------------------------------------------------------------------------------------------------------------

N, NGROUP, NINS, NCAT = TT.N, TT.NGROUP, TT.NINS, TT.NCAT                            # 4096, 12, 512, 9
SCENES, BATCH = 5, 2
BATCHES = ([0, 1], [2, 3], [4])
STORE_SEED = TI.STORE_SEED
SCANS = ["scene%04d_00" % (7 * k) for k in range(SCENES)]


def label_map():
    from gspn_amd.predict import SCANNET_LABEL_MAP
    return SCANNET_LABEL_MAP[:NCAT]


@functools.lru_cache(maxsize=None)
def cache():
    """5 scenes as tests/test_gpu_train.py's datasets() makes them, two with 10 of the 12 groups; no permutation, no augmentation"""
    from gspn_amd.train import DeviceDataset
    d = {k: torch.from_numpy(v) for k, v in synth.spn_batch("S", SCENES, N, NGROUP, NINS, NCAT, 70).items()}
    counts = [12, 10, 12, 10, 12]
    for k, c in enumerate(counts):
        lab = d["group_label"][k]
        d["group_label"][k] = torch.where(lab >= c, lab - c, lab)
        d["pc_ins"][k, c:] = 0.0
    return DeviceDataset(d["pc"].cuda(), d["color"].cuda(), d["group_label"].cuda(), d["seg_label"].cuda(), d["pc_ins"].cuda(),
                         torch.tensor(counts, dtype=torch.int32).cuda(), is_augment=False, permute_points=False)


def make_tester(seed=STORE_SEED, captured=True):
    from gspn_amd.tester import Tester
    return Tester(TI.small_config(), cache(), scans=SCANS, batch_size=BATCH, seed=seed, captured=captured, label_map=label_map())


def plant_boxes(store):
    """Freshly initialised, the decoder draws every instance within centimetres of its seed: the proposals hold a handful of points and no
    mask reaches the 100 points the benchmark asks of a prediction.  A bias of up to a metre either way on the decoder's fully connected
    points gives every proposal a box of about two metres in this 8 x 6 x 3 m room."""
    bias = store.vars["shape_proposal_net/decoder/de_fc4/biases"]
    with torch.no_grad():
        bias.copy_((torch.rand(bias.shape, generator=torch.Generator().manual_seed(9)) * 2.0 - 1.0).to(bias.device))


def by_hand(store, idx, seed):
    """rpointnet_inference + scene_predictions on data.batch's output for the slots of the batch idx, a short one filled by repeating its
    last scene -> (pred, batch, end_points), uncut"""
    from gspn_amd.predict import scene_predictions
    from gspn_amd.rpointnet import rpointnet_inference
    slots = list(idx) + [idx[-1]] * (BATCH - len(idx))
    cfg = TI.small_config(NUM_POINT_INS=NINS, BATCH_SIZE=BATCH)
    tf_util.set_variable_store(store)
    batch = cache().batch(slots)
    ep = rpointnet_inference(*TI.scene_args(batch), cfg, scene_seeds=dev_seeds([seed + 2 * k for k in slots]))
    return scene_predictions(ep, batch["pc"], label_map=label_map()), batch, ep


def snapshot(store):
    return {n: v.detach().clone() for n, v in store.vars.items()}


def same_store(store, snap):
    return list(store.vars) == list(snap) and all(torch.equal(v, snap[n]) for n, v in store.vars.items())


class Drivers:
    def __init__(self):
        self.captured, self.eager = make_tester(captured=True), make_tester(captured=False)
        plant_boxes(self.captured.store)
        plant_boxes(self.eager.store)
        self.hand = [by_hand(self.captured.store, idx, STORE_SEED) for idx in BATCHES]          # computed once, shared, left unchanged


@pytest.fixture(scope="module")
def drivers():
    return Drivers()


def test_tester_sets_the_config_and_creates_the_reference_s_variables(drivers):
    t = drivers.captured
    assert (t.cfg.NUM_GROUP, t.cfg.NUM_POINT, t.cfg.NUM_POINT_INS, t.cfg.BATCH_SIZE) == (NGROUP, N, NINS, BATCH)
    fpn = sum([TH.layer_names("fpn%d" % i) for i in (1, 2, 3, 4)], [])              # rpointnet_inference's, in the reference's order
    assert list(t.store.vars) == TS.expected_variable_names() + fpn + TH.cls_names(*TI.CLS_LISTS) + TH.seg_names(*TI.SEG_LISTS)
    assert same_store(drivers.eager.store, snapshot(t.store))                       # one seed, one set of initial values
    assert t.scans == SCANS and drivers.eager.store is not t.store


@pytest.mark.parametrize("at", [0, 2])
def test_predict_equals_the_parts_chained_by_hand(drivers, at):
    idx = BATCHES[at]
    want, want_batch, _ = drivers.hand[at]
    k = len(idx)
    got = {}
    for name, t in (("captured", drivers.captured), ("eager", drivers.eager)):
        pred, batch = t.predict(idx)
        assert set(pred) == set(want) == {"order", "count", "label_ids", "confidence", "sem_conf", "fb_conf", "score", "masks", "mask_points"}
        for key, w in want.items():
            assert pred[key].shape[0] == k and torch.equal(pred[key], w[:k]), (name, key)
        for key, w in want_batch.items():
            assert torch.equal(batch[key], w[:k]), (name, key)
        assert batch["iou_inter"].shape == (k, NCAT - 1) and batch["ap_counts"]["n_true"].shape[0] == k
        got[name] = (pred, batch)
    for key in want:
        assert torch.equal(got["captured"][0][key], got["eager"][0][key]), key
    for key in got["captured"][1]["ap_counts"]:
        assert torch.equal(got["captured"][1]["ap_counts"][key], got["eager"][1]["ap_counts"][key]), key
    # what is returned are clones: another batch through the same graph leaves them alone
    kept = {key: v.clone() for key, v in got["captured"][0].items()}
    drivers.captured.predict(BATCHES[1])
    assert all(torch.equal(got["captured"][0][key], kept[key]) for key in kept)
    count, points = want["count"][:k].cpu(), want["mask_points"][:k].cpu()
    print("batch %s: %s predictions, the largest masks %s points" % (idx, count.tolist(), points.max(1).values.tolist()))
    assert any(int(count[s]) > 0 and bool((points[s, :int(count[s])] > 0).any()) for s in range(k))          # not vacuous


def read_tree(root):
    out = {}
    for base, _, files in os.walk(root):
        for name in files:
            with open(os.path.join(base, name), "rb") as f:
                out[os.path.relpath(os.path.join(base, name), root)] = f.read()
    return out


def same_result(a, b):
    """two dicts of InstanceAP.compute(): arrays equal with nan == nan, floats likewise"""
    def same(x, y):
        if isinstance(x, dict):
            return set(x) == set(y) and all(same(x[k], y[k]) for k in x)
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        if isinstance(x, (float, np.ndarray)):
            return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)
        return x == y
    return same(a, b)


def test_run_over_the_five_scenes(drivers, tmp_path, monkeypatch):
    from gspn_amd import tester as T
    from gspn_amd.evaluate import InstanceAP, evaluate_files
    from gspn_amd.predict import mean_iou
    t = drivers.captured
    before = snapshot(t.store)
    written = []
    real_pred, real_gt = T.write_predictions, T.write_ground_truth
    monkeypatch.setattr(T, "write_predictions", lambda out_dir, scan, *a, **kw: (written.append(("pred", scan)), real_pred(out_dir, scan, *a, **kw))[1])
    monkeypatch.setattr(T, "write_ground_truth", lambda out_dir, scan, *a, **kw: (written.append(("gt", scan)), real_gt(out_dir, scan, *a, **kw))[1])
    ours = str(tmp_path / "ours")
    result = t.run(out_dir=ours)
    assert same_store(t.store, before)                                              # the moving statistics and every other variable
    assert sorted(written) == sorted([("gt", s) for s in SCANS] + [("pred", s) for s in SCANS])          # every scene once, the filled slot never

    # the files, against the reference's exporters fed with the tensors of the hand chain
    theirs = str(tmp_path / "theirs")
    os.makedirs(os.path.join(theirs, "pred"))
    metric = InstanceAP(NCAT, label_map=label_map())
    inter = union = None
    for idx, (pred, batch, ep) in zip(BATCHES, drivers.hand):
        k = len(idx)
        metric.add_predictions({key: v[:k] for key, v in pred.items()}, batch["seg_label"][:k], batch["group_label"][:k], NGROUP)
        for s, scene in enumerate(idx):
            nd = int(pred["count"][s])
            PR.export_instance_ids_for_eval_customized(os.path.join(theirs, "pred", SCANS[scene] + ".txt"), pred["label_ids"][s, :nd].cpu().numpy(),
                                                       pred["masks"][s, :nd].cpu().numpy(), pred["confidence"][s, :nd].cpu().numpy())
            PR.gen_gt(os.path.join(theirs, "gt"), SCANS[scene], batch["seg_label"][s].cpu().numpy(), batch["group_label"][s].cpu().numpy(),
                      PR.SEG_LABEL_MAP[:NCAT])
            inter, union = PR.iou_counts(ep["sem_class_logits"][s].cpu().numpy(), batch["seg_label"][s].cpu().numpy(), NCAT, inter, union)
    a, w = read_tree(ours), read_tree(theirs)
    result_file = os.path.join("pred", T.RESULT_FILE)
    assert sorted(a) == sorted(list(w) + [result_file]) and all(a[k] == w[k] for k in w)
    masks = [k for k in w if k.startswith(os.path.join("pred", "pred_mask"))]
    assert len(w) == 2 * SCENES + len(masks) and len(masks) > 0
    assert a[result_file].startswith(b"class,class id,ap,ap50,ap25\n") and a[result_file].count(b"\n") == NCAT

    # the figures
    figures = {k: v for k, v in result.items() if k != "iou"}
    assert same_result(figures, evaluate_files(os.path.join(ours, "pred"), os.path.join(ours, "gt"), SCANS, label_map=label_map()))
    assert same_result(figures, metric.compute())
    assert result["iou"] == float(mean_iou(torch.from_numpy(inter).cuda(), torch.from_numpy(union).cuda())) and int(union.sum()) > 0
    assert PR.within_bound(np.float64(result["iou"]), PR.mean_iou(inter, union), NCAT - 1)
    ap = result["ap"]
    both = ~np.isnan(ap).all(1) & np.array([any(int((b["n_pred"][:, s] > 0).sum()) for b in metric._records()) for s in range(1, NCAT)])
    print("classes with ground truth and predictions: %s; AP %.4f AP50 %.4f AP25 %.4f, mean IoU %.4f"
          % ((np.nonzero(both)[0] + 1).tolist(), result["all_ap"], result["all_ap_50%"], result["all_ap_25%"], result["iou"]))
    assert bool(both.any())                                                         # not vacuous
    # eager, without files and then without figures
    assert same_result(drivers.eager.run(), result)
    assert drivers.eager.run(out_dir=str(tmp_path / "files_only"), evaluate=False) is None
    files_only = read_tree(str(tmp_path / "files_only"))
    assert sorted(files_only) == sorted(w) and all(files_only[k] == w[k] for k in w)


def test_restore(drivers, tmp_path):
    from gspn_amd.train import save_variables
    # a store built under one seed, into a Tester built under another (its crops keep that Tester's seeds)
    other = STORE_SEED + 1
    path = save_variables(str(tmp_path / "heads.ckpt"), drivers.captured.store, optimizer={"t": 3}, step=7)
    t = make_tester(seed=other)
    assert not torch.equal(t.store.vars["fpn1/weights"], drivers.captured.store.vars["fpn1/weights"])
    first, _ = t.predict(BATCHES[0])                                                # captured here, replayed after the restore
    ckpt = t.restore(path)
    assert ckpt["step"] == 7 and same_store(t.store, snapshot(drivers.captured.store))
    want, _, _ = by_hand(drivers.captured.store, BATCHES[0], other)
    got, _ = t.predict(BATCHES[0])
    for key, w in want.items():
        assert torch.equal(got[key], w), key
    assert not torch.equal(got["score"], first["score"])

    # a file of Trainer.save after two captured SPN steps: the proposal net alone
    tr = TT.trainer('SPN', True)
    tr.train_one_epoch()
    assert tr.step == 2
    spn = tr.save(str(tmp_path / "spn.ckpt"))
    tr.close()
    before = snapshot(t.store)
    with pytest.raises(KeyError) as e:
        t.restore(spn)
    name = str(e.value).split("variable ")[1].split(" is not in the checkpoint")[0]
    assert name in t.store.vars and not name.startswith("shape_proposal_net/"), name          # a variable behind the proposal net
    assert same_store(t.store, before)                                              # nothing was written
    t.restore(spn, scope='shape_proposal_net')
    scoped = [n for n in t.store.vars if n.startswith("shape_proposal_net/")]
    assert 0 < len(scoped) < len(t.store.vars)
    assert all(torch.equal(t.store.vars[n], tr.store.vars[n].detach()) for n in scoped)
    assert any(not torch.equal(t.store.vars[n], before[n]) for n in scoped)
    assert all(torch.equal(v, before[n]) for n, v in t.store.vars.items() if n not in set(scoped))          # the heads are untouched
    pred, _ = t.predict(BATCHES[2])                                                 # and the driver still runs
    assert pred["count"].shape == (1,)
