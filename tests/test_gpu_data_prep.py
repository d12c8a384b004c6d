"""GPU tests of gspn_amd/data_prep.py on csrc/data_prep.hip: segment_labels equal to the restated loop of the reference's collect_label, labels
and Error! count, on constructed and seeded cases; downsample_scans equal to the CPU oracle's picks per scan, batched or not, on both sampling
paths; prepare_scans end to end on a directory in ScanNet's layout written by the test's own binary writer; build_cache equal to the
composition of tests/dataset_ref.py under the documented chunk-seed rule, and its file through tools/train.py's loader."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import data_prep_ref as PR
from tests import dataset_ref as DR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. segment_labels -------------------------------------------------------------------------------------------------------------------

def run_labels(seg, groups, num_segments=None, offset=0):
    """segment_labels on the device against the loop; offset: seg_indices starts that many entries behind a 16-byte boundary"""
    from gspn_amd import data_prep
    seg = np.asarray(seg, dtype=np.int64)
    want, errors = PR.collect_label_loop(seg, groups)
    segments, objects = PR.pairs_of(groups)
    dev_seg = torch.cat((torch.zeros(offset, dtype=torch.int32), torch.from_numpy(seg.astype(np.int32)))).cuda()[offset:]
    assert dev_seg.data_ptr() % 16 == (4 * offset) % 16
    label, conflicts = data_prep.segment_labels(dev_seg, torch.tensor(segments, dtype=torch.int32).cuda(),
                                                torch.tensor(objects, dtype=torch.int64).cuda(), num_segments)
    assert label.dtype == torch.int32 and conflicts.dtype == torch.int32 and tuple(label.shape) == (len(seg),) and tuple(conflicts.shape) == (1,)
    assert np.array_equal(label.cpu().numpy(), want)
    assert int(conflicts.item()) == errors
    return want, errors


def test_segment_labels_constructed_cases():
    seg = [4, 4, 1, 9, 1, 6, 6, 2, 0, 9, 4]
    # a segment named by two groups: the later wins, one conflict
    want, errors = run_labels(seg, [{"objectId": 5, "segments": [4, 1]}, {"objectId": 2, "segments": [4]}])
    assert errors == 1 and want.tolist() == [2, 2, 5, -1, 5, -1, -1, -1, -1, -1, 2]
    # ... also when the later objectId is the smaller or equal one, and across three groups
    assert run_labels(seg, [{"objectId": 0, "segments": [6]}, {"objectId": 0, "segments": [6]}, {"objectId": 7, "segments": [6, 2]}])[1] == 2
    # the same segment twice inside one group
    want, errors = run_labels(seg, [{"objectId": 3, "segments": [9, 9, 0]}])
    assert errors == 1 and want.tolist() == [-1, -1, -1, 3, -1, -1, -1, -1, 3, 3, -1]
    # a pair whose segment has no vertex: no conflict, named once or twice, below or beyond the largest id, negative
    assert run_labels(seg, [{"objectId": 1, "segments": [3, 3, 5]}, {"objectId": 2, "segments": [3, 10, 77, 1000000, -4, 2]}])[1] == 0
    # vertices in no group, and a group without a segment
    want, errors = run_labels(seg, [{"objectId": 6, "segments": []}, {"objectId": 1, "segments": [2]}])
    assert errors == 0 and (want == -1).sum() == 10
    # p == 0
    want, errors = run_labels(seg, [])
    assert errors == 0 and (want == -1).all()
    run_labels(seg, [{"objectId": 1, "segments": []}])
    # num_segments given by the caller, as collect_label does; a smaller one leaves the vertices beyond it unlabelled
    run_labels(seg, [{"objectId": 5, "segments": [4, 1, 9]}, {"objectId": 2, "segments": [4]}], num_segments=10)
    from gspn_amd import data_prep
    label, conflicts = data_prep.segment_labels(torch.tensor(seg, dtype=torch.int64).cuda(), torch.tensor([4, 9, 9]).cuda(),
                                                torch.tensor([5, 1, 2]).cuda(), num_segments=9)
    assert label.tolist() == [5, 5, -1, -1, -1, -1, -1, -1, -1, -1, 5] and conflicts.item() == 0
    # negative entries of seg_indices get -1
    label, conflicts = data_prep.segment_labels(torch.tensor([-1, 3, -7, 3], dtype=torch.int32).cuda(), torch.tensor([3, 3], dtype=torch.int32).cuda(),
                                                torch.tensor([8, 9], dtype=torch.int32).cuda())
    assert label.tolist() == [-1, 9, -1, 9] and conflicts.item() == 1


def test_segment_labels_sparse_ids():
    rng = np.random.default_rng(5)
    ids = rng.choice(1000001, 60, replace=False)
    ids[0] = 1000000
    seg = ids[rng.integers(0, 60, 500)]
    seg[0] = 1000000
    groups = [{"objectId": int(g), "segments": [int(v) for v in ids[g * 5:g * 5 + 6]]} for g in range(11)]      # each shares one segment with the next
    want, errors = run_labels(seg, groups)
    assert errors >= 5 and (want >= 0).any() and (want == -1).any()


def random_case(n, seed, twice):
    rng = np.random.default_rng(seed)
    nseg = max(2, n // 9)
    seg = rng.integers(0, nseg, n)
    ngroup = max(1, nseg // 5)
    owner = rng.integers(0, ngroup + 2, nseg)                                     # >= ngroup: in no group
    groups = [{"objectId": int(rng.integers(0, 50)), "segments": [int(s) for s in np.nonzero(owner == g)[0]]} for g in range(ngroup)]
    named = np.nonzero(owner < ngroup)[0]
    for s in rng.choice(named, int(twice * len(named)), replace=False):
        groups[int(rng.integers(0, ngroup))]["segments"].append(int(s))
    for g in groups:
        rng.shuffle(g["segments"])
    return seg, groups


@pytest.mark.parametrize("n", [1, 63, 64, 257, 4099, 70001])
def test_segment_labels_seeded_cases(n):
    seen = 0
    for at, twice in enumerate((0.0, 0.1, 0.3)):
        seg, groups = random_case(n, 100 * n + at, twice)
        want, errors = run_labels(seg, groups, offset=at)                          # offsets 0, 1, 2: the vector path with and without a head
        seen += errors
        assert twice == 0.0 or n < 257 or errors > 0
    run_labels(seg, groups, offset=3)
    assert n < 257 or seen > 0


def test_segment_labels_refuses_a_negative_object_id():
    from gspn_amd import data_prep
    seg, ps = torch.zeros(8, dtype=torch.int32).cuda(), torch.tensor([0, 0], dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match="negative"):
        data_prep.segment_labels(seg, ps, torch.tensor([3, -1], dtype=torch.int32).cuda())
    with pytest.raises(ValueError):
        data_prep.segment_labels(seg, ps, torch.tensor([3, 1 << 31], dtype=torch.int64).cuda())


# ---- 2. downsample_scans -----------------------------------------------------------------------------------------------------------------

def scan_of(n, seed):
    """a duplicate-heavy scan with attributes of every kind: xyz float32, colour uint8, sem int32, ins int64"""
    from gspn_amd import synth
    rng = np.random.default_rng(seed)
    xyz = synth.cloud_d(n, seed, frac=0.3)
    return xyz, rng.integers(0, 256, (n, 3)).astype(np.uint8), rng.integers(0, 40, n).astype(np.int32), rng.integers(-1, 30, n).astype(np.int64)


@functools.lru_cache(maxsize=None)
def scans_and_picks(sizes, nsample):
    """the scans and, for those above nsample, the oracle's picks -- shared, never written"""
    scans = [scan_of(n, 7 + n) for n in sizes]
    picks = [O.farthest_point_sample(nsample, s[0][None])[0].astype(np.int64) if s[0].shape[0] > nsample else None for s in scans]
    for arrays in scans:
        for a in arrays:
            a.setflags(write=False)
    return scans, picks


@pytest.mark.parametrize("sizes,nsample,batch", [((36500, 900, 40000, 33000), 1500, 3), ((3000, 2500), 2000, 2)], ids=["multi_cu", "single_cu"])
def test_downsample_scans_equals_the_oracle_batched_or_not(sizes, nsample, batch):
    from gspn_amd import data_prep
    scans, picks = scans_and_picks(sizes, nsample)
    dev_scans = [tuple(torch.from_numpy(a.copy()).cuda() for a in s) for s in scans]
    single = data_prep.downsample_scans(dev_scans, nsample)                         # batch = 1
    batched = data_prep.downsample_scans(dev_scans, nsample, batch=batch)
    assert len(single) == len(batched) == len(scans)
    for at, (scan, pick) in enumerate(zip(scans, picks)):                           # in the caller's order
        for k in range(4):
            want = scan[k] if pick is None else scan[k][pick]
            for got in (single[at][k], batched[at][k]):
                assert got.dtype == dev_scans[at][k].dtype and tuple(got.shape) == want.shape
                assert np.array_equal(got.cpu().numpy().view(np.int32) if k == 0 else got.cpu().numpy(), want.view(np.int32) if k == 0 else want)
            assert torch.equal(single[at][k], batched[at][k])
        if pick is None:
            assert all(single[at][k] is dev_scans[at][k] for k in range(4))         # returned as it is
        else:
            assert pick.max() < scan[0].shape[0]


# ---- 3. / 4. prepare_scans and build_cache on a directory in ScanNet's layout ------------------------------------------------------------------

NSAMPLE, NPOINT, NPOINT_INS, SEED = 2000, 1024, 64, 11
SCANS = (("scene0002_00", 2300, 9, 0), ("scene0000_00", 2600, 12, 2), ("scene0001_01", 700, 5, 0))       # name, points, groups, segments named twice
SEM_OF_GROUP = (3, 4, 0, 39, 5, 1, 24, 36, 14, 7, 2, 12)                         # 0, 1 and 2 are no valid class: groups that do not count


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    """the three scans written, prepare_scans run once over them with two scans per window -> everything the tests below compare"""
    from gspn_amd import data_prep
    root, out = str(tmp_path_factory.mktemp("scannet")), str(tmp_path_factory.mktemp("prepared"))
    truth = {}
    for at, (name, n, ngroup, twice) in enumerate(SCANS):
        xyz, color, sem, seg_indices, groups = PR.labelled_scan(n, ngroup, 31 + at, SEM_OF_GROUP, twice)
        PR.write_scan(root, name, xyz, color, sem, seg_indices, groups)
        ins, errors = PR.collect_label_loop(seg_indices, groups)
        pick = O.farthest_point_sample(NSAMPLE, xyz[None])[0].astype(np.int64) if n > NSAMPLE else np.arange(n)
        truth[name] = dict(xyz=xyz[pick], color=color[pick], sem=sem[pick], ins=ins[pick], errors=errors, n=n)
    lines = []
    report = data_prep.prepare_scans(root, out, NSAMPLE, batch=2, log=lines.append)
    return dict(root=root, out=out, truth=truth, report=report, lines=lines)


def test_prepare_scans_end_to_end(prepared, capfd):
    from gspn_amd import data_prep, io_util
    out, truth = prepared["out"], prepared["truth"]
    names = sorted(truth)
    assert [r[0] for r in prepared["report"]] == names                              # sorted by name
    assert prepared["lines"] == ["Scene %d done!" % i for i in range(3)]
    assert sorted(os.listdir(os.path.join(out, "mesh/scans"))) == [n + ".ply" for n in names]
    assert sorted(os.listdir(os.path.join(out, "label/scans"))) == sorted(k + n + ".txt" for n in names for k in ("sem_", "group_"))
    for scan, n_in, n_out, conflicts in prepared["report"]:
        t = truth[scan]
        assert (n_in, n_out, conflicts) == (t["n"], min(t["n"], NSAMPLE), t["errors"])
        assert open(os.path.join(out, "label/scans", "sem_" + scan + ".txt"), "rb").read() == PR.label_lines(t["sem"])
        assert open(os.path.join(out, "label/scans", "group_" + scan + ".txt"), "rb").read() == PR.label_lines(t["ins"])
        rows = io_util.read_color_ply(os.path.join(out, "mesh/scans", scan + ".ply"))
        assert rows.dtype == np.float32 and np.array_equal(rows[:, :3].view(np.int32), t["xyz"].view(np.int32))
        assert np.array_equal(rows[:, 3:], t["color"].astype(np.float32))
    assert truth["scene0000_00"]["errors"] >= 2 and truth["scene0002_00"]["errors"] == 0 and (truth["scene0000_00"]["ins"] == -1).any()
    # the conflict is reported where the reference prints Error!: collect_label's count, and a line on stderr per scan that has one
    capfd.readouterr()
    sem, ins, conflicts = data_prep.collect_label(os.path.join(prepared["root"], "label/scans"), "scene0000_00", "cuda")
    assert conflicts == truth["scene0000_00"]["errors"] and sem.dtype == ins.dtype == torch.int32 and sem.is_cuda and ins.is_cuda
    only = data_prep.prepare_scans(prepared["root"], os.path.join(out, "again"), NSAMPLE, scans=["scene0000_00", "scene0001_01"], log=lambda line: None)
    err = capfd.readouterr().err
    assert [r[0] for r in only] == ["scene0000_00", "scene0001_01"]
    assert sorted(os.listdir(os.path.join(out, "again/mesh/scans"))) == ["scene0000_00.ply", "scene0001_01.ply"]
    assert err.count("Error!") == 1 and "scene0000_00" in err and "scene0001_01" not in err


@pytest.fixture(scope="module")
def cache_case(prepared, tmp_path_factory):
    from gspn_amd import data_prep
    order = ["scene0000_00", "scene0001_01", "scene0002_00"]                        # 2000, 700, 2000 points: chunks [0, 2] and [1]
    list_path = str(tmp_path_factory.mktemp("lists") / "train.txt")
    with open(list_path, "w") as f:
        f.write("\n".join(order) + "\n")
    mesh, label = os.path.join(prepared["out"], "mesh/scans"), os.path.join(prepared["out"], "label/scans")
    cache = data_prep.build_cache(mesh, label, list_path, NPOINT, NPOINT_INS, SEED, batch=2)
    return dict(order=order, list_path=list_path, mesh=mesh, label=label, cache=cache)


def test_build_cache_equals_the_restated_composition(prepared, cache_case):
    from gspn_amd import data_prep
    from gspn_amd.train import DeviceDataset
    cache, order, truth = cache_case["cache"], cache_case["order"], prepared["truth"]
    assert data_prep.cache_chunks([2000, 700, 2000], 2) == [[0, 2], [1]]
    want = {k: [None] * 3 for k in ("pc", "color", "group_label", "seg_label", "pc_ins", "ngroup")}
    for chunk in ([0, 2], [1]):
        seed = SEED + chunk[0]                                                      # the documented rule
        remapped = [DR.remap_labels(truth[order[i]]["ins"], truth[order[i]]["sem"]) for i in chunk]
        pcs = np.stack([truth[order[i]]["xyz"] for i in chunk])
        width = max(r[2] for r in remapped)
        sets = DR.instance_sets(pcs, np.stack([r[0] for r in remapped]), width, NPOINT_INS, seed)[1]
        for row, i in enumerate(chunk):
            choice = DR.resample_choice(pcs[row], NPOINT, seed, row)
            want["pc"][i] = pcs[row][choice]
            want["color"][i] = (truth[order[i]]["color"].astype(np.float32) / 255.0)[choice]
            want["group_label"][i], want["seg_label"][i], want["ngroup"][i] = remapped[row][0][choice], remapped[row][1][choice], remapped[row][2]
            want["pc_ins"][i] = sets[row]
    widest = max(want["ngroup"])
    assert len(set(want["ngroup"])) > 1 and min(want["ngroup"]) >= 3                # pc_ins is padded for some scene; the invalid groups do not count
    assert sorted(cache) == sorted(data_prep.CACHE_KEYS) and all(not t.is_cuda for t in cache.values())
    assert cache["pc"].dtype == cache["color"].dtype == cache["pc_ins"].dtype == torch.float32
    assert cache["group_label"].dtype == cache["seg_label"].dtype == cache["ngroup"].dtype == torch.int32
    assert tuple(cache["pc_ins"].shape) == (3, widest, NPOINT_INS, 3) and cache["ngroup"].tolist() == want["ngroup"]
    for i in range(3):
        assert np.array_equal(cache["pc"][i].numpy().view(np.int32), want["pc"][i].view(np.int32))
        assert np.array_equal(cache["color"][i].numpy().view(np.int32), want["color"][i].astype(np.float32).view(np.int32))
        assert np.array_equal(cache["group_label"][i].numpy(), want["group_label"][i]) and np.array_equal(cache["seg_label"][i].numpy(), want["seg_label"][i])
        g = want["pc_ins"][i].shape[0]
        assert np.array_equal(cache["pc_ins"][i, :g].numpy().view(np.int32), want["pc_ins"][i].view(np.int32)) and not cache["pc_ins"][i, g:].any()
        assert not cache["pc_ins"][i, want["ngroup"][i]:].any() and cache["pc_ins"][i, 1:want["ngroup"][i]].abs().sum() > 0
    assert cache["color"].min() >= 0 and cache["color"].max() <= 1
    # a scene below npoint was padded by the documented draws, the others sampled
    assert truth[order[1]]["n"] < NPOINT < truth[order[0]]["n"]
    batch = DeviceDataset(**{k: v.cuda() for k, v in cache.items()}).batch([0, 1])
    torch.cuda.synchronize()
    assert tuple(batch["pc"].shape) == (2, NPOINT, 3) and tuple(batch["pc_ins"].shape) == (2, widest, NPOINT_INS, 3)
    assert bool(torch.isfinite(batch["bbox_ins"]).all())


def test_make_cache_writes_what_train_loads(cache_case, tmp_path):
    def tool(name):
        spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        return module

    out = str(tmp_path / "train.pt")
    tool("make_cache").main(["--mesh_path", cache_case["mesh"], "--label_path", cache_case["label"], "--list", cache_case["list_path"], "--out", out,
                             "--npoint", str(NPOINT), "--npoint_ins", str(NPOINT_INS), "--seed", str(SEED), "--batch", "2"])
    train = tool("train")
    loaded = train.load_cache(out)
    assert tuple(loaded) == train.CACHE_KEYS
    for k in train.CACHE_KEYS:
        assert loaded[k].dtype == cache_case["cache"][k].dtype and torch.equal(loaded[k], cache_case["cache"][k])
    held = train.split(loaded, 0, 2, torch.device("cuda"), is_augment=False, permute_points=False)
    assert len(held) == 2 and held.pc.shape[1] == NPOINT
