"""Writes the fixtures that pin the stages the REFERENCE runs in plain numpy to the reference's own code:

    tests/golden/dataset/remap_ref.npz            dataset.py:48-56, 64-84 (+ changem :136-141)          -> gspn_amd.dataset.remap_labels
    tests/golden/dataset/getitem_ref.npz          dataset.py:168-188 (+ gen_rotation_matrix :127-134)   -> gspn_amd.dataset.augment_and_box
    tests/golden/data_prep/collect_label_ref.npz  data_prep.py:26-40                                    -> gspn_amd.data_prep.segment_labels
    tests/golden/predict/export_ref.npz           test.py:136-139, 155-205                              -> gspn_amd.predict.scene_predictions
    tests/golden/predict/iou_ref.npz              train.py:365-368, 385-386                             -> gspn_amd.predict.semantic_iou_counts, mean_iou

    python tools/make_golden_stages.py --reference /path/to/the/reference/checkout [--stage NAME]

The line ranges are cut out of the reference at generation time, dedented, exec'd with numpy (and scikit-learn's NearestNeighbors for the
export) and only inputs and outputs are stored -- nothing of the source, as with tools/make_golden_roi.py.  Every cut is guarded by its
line numbers and the sha256 of the cut lines.  The inputs come from np.random.default_rng(seed) here; they are stored next to the outputs,
so the tests never rebuild them.  Masks of 0 / 1 are stored packed (np.packbits).  Each fixture carries `cases` (names) and `case_counts`:
the generator prints one line per case and refuses to write a fixture in which a case does not occur, and
tests/test_cpu_reference_pins.py checks the stored flags against its own list.  No fixture may be larger than the largest file already
under tests/golden/.  Two runs write equal arrays."""
import argparse
import contextlib
import hashlib
import io
import os
import textwrap
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# name -> (file, first line, last line, sha256 of the cut lines joined by "\n")
CUTS = {
    "class_table": ("dataset.py", 48, 56, "86230dd1c69e79d993c042c5ecdbabe4494ae10b6fdec4c3f9b58270ea5c37fe"),
    "remap": ("dataset.py", 64, 84, "7645e748eedf80217b3ca0b5ed671c88e78bd582b417494c6c76185f5864691e"),
    "changem": ("dataset.py", 136, 141, "abfcf5a44f9687c92da1f4ad83e963187bc65356e74ddcb08da99669a532e85d"),
    "gen_rotation_matrix": ("dataset.py", 127, 134, "adafee9e9098855e15c9211cef5f9a2d35d7849dc62a8a08ad0c4184ba6d213d"),
    "getitem": ("dataset.py", 168, 188, "53c46adc61df3dd1ca9a547a573044cef30cac55fabfec15054e3ef6a2b4c54e"),
    "collect_label": ("data_prep.py", 26, 40, "bb81f5e729f8373a7968af9ba487b9a6f568ed90348da19a3a7b8b02279452d1"),
    "export_constants": ("test.py", 136, 139, "162845dca2cd5681521f189f0fe2e86ead7df9f280b68a97a9e579c07ef83dbb"),
    "export": ("test.py", 155, 205, "8a4b7faa564b116082ba6b03275ef18662d94da93508a2779ce32940680d6d21"),
    "iou_counts": ("train.py", 365, 368, "7f16b71b1f9130328e8ca69e9604199654b091008044bcd87ff82029cf198e6a"),
    "iou": ("train.py", 385, 386, "7207826e7df3d89f399b61ee99e84ecb6aa14e4911dd74bb8ed75de0200bdf98"),
}
FILES = {
    "remap": os.path.join("dataset", "remap_ref.npz"),
    "getitem": os.path.join("dataset", "getitem_ref.npz"),
    "collect_label": os.path.join("data_prep", "collect_label_ref.npz"),
    "export": os.path.join("predict", "export_ref.npz"),
    "iou": os.path.join("predict", "iou_ref.npz"),
}
MAX_POINTS = 4096


class Reference:
    """the checkout; cut(name) -> the compiled code of one guarded line range"""

    def __init__(self, root):
        self.root = root
        self.code = {}

    def cut(self, name):
        if name not in self.code:
            path, first, last, digest = CUTS[name]
            lines = open(os.path.join(self.root, path)).read().split("\n")[first - 1:last]
            found = hashlib.sha256("\n".join(lines).encode("utf-8")).hexdigest()
            if found != digest:
                raise SystemExit("%s:%d-%d is not the text this tool was written against (sha256 %s, expected %s)" % (path, first, last, found, digest))
            self.code[name] = compile(textwrap.dedent("\n".join(lines)), "<reference %s:%d-%d>" % (path, first, last), "exec")
        return self.code[name]

    def run(self, name, scope):
        exec(self.cut(name), scope)
        return scope


class Cases:
    """the named cases of one fixture with how often each occurs"""

    def __init__(self, stage):
        self.stage, self.names, self.counts = stage, [], []

    def add(self, name, count, note=""):
        print("%-14s %-28s %6d  %s" % (self.stage, name, int(count), note))
        self.names.append(name)
        self.counts.append(int(count))

    def arrays(self):
        missing = [n for n, c in zip(self.names, self.counts) if c <= 0]
        if missing:
            raise SystemExit("%s: the inputs do not contain the case(s) %s; nothing written" % (self.stage, ", ".join(missing)))
        return {"cases": np.array(self.names), "case_counts": np.array(self.counts, np.int64)}


def largest_existing(own):
    sizes = [os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(GOLDEN) for f in fs if os.path.join(d, f) not in own]
    return max(sizes)


def write(stage, store, cases, out_dir):
    store.update(cases.arrays())
    path = os.path.join(out_dir, FILES[stage])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = path + ".tmp.npz"
    np.savez_compressed(tmp, **store)
    size, limit = os.path.getsize(tmp), largest_existing([os.path.join(GOLDEN, f) for f in FILES.values()] + [tmp])
    if size > limit:
        os.remove(tmp)
        raise SystemExit("%s: %d bytes, larger than the largest file under tests/golden (%d); nothing written" % (stage, size, limit))
    with np.load(tmp, allow_pickle=False) as back:                       # every array loads without pickle
        assert sorted(back.files) == sorted(store)
    os.replace(tmp, path)
    print("wrote %s (%d bytes, limit %d)" % (path, size, limit))


# ---- remap: dataset.py:48-56, 64-84 ------------------------------------------------------------------------------------------------------

def run_remap(ref, group, seg):
    """one scan: raw group, seg (N,) -> curgroup int32, curseg int64, curngroup, and the class table of :48-56"""
    scope = {"np": np}
    ref.run("changem", scope)
    me = types.SimpleNamespace()
    me.changem = types.MethodType(scope["changem"], me)
    scope["self"] = me
    ref.run("class_table", scope)
    scope.update(curgroup=group.astype(np.int32), curseg=seg.astype(np.int32))               # as the label reader's .astype(np.int32)
    ref.run("remap", scope)
    return scope["curgroup"], scope["curseg"], int(scope["curngroup"]), scope["target_sem_idx"]


def remap_scans(rng):
    """name -> (group, seg): raw labels of seeded scans, group by group"""
    def scan(groups, pad):
        g = np.concatenate([np.full(len(s), gid) for gid, s in groups])
        s = np.concatenate([np.asarray(s) for _, s in groups])
        at = rng.permutation(len(g) + pad)
        g, s = np.concatenate((g, rng.integers(100, 104, pad))), np.concatenate((s, np.full(pad, 5)))      # four more valid groups
        return g[at].astype(np.int64), s[at].astype(np.int64)

    not_a_class = [0, 1, 2, 13, 15, 17, 23, 25, 32, 35, 37, 38]
    main = [
        (0, [3] * 40),                                              # class 1
        (1, [3] * 30 + [2] * 30),                                   # mean exactly 0.5
        (2, [3] * 20 + [4] * 20),                                   # 1.5
        (3, [4] * 20 + [5] * 20),                                   # 2.5
        (4, [3] * 50 + [0] * 51),                                   # just below 0.5
        (5, [3] * 51 + [1] * 50),                                   # just above 0.5
        (7, rng.integers(-5, 0, 33)),                               # id 6 absent; seg < 0
        (8, rng.integers(40, 60, 33)),                              # seg >= 40
        (9, rng.choice(not_a_class, 33)),                           # inside [0, 40) and no class
        (11, [39] * 25),                                            # id 10 absent
        (12, [39] * 1 + [0] * 35),                                  # 18 / 36: exactly 0.5 again
        (13, [39] * 1 + [2] * 34),                                  # 18 / 35
        (14, rng.choice([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39], 300)),
        (15, [2] * 1000 + [3] * 999),                               # 999 / 1999: closer to 0.5 from below
        (-1, rng.integers(-3, 45, 300)),
    ]
    scans = {"main": scan(main, 0)}
    g, s = scans["main"]
    assert len(g) <= MAX_POINTS - 2
    scans["main"] = (np.concatenate((g, [16, 16])), np.concatenate((s, [24, 24])))                          # the largest id is a valid group
    scans["background"] = scan([(0, rng.choice(not_a_class, 200)), (2, [3] * 50 + [2] * 50), (3, rng.integers(40, 99, 100)),
                                (-1, rng.integers(0, 40, 150))], 0)
    scans["one_group"] = scan([(-1, [3] * 100), (0, [2] * 90), (4, [16] * 77), (5, [3] * 10 + [0] * 11)], 0)
    scans["many"] = scan([(gid, [int(rng.choice([3, 4, 1, 0]))] * int(rng.integers(1, 30))) for gid in range(0, 100, 3)], 400)
    return scans


def make_remap(ref, out_dir):
    rng = np.random.default_rng(20240601)
    cases, store = Cases("remap"), {}
    seen = dict.fromkeys(("mean_exactly_0.5", "mean_exactly_1.5", "mean_exactly_2.5", "mean_just_below_0.5", "mean_just_above_0.5", "id_gap",
                          "group_minus_1", "seg_negative", "seg_40_or_more", "seg_in_range_not_a_class", "all_background", "one_valid_group",
                          "id_max_groups_minus_1_valid"), 0)
    names = []
    for name, (group, seg) in remap_scans(rng).items():
        assert len(group) == len(seg) <= MAX_POINTS
        out_group, out_seg, ngroup, table = run_remap(ref, group, seg)
        assert out_group.dtype == np.int32 and out_seg.dtype == np.int64 and out_group.shape == out_seg.shape == group.shape
        clamped = np.where((seg < 0) | (seg >= 40), 0, seg)
        assert np.array_equal(out_seg, np.asarray(table)[clamped])                        # how the flags below read a group's classes
        top = int(group.max())
        valid_ids = []
        for gid in range(top + 1):
            members = group == gid
            if not members.any():
                seen["id_gap"] += int(gid < top)
                continue
            mean = float(np.mean(out_seg[members]))
            for key, hit in (("mean_exactly_0.5", mean == 0.5), ("mean_exactly_1.5", mean == 1.5), ("mean_exactly_2.5", mean == 2.5),
                             ("mean_just_below_0.5", 0.49 < mean < 0.5), ("mean_just_above_0.5", 0.5 < mean < 0.51)):
                seen[key] += int(hit)
            new = np.unique(out_group[members])
            assert len(new) == 1
            if new[0] > 0:
                valid_ids.append(int(new[0]))
        assert valid_ids == list(range(1, ngroup)), "valid groups are numbered densely in ascending id"
        assert not out_group[group == -1].any()
        seen["group_minus_1"] += int((group == -1).sum() > 0)
        seen["seg_negative"] += int((seg < 0).sum())
        seen["seg_40_or_more"] += int((seg >= 40).sum())
        seen["seg_in_range_not_a_class"] += int(((seg > 0) & (seg < 40) & (np.asarray(table)[clamped] == 0)).sum())
        seen["all_background"] += int(ngroup == 1)
        seen["one_valid_group"] += int(ngroup == 2)
        seen["id_max_groups_minus_1_valid"] += int(out_group[group == top][0] == ngroup - 1 and ngroup > 1)
        print("remap          scan %-12s n %5d, ids -1..%d, ngroup %d" % (name, len(group), top, ngroup))
        names.append(name)
        store[name + "/group"], store[name + "/seg"] = group.astype(np.int32), seg.astype(np.int32)
        store[name + "/group_label"], store[name + "/seg_label"], store[name + "/ngroup"] = out_group, out_seg, np.array(ngroup, np.int64)
    for key, count in seen.items():
        cases.add(key, count)
    store["scans"] = np.array(names)
    write("remap", store, cases, out_dir)


# ---- getitem: dataset.py:168-188 ---------------------------------------------------------------------------------------------------------

def run_getitem(ref, pc, pc_ins, curngroup, ngroup, is_augment, seed):
    scope = {"np": np}
    ref.run("gen_rotation_matrix", scope)
    me = types.SimpleNamespace(ngroup=ngroup, npoint_ins=pc_ins.shape[1], is_augment=is_augment)
    me.gen_rotation_matrix = types.MethodType(scope["gen_rotation_matrix"], me)
    scope.update(self=me, pc=pc.copy(), pc_ins=pc_ins.copy(), curngroup=curngroup)
    np.random.seed(seed)
    ref.run("getitem", scope)
    out = {k: scope[k] for k in ("pc", "pc_ins_full", "group_indicator", "bbox_ins_full")}
    if is_augment:                                                                        # the same seed's two draws, in the run's order
        np.random.seed(seed)
        out["R"] = me.gen_rotation_matrix()
        out["t"] = np.random.normal(0, 1, [1, 3])
        padded = np.zeros((ngroup,) + pc_ins.shape[1:], np.float32)
        padded[:curngroup] = pc_ins
        assert out["R"].dtype == out["t"].dtype == np.float64
        assert np.array_equal(np.matmul(pc, out["R"]) + out["t"], out["pc"]), "the replay does not reproduce the run"
        assert np.array_equal(np.matmul(padded.reshape(-1, 3), out["R"]).reshape(padded.shape) + out["t"].reshape(1, 1, 3), out["pc_ins_full"])
    return out


def make_getitem(ref, out_dir):
    rng = np.random.default_rng(20240602)
    cases, store = Cases("getitem"), {}
    n, ngroup, m = 1024, 8, 128
    seen = dict.fromkeys(("plain", "plain_curngroup_equals_ngroup", "plain_curngroup_1", "augmented", "augmented_padded_rows_equal_t",
                          "augmented_box_spans_zero"), 0)
    names = []
    for name, augment, cur, seed in (("plain_full", False, ngroup, 1), ("plain_one", False, 1, 2), ("plain_some", False, 5, 3),
                                     ("aug_full", True, ngroup, 4), ("aug_some", True, 3, 5), ("aug_one", True, 1, 6), ("aug_far", True, 6, 7)):
        scale = np.float32(40.0 if name == "aug_far" else 8.0)
        pc = ((rng.random((n, 3), dtype=np.float32) - np.float32(0.5)) * scale)
        centre = (rng.random((cur, 1, 3), dtype=np.float32) - np.float32(0.5)) * scale
        pc_ins = (centre + (rng.random((cur, m, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(3.0)).astype(np.float32)
        pc_ins[0] = 0                                                                     # the background's row
        out = run_getitem(ref, pc, pc_ins, cur, ngroup, augment, seed)
        assert out["group_indicator"].dtype == np.int32 and out["bbox_ins_full"].dtype == np.float32
        assert out["pc_ins_full"].shape == (ngroup, m, 3) and out["bbox_ins_full"].shape == (ngroup, 6)
        store[name + "/pc"], store[name + "/pc_ins"], store[name + "/curngroup"] = pc, pc_ins, np.array(cur, np.int64)
        store[name + "/group_indicator"], store[name + "/bbox_ins_full"] = out["group_indicator"], out["bbox_ins_full"]
        if augment:
            assert out["pc"].dtype == out["pc_ins_full"].dtype == np.float64
            store[name + "/R"], store[name + "/t"] = out["R"], out["t"].reshape(3)
            rows = np.ones(ngroup, bool)
            rows[1:cur] = False
            assert np.array_equal(out["pc_ins_full"][rows], np.broadcast_to(out["t"].reshape(1, 1, 3), (int(rows.sum()), m, 3)))
            seen["augmented"] += 1
            seen["augmented_padded_rows_equal_t"] += int(rows.sum())
            hi, lo = out["pc_ins_full"].max(1), out["pc_ins_full"].min(1)
            seen["augmented_box_spans_zero"] += int(((hi > 0) & (lo < 0))[1:cur].sum())
        else:
            assert out["pc"].dtype == out["pc_ins_full"].dtype == np.float32
            assert np.array_equal(out["pc"], pc) and not np.signbit(pc_ins[pc_ins == 0]).any()
            seen["plain"] += 1
            seen["plain_curngroup_equals_ngroup"] += int(cur == ngroup)
            seen["plain_curngroup_1"] += int(cur == 1)
        # the float32 a placeholder makes of the result (the float64 result itself is not kept)
        store[name + "/pc_out"], store[name + "/pc_ins_full"] = out["pc"].astype(np.float32), out["pc_ins_full"].astype(np.float32)
        print("getitem        %-12s augment %d curngroup %d of %d, %d x %d instance points" % (name, augment, cur, ngroup, cur, m))
        names.append(name)
    for key, count in seen.items():
        cases.add(key, count)
    store["runs"] = np.array(names)
    write("getitem", store, cases, out_dir)


# ---- collect_label: data_prep.py:26-40 ---------------------------------------------------------------------------------------------------

def run_collect_label(ref, seg_indices, seg_groups):
    scope = {"np": np, "aggreData": {"segGroups": seg_groups}, "segsData": {"segIndices": [int(v) for v in seg_indices]}}
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        ref.run("collect_label", scope)
    lines = text.getvalue().split("\n")
    assert lines[-1] == "" and len(set(lines[:-1])) <= 1                                  # nothing but that one line, repeated
    return scope["outGroups"], len(lines) - 1


def make_collect_label(ref, out_dir):
    rng = np.random.default_rng(20240603)
    cases, store = Cases("collect_label"), {}
    seen = dict.fromkeys(("segment_in_two_groups", "segment_twice_in_one_group", "segment_named_three_times", "named_segment_without_vertex",
                          "vertex_in_no_group", "object_id_0", "no_pairs", "group_without_segments"), 0)
    names = []
    for name, n, ngroup in (("scan", 2500, 9), ("no_pairs", 300, 0), ("dense", 1201, 5)):
        nseg = 6 * max(ngroup, 1) + 5
        seg_indices = rng.integers(0, nseg, n) * 5 + 1                                    # sparse ids
        if ngroup:
            seg_indices[seg_indices == 1] = 6                                             # segment 1 has no vertex and is named below
        groups = []
        owner = rng.integers(0, ngroup + 1, nseg)                                         # == ngroup: in no group
        for g in range(ngroup):
            # objectIds as ScanNet's: the group's number, not in the order of the file
            groups.append({"id": g, "objectId": int((g * 4) % ngroup), "segments": [int(s) * 5 + 1 for s in np.nonzero(owner == g)[0]], "label": "thing"})
        if ngroup:
            groups.append({"id": ngroup, "objectId": int(ngroup + 3), "segments": [], "label": "empty"})
            first, last = groups[0]["segments"], groups[ngroup - 1]["segments"]
            assert len(first) >= 3 and len(last) >= 2
            last.append(first[0])                                                         # named by two groups: the last wins
            groups[2]["segments"].append(first[1])
            last.append(first[1])                                                         # three times
            groups[1]["segments"].append(groups[1]["segments"][0])                        # twice inside one group
            groups[3]["segments"] += [1, 1, 3]                                            # 1 and 3: no vertex has them (ids are 5 k + 1)
        pairs = [(s, g["objectId"]) for g in groups for s in g["segments"]]
        label, lines = run_collect_label(ref, seg_indices, groups)
        assert label.shape == (n,) and np.array_equal(label, np.round(label))
        label = label.astype(np.int32)
        pair_segment = np.array([s for s, _ in pairs], np.int32).reshape(-1)
        pair_object = np.array([o for _, o in pairs], np.int32).reshape(-1)
        named = np.bincount(pair_segment[np.isin(pair_segment, seg_indices)], minlength=1) if len(pairs) else np.zeros(1, np.int64)
        group_of_pair = np.array([i for i, g in enumerate(groups) for _ in g["segments"]], np.int64)
        two_groups = sum(len(set(group_of_pair[pair_segment == s])) > 1 for s in np.unique(pair_segment) if s in seg_indices) if len(pairs) else 0
        in_group = sum(len(g["segments"]) - len(set(g["segments"])) for g in groups if set(g["segments"]) & set(seg_indices.tolist()))
        seen["segment_in_two_groups"] += two_groups
        seen["segment_twice_in_one_group"] += in_group
        seen["segment_named_three_times"] += int((named >= 3).sum())
        seen["named_segment_without_vertex"] += int((~np.isin(pair_segment, seg_indices)).sum())
        seen["vertex_in_no_group"] += int((label == -1).sum())
        seen["object_id_0"] += int((label == 0).sum())
        seen["no_pairs"] += int(len(pairs) == 0)
        seen["group_without_segments"] += sum(len(g["segments"]) == 0 for g in groups)
        print("collect_label  %-10s n %5d, %2d groups, %3d pairs, %d lines" % (name, n, len(groups), len(pairs), lines))
        names.append(name)
        store[name + "/seg_indices"], store[name + "/pair_segment"], store[name + "/pair_object"] = seg_indices.astype(np.int32), pair_segment, pair_object
        store[name + "/group_sizes"] = np.array([len(g["segments"]) for g in groups], np.int64)
        store[name + "/label"], store[name + "/conflicts"] = label, np.array(lines, np.int64)
    for key, count in seen.items():
        cases.add(key, count)
    store["scans"] = np.array(names)
    write("collect_label", store, cases, out_dir)


# ---- export: test.py:136-139, 155-205 ----------------------------------------------------------------------------------------------------

def run_export(ref, ep):
    """ep: the arrays sess.run returns and the batch's points, each with its leading batch axis of 1"""
    from sklearn.neighbors import NearestNeighbors
    scope = {"np": np, "NearestNeighbors": NearestNeighbors, "batch_pc": ep["pc"].copy()}
    for key in ("rpointnet_mask_selected", "pc_coord_cropped_final_unnormalized", "detections", "sem_class_logits", "pc_seed", "fb_prob"):
        scope[key] = ep[key].copy()
    ref.run("export_constants", scope)
    ref.run("export", scope)
    return {k: scope[k] for k in ("group_label_pred", "seg_label_pred", "confidence_pred", "sem_conf", "fb_conf", "detections")}


def two_nearest_differ(query, points):
    """query (n, 3), points (k, 3) int64 on one raster -> (n,) bool: the nearest and the second nearest point are at different distances"""
    if len(query) == 0 or len(points) < 2:
        return np.ones(len(query), bool)
    d = ((query[:, None, :] - points[None, :, :]) ** 2).sum(-1)
    d.partition(1, axis=1)
    return d[:, 0] != d[:, 1]


def nearest(query, points):
    return np.argmin(((query[:, None, :] - points[None, :, :]) ** 2).sum(-1), 1)


def export_scene(rng, n, r, p, nc, ns, kind):
    """One scene on rasters: points and seeds at multiples of 1/16 in [0, 16) x [0, 16) x [0, 12), crop points at multiples of 1/64, box
    centres at multiples of 1/16 and sizes at multiples of 1/8 -- every difference, square and sum of squares is a small integer over 4096,
    exact in float32 and float64 in any order.  Integers here are in units of 1/64.  kind: 'general', 'second_only', 'none'."""
    extent = np.array([256, 256, 192])
    seeds = np.unique(rng.integers(0, extent, (4 * ns, 3)), axis=0)
    seeds = seeds[rng.permutation(len(seeds))[:ns]] * 4
    pts = rng.integers(0, extent, (n, 3)) * 4
    while True:
        bad = ~two_nearest_differ(pts, seeds)
        if not bad.any():
            break
        pts[bad] = rng.integers(0, extent, (int(bad.sum()), 3)) * 4
    det = np.zeros((r, 8), np.float32)
    crops = np.zeros((r, p, 3), np.int64)
    masks = (1.0 / (1.0 + np.exp(-2.5 * rng.standard_normal((r, p))))).astype(np.float32)
    notes = {"face": [], "at_threshold": None, "empty": None}
    common, rare = np.arange(1, nc - 3), np.arange(nc - 3, nc)
    cls = rng.choice(common, r)
    if kind == "general":
        cls[rng.permutation(r)[:max(r // 4, 2)]] = rng.choice(rare, max(r // 4, 2))
    elif kind == "second_only":
        cls[:] = rng.choice(rare, r)
    dead = rng.permutation(r)[:max(r // 5, 1)] if kind != "none" else np.arange(r)
    cls[dead] = 0
    live = [k for k in range(r) if cls[k] > 0]
    special = {}
    if kind == "general":
        special = dict(zip(("empty", "face_lo", "face_hi", "at_threshold"), live))
        for key in ("face_lo", "face_hi", "at_threshold"):
            cls[special[key]] = rng.choice(common)
        notes["empty"] = special["empty"]
    for k in range(r):
        half = rng.integers(8, 25, 3) * 8                                                  # half sizes 1 .. 3 in steps of 1/8
        centre = pts[rng.integers(n)].copy()
        if special.get("empty") == k:
            centre, half = np.array([512, 512, 896]), np.array([48, 48, 48])                # z in [13.25, 14.75]: no point is there
        if special.get("face_lo") == k:
            centre[0] += half[0]                                                           # the lower x face passes through that point
        if special.get("face_hi") == k:
            centre[1] -= half[1]                                                           # the upper y face
        lo, hi = centre - half, centre + half
        det[k, :3], det[k, 3:6] = centre / 64.0, half / 32.0
        inside = np.all((pts >= lo) & (pts <= hi), 1)
        if special.get("face_lo") == k or special.get("face_hi") == k:
            masks[k] = (0.5 + 0.45 * rng.random(p)).astype(np.float32)                      # every inside point is in the mask
            notes["face"].append(k)
        while True:
            c = np.unique(rng.integers(lo, hi + 1, (2 * p, 3)), axis=0)
            c = c[rng.permutation(len(c))[:p]]
            if len(c) == p and two_nearest_differ(pts[inside], c).all():
                break
        crops[k] = c
        if special.get("at_threshold") == k:
            assert inside.sum() >= 8
            order = np.argsort(-np.bincount(nearest(pts[inside], c), minlength=p), kind="stable")      # the crop points most points take
            masks[k, order[0::2][:p // 4]] = np.float32(0.4)
            masks[k, order[1::2][:p // 4]] = np.nextafter(np.float32(0.4), np.float32(0))
            notes["at_threshold"] = k
    det[:, 6] = cls
    det[:, 7] = (0.05 + 0.9 * rng.random(r)).astype(np.float32)
    logits = (np.round(2.0 * rng.standard_normal((n, nc)) * 8) / 8).astype(np.float32)      # eighths: they compress
    logits[:, nc - 3:] -= 6.0
    fb1 = (np.round((0.05 + 0.9 * rng.random(ns)) * 1024) / 1024).astype(np.float32)
    fb_prob = np.stack((1 - fb1, fb1), -1).astype(np.float32)
    ep = {"pc": (pts / 64.0).astype(np.float32)[None], "rpointnet_mask_selected": masks[None],
          "pc_coord_cropped_final_unnormalized": (crops / 64.0).astype(np.float32)[None], "detections": det[None],
          "sem_class_logits": logits[None], "pc_seed": (seeds / 64.0).astype(np.float32)[None], "fb_prob": fb_prob[None]}
    assert np.array_equal(ep["pc"][0].astype(np.float64) * 64, pts) and np.array_equal(ep["pc_coord_cropped_final_unnormalized"][0].astype(np.float64) * 64, crops)
    assert ep["pc"].max() < 64 and ep["pc_coord_cropped_final_unnormalized"].max() < 64
    return ep, pts, crops, notes


def rows_of(out, ep):
    """the input row of every output row, by its score (pairwise distinct)"""
    score = ep["detections"][0, :, 7]
    assert len(np.unique(score)) == len(score)
    return np.array([int(np.nonzero(score == s)[0][0]) for s in out["detections"][:, 7]], np.int64)


def make_export(ref, out_dir):
    rng = np.random.default_rng(20240604)
    cases, store = Cases("export"), {}
    seen = dict.fromkeys(("class_0_rows", "box_without_point_in_second_partition", "both_partitions", "empty_first_partition", "no_detection",
                          "point_on_box_face_in_mask", "mask_value_float32_0.4_set", "mask_value_below_0.4_clear"), 0)
    names = []
    p, nc, ns = 64, 19, 128
    for name, n, r, kind in (("general", 3001, 16, "general"), ("second_only", 2999, 16, "second_only"), ("none", 3000, 16, "none"),
                             ("few", 3072, 5, "general")):
        ep, pts, crops, notes = export_scene(rng, n, r, p, nc, ns, kind)
        first = run_export(ref, ep)                                                        # for the confidences: they do not read column 7
        rows = rows_of(first, ep)
        conf = first["sem_conf"] * first["fb_conf"]
        top = first["confidence_pred"] == 1.0
        for part in (top, ~top):                                                           # a ladder of ratio 0.97 per partition, scores below 1
            at = np.nonzero(part & (conf > 0))[0]
            if len(at):
                step = rng.permutation(len(at))
                ep["detections"][0, rows[at], 7] = (0.9 * conf[at].min() * 0.97 ** step / conf[at]).astype(np.float32)
        out = run_export(ref, ep)
        rows = rows_of(out, ep)
        nd = len(rows)
        assert out["group_label_pred"].dtype == np.int32 and out["group_label_pred"].shape == (nd, n)
        assert out["seg_label_pred"].dtype == np.int64 and out["confidence_pred"].dtype == out["sem_conf"].dtype == out["fb_conf"].dtype == np.float64
        cls = ep["detections"][0, :, 6]
        assert sorted(rows.tolist()) == np.nonzero(cls > 0)[0].tolist()
        top = out["confidence_pred"] == 1.0
        assert not top[int(top.sum()):].any() and (out["confidence_pred"][~top] == 0.97).all()
        score = out["detections"][:, 7] * out["sem_conf"] * out["fb_conf"]
        for part in (top, ~top):
            s = score[part]
            assert np.all(s[:-1] > s[1:]) and np.all(s[:-1] - s[1:] > 1e-4 * s[:-1]), "adjacent scores of a partition are too close"
        for v in (out["sem_conf"], out["fb_conf"]):
            assert np.all(np.abs(v - 0.01) > 1e-4 * 0.01), "a confidence is within 1e-4 of its threshold"
        # the tie condition, on the detections the reference keeps
        seeds = np.round(ep["pc_seed"][0].astype(np.float64) * 64).astype(np.int64)
        assert two_nearest_differ(pts, seeds).all()
        on_face = 0
        for k in np.nonzero(cls > 0)[0]:
            lo = np.round((ep["detections"][0, k, :3] - ep["detections"][0, k, 3:6] / 2).astype(np.float64) * 64).astype(np.int64)
            hi = np.round((ep["detections"][0, k, :3] + ep["detections"][0, k, 3:6] / 2).astype(np.float64) * 64).astype(np.int64)
            inside = np.all((pts >= lo) & (pts <= hi), 1)
            assert len(np.unique(crops[k], axis=0)) == p and two_nearest_differ(pts[inside], crops[k]).all()
            row = out["group_label_pred"][rows.tolist().index(k)]
            assert not row[~inside].any()
            face = inside & np.any((pts == lo) | (pts == hi), 1)
            on_face += int(row[face].sum())
            if k in notes["face"]:
                assert face.any() and row[inside].all()
            if k == notes["empty"]:
                assert not inside.any() and not row.any()
                seen["box_without_point_in_second_partition"] += int(out["confidence_pred"][rows.tolist().index(k)] == 0.97)
            if k == notes["at_threshold"]:
                value = ep["rpointnet_mask_selected"][0, k][nearest(pts[inside], crops[k])]
                at, below = value == np.float32(0.4), value == np.nextafter(np.float32(0.4), np.float32(0))
                assert row[inside][at].all() and not row[inside][below].any()
                seen["mask_value_float32_0.4_set"] += int(at.sum())
                seen["mask_value_below_0.4_clear"] += int(below.sum())
        seen["class_0_rows"] += int((cls <= 0).sum())
        seen["point_on_box_face_in_mask"] += on_face
        seen["both_partitions"] += int(top.any() and (~top).any())
        seen["empty_first_partition"] += int(nd > 0 and not top.any())
        seen["no_detection"] += int(nd == 0)
        print("export         %-12s n %d, %2d rows: %2d kept, %2d first / %2d second partition, %d mask points" % (
            name, n, r, nd, int(top.sum()), int((~top).sum()), int(out["group_label_pred"].sum())))
        names.append(name)
        for key, value in ep.items():
            assert value.dtype == np.float32
            store[name + "/" + key] = value[0]
        store[name + "/rows"] = rows
        store[name + "/group_label_pred"] = np.packbits(out["group_label_pred"].astype(np.uint8), axis=1)
        for key in ("seg_label_pred", "confidence_pred", "sem_conf", "fb_conf"):
            store[name + "/" + key] = out[key]
    for key, count in seen.items():
        cases.add(key, count)
    store["scenes"] = np.array(names)
    write("export", store, cases, out_dir)


# ---- iou: train.py:365-368, 385-386 ------------------------------------------------------------------------------------------------------

def make_iou(ref, out_dir):
    rng = np.random.default_rng(20240605)
    cases, store = Cases("iou"), {}
    nc, absent = 19, (7, 18)
    scope = {"np": np, "cum_intersection": np.zeros(nc - 1), "cum_union": np.zeros(nc - 1)}
    ties = first_is_0 = zeros = 0
    for batch, (b, n) in enumerate(((2, 1500), (3, 1001))):
        logits = (np.round(rng.standard_normal((b, n, nc)) * 4) / 4).astype(np.float32)     # quarters: many exact ties
        logits[:, :, list(absent)] -= 100.0                                                # never predicted
        labels = rng.integers(0, nc, (b, n)).astype(np.int32)
        labels[np.isin(labels, absent)] = 0                                                # and never a label
        best = logits.max(-1, keepdims=True)
        ties += int(((logits == best).sum(-1) > 1).sum())
        first_is_0 += int(((logits == best).sum(-1) > 1)[logits[:, :, 0] == best[:, :, 0]].sum())
        store["batch%d/logits" % batch], store["batch%d/labels" % batch] = logits, labels
        scope.update(pred_val=logits.copy(), sem_labels_val=labels.copy())
        ref.run("iou_counts", scope)
        store["batch%d/cum_intersection" % batch] = scope["cum_intersection"].astype(np.int64)
        store["batch%d/cum_union" % batch] = scope["cum_union"].astype(np.int64)
        assert np.array_equal(store["batch%d/cum_union" % batch], scope["cum_union"])
        zeros += int((labels == 0).sum())
    ref.run("iou", scope)
    assert scope["iou"].dtype == np.float64 and scope["iou"].shape == (nc - 1,)
    store["iou"], store["meaniou"] = scope["iou"], np.array(scope["meaniou"], np.float64)
    cases.add("labels_0", zeros)
    cases.add("exact_logit_ties", ties, "%d with class 0 among the maxima" % first_is_0)
    cases.add("class_absent_from_both", int((scope["cum_union"] == 0).sum()), "iou there %s" % scope["iou"][scope["cum_union"] == 0].tolist())
    cases.add("tie_with_class_0_first", first_is_0)
    print("iou            mean %.17g" % scope["meaniou"])
    store["batches"] = np.array(2, np.int64)
    write("iou", store, cases, out_dir)


STAGES = {"remap": make_remap, "getitem": make_getitem, "collect_label": make_collect_label, "export": make_export, "iou": make_iou}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GSPN_REFERENCE"), help="checkout of the reference (or GSPN_REFERENCE)")
    ap.add_argument("--stage", choices=sorted(STAGES), help="one stage only (default: all)")
    ap.add_argument("--out", default=GOLDEN, help="the directory to write under (default: tests/golden)")
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or GSPN_REFERENCE) is required")
    ref = Reference(a.reference)
    for stage in ([a.stage] if a.stage else list(STAGES)):
        STAGES[stage](ref, a.out)


if __name__ == "__main__":
    main()
