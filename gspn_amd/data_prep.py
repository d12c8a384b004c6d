"""The compute of the reference's data_prep.py, and the file half of its dataset.py, on the device: from a ScanNet download to the training
cache tools/train.py --cache loads.

  segment_labels     data_prep.py:25-40   the (segment, objectId) pairs of segGroups onto the vertices: gspn_segment_labels
                                          (csrc/data_prep.hip), a table and a gather instead of groups x segments passes of np.where
  read_segments      :15, :27             the segIndices of a scan's segs.json as they are (also what segments.compact_segments takes)
  collect_label      :13-45               the three label files of a scan -> semantic labels, instance labels, the count of Error! lines
  downsample_scans   :76-87               scans of unequal size to nsample points by farthest_point_sample, one scan or several per call
  prepare_scans      :48-92               the driver: <dataset>/mesh/scans, <dataset>/label/scans -> <out>/mesh/scans/<scan>.ply,
                                          <out>/label/scans/sem_<scan>.txt and group_<scan>.txt
  build_cache        dataset.py:38-125    those files -> the six cache tensors of gspn_amd.train.DeviceDataset, composed from
                                          dataset.remap_labels / resample_scene / instance_point_sets

The seed rule of build_cache.  The reference draws its duplicates (dataset.py:101, :117) with np.random; here they are draws of
gspn_roi_rand32(seed, row, stream, t), where row is a scene's row in the call it shares with other scenes.  Scenes of unequal size cannot
share a call, so build_cache forms chunks: for every distinct point count, the scenes of that count in list order, at most `batch` to a
chunk.  A chunk's calls get the seed `seed + (list index of the chunk's first scene)` and a scene's row is its place in the chunk.  The cache
is therefore a function of the files, `seed` and `batch` alone.

The .npz pickle of dataset.py:125 is not written: the cache is the torch.save dict tools/train.py defines.  No CPU fallback for the
kernel-backed ops."""
import json
import os
import sys

import numpy as np
import torch

from . import _lib as L
from . import io_util
from .dataset import instance_point_sets, remap_labels, resample_scene
from .tf_sampling import farthest_point_sample

__all__ = ["SEGMENT_LABELS_MAX_N", "SEGMENT_LABELS_MAX_S", "FPS_SEGMENTS_MAX_N", "CACHE_KEYS", "segment_labels", "read_segments", "collect_label",
           "downsample_scans", "prepare_scans", "build_cache"]

SEGMENT_LABELS_MAX_N = 1 << 24    # GSPN_SEGMENT_LABELS_MAX_N of include/gspn_hip.h
SEGMENT_LABELS_MAX_S = 1 << 26    # GSPN_SEGMENT_LABELS_MAX_S
FPS_SEGMENTS_MAX_N = 32768        # the limit of dataset.fps_segments (gspn_fps_segments): one scene's instances are sampled on one CU each
CACHE_KEYS = ("pc", "color", "group_label", "seg_label", "pc_ins", "ngroup")      # as tools/train.py names them

_INT_DTYPES = (torch.int32, torch.int64)


def _ints(t, name):
    """an integer vector; TypeError / ValueError otherwise"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype not in _INT_DTYPES:
        raise ValueError("%s must be int32 or int64, got %s" % (name, t.dtype))
    if t.dim() != 1:
        raise ValueError("%s must be 1-D, got shape %s" % (name, tuple(t.shape)))
    return t


# ---- data_prep.py:25-40 ------------------------------------------------------------------------------------------------------------------

def segment_labels(seg_indices, pair_segment, pair_object, num_segments=None):
    """data_prep.py:25-40.  seg_indices (n,) int: the segment of every vertex; pair_segment, pair_object (p,) int: the (segment, objectId)
    pairs of segGroups flattened in file order, group by group and segment by segment -> label (n,) int32, conflicts (1,) int32.
    label[v] is the objectId of the LAST pair naming seg_indices[v], -1 without one (and for an entry that is negative or >= num_segments).
    conflicts is the number of Error! lines of the reference: over the segments that have a vertex, the pairs naming it minus one.  A pair
    whose segment no vertex has does nothing.  p == 0 is legal.
    num_segments: one more than the largest entry of seg_indices, when the caller knows it (collect_label does, from the file); with None it
    is read back from the device.  Raises ValueError for a negative objectId (-1 is the reference's value of an unlabelled vertex), which
    reads pair_object's minimum back: this is preparation, not a step.  Device tensors only."""
    seg_indices, pair_segment, pair_object = _ints(seg_indices, "seg_indices"), _ints(pair_segment, "pair_segment"), _ints(pair_object, "pair_object")
    n, p = seg_indices.shape[0], pair_segment.shape[0]
    if pair_object.shape[0] != p:
        raise ValueError("segment_labels: one objectId per pair, got %d segments and %d objectIds" % (p, pair_object.shape[0]))
    if n < 1:
        raise ValueError("segment_labels: no vertex")
    if n > SEGMENT_LABELS_MAX_N:
        raise NotImplementedError("segment_labels: n <= %d (got %d)" % (SEGMENT_LABELS_MAX_N, n))
    seg = L.need(seg_indices.int(), torch.int32, 1, "seg_indices")
    dev = seg.device
    if p > 0:
        pseg = L.need(pair_segment.int(), torch.int32, 1, "pair_segment")
        pobj = L.need(pair_object.int(), torch.int32, 1, "pair_object")
        lo, hi = (int(v) for v in torch.stack(torch.aminmax(pair_object)).tolist())         # one read-back
        if lo < 0:
            raise ValueError("segment_labels: objectIds must not be negative (found %d)" % lo)
        if hi >= (1 << 31):
            raise ValueError("segment_labels: objectIds must fit an int32 (found %d)" % hi)
    else:
        pseg = pobj = torch.zeros(1, dtype=torch.int32, device=dev)              # never read: the entry point wants pointers that are not null
    s = int(seg_indices.max()) + 1 if num_segments is None else int(num_segments)
    s = max(s, 1)                                                                 # nothing but negative entries: one empty segment
    if s > SEGMENT_LABELS_MAX_S:
        raise NotImplementedError("segment_labels: segment ids < %d (got %d)" % (SEGMENT_LABELS_MAX_S, s - 1))
    lib = L.lib()
    ws_bytes = int(lib.gspn_segment_labels_ws_bytes(s))
    if ws_bytes < 0:
        L.check(ws_bytes, "segment_labels")
    with torch.no_grad():
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
        label = torch.empty(n, dtype=torch.int32, device=dev)
        conflicts = torch.empty(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.gspn_segment_labels(n, p, s, L.ptr(seg), L.ptr(pseg), L.ptr(pobj), L.ptr(ws), L.ptr(label), L.ptr(conflicts), L.stream()),
                    "segment_labels")
    return label, conflicts


def flatten_seg_groups(seg_groups):
    """aggregation.json's segGroups -> (segments, objectIds), one entry per (group, segment) in file order"""
    segments, objects = [], []
    for group in seg_groups:
        segments.extend(int(v) for v in group["segments"])
        objects.extend([int(group["objectId"])] * len(group["segments"]))
    return segments, objects


def read_segments(label_path, scan):
    """<label_path>/<scan>/<scan>_vh_clean_2.0.010000.segs.json -> its segIndices, (V,) np.int64: the raw id of every vertex's segment of the
    mesh's over-segmentation, what collect_label joins into instances and segments.compact_segments numbers for a vote."""
    with open(os.path.join(label_path, scan, scan) + "_vh_clean_2.0.010000.segs.json") as f:
        return np.asarray(json.load(f)["segIndices"], dtype=np.int64).reshape(-1)


def collect_label(label_path, scan, device=None):
    """data_prep.py:13-45.  Reads <label_path>/<scan>/<scan>.aggregation.json, <scan>_vh_clean_2.0.010000.segs.json and
    <scan>_vh_clean_2.labels.ply -> sem_label (n,) int32, ins_label (n,) int32 on `device`, and the number of Error! lines as an int."""
    device = torch.device("cuda" if device is None else device)
    base = os.path.join(label_path, scan, scan)
    with open(base + ".aggregation.json") as f:
        seg_groups = json.load(f)["segGroups"]
    seg_indices = read_segments(label_path, scan)
    _, sem = io_util.read_label_ply(base + "_vh_clean_2.labels.ply")
    if sem.shape[0] != seg_indices.shape[0]:
        raise ValueError("collect_label: %s: %d vertices in the labels file, %d segment entries" % (scan, sem.shape[0], seg_indices.shape[0]))
    if seg_indices.size and (seg_indices.min() < -(1 << 31) or seg_indices.max() >= (1 << 31)):
        raise ValueError("collect_label: %s: a segment id does not fit an int32" % scan)
    segments, objects = flatten_seg_groups(seg_groups)
    inside = [(a, b) for a, b in zip(segments, objects) if -(1 << 31) <= a < (1 << 31)]          # any other segment no vertex can have
    pair_segment = torch.tensor([a for a, _ in inside], dtype=torch.int32).to(device)
    pair_object = torch.tensor([b for _, b in inside], dtype=torch.int64).to(device)
    num_segments = int(seg_indices.max()) + 1 if seg_indices.size else 1
    ins, conflicts = segment_labels(torch.from_numpy(seg_indices.astype(np.int32)).to(device), pair_segment, pair_object, num_segments)
    return torch.from_numpy(sem.astype(np.int32)).to(device), ins, int(conflicts.item())


# ---- data_prep.py:76-87 ------------------------------------------------------------------------------------------------------------------

def _check_scan(at, scan):
    if len(scan) != 4:
        raise ValueError("downsample_scans: scan %d must be (xyz, color, sem, ins), got %d entries" % (at, len(scan)))
    xyz = scan[0]
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError("downsample_scans: scan %d: xyz must be a float32 tensor (n, 3) with n >= 1" % at)
    for name, t in zip(("color", "sem", "ins"), scan[1:]):
        if not isinstance(t, torch.Tensor) or t.shape[0] != xyz.shape[0]:
            raise ValueError("downsample_scans: scan %d: %s must be a tensor of %d rows" % (at, name, xyz.shape[0]))
    L.need(xyz, torch.float32, 2, "xyz")


def downsample_scans(scans, nsample=30000, batch=1):
    """data_prep.py:76-87 for a list of scans.  scans: [(xyz (n, 3) float32, color (n, 3) uint8, sem (n,), ins (n,))] device tensors of unequal
    n -> the list of the same four per scan, in the caller's order.  A scan with n <= nsample is returned as it is; the others are the rows
    farthest_point_sample(nsample, xyz) picks.
    batch > 1: the scans to sample are sorted by size and up to `batch` of them share one farthest_point_sample call, each padded to the
    chunk's largest with copies of its own point 0.  Padding changes no pick: a copy of point 0 has distance 0 from the first pick (point 0)
    onward, and where every distance is 0 the reference's tie order (k mod 512, k) chooses index 0 with or without the copies -- so every pick
    stays below the real n.  The status word of a multi-CU launch is waited for (L.check_async(block=True)) before a chunk's picks are used."""
    nsample, batch = int(nsample), int(batch)
    if nsample < 1 or batch < 1:
        raise ValueError("downsample_scans: nsample and batch must be positive, got %d and %d" % (nsample, batch))
    scans = [tuple(scan) for scan in scans]
    for at, scan in enumerate(scans):
        _check_scan(at, scan)
    out = list(scans)
    todo = sorted((at for at, scan in enumerate(scans) if scan[0].shape[0] > nsample), key=lambda at: (scans[at][0].shape[0], at))
    with torch.no_grad():
        for lo in range(0, len(todo), batch):
            chunk = todo[lo:lo + batch]
            width = max(scans[at][0].shape[0] for at in chunk)
            first = scans[chunk[0]][0]
            cloud = torch.empty((len(chunk), width, 3), dtype=torch.float32, device=first.device)
            for row, at in enumerate(chunk):
                xyz = scans[at][0]
                cloud[row, :xyz.shape[0]] = xyz
                cloud[row, xyz.shape[0]:] = xyz[0]
            idx = farthest_point_sample(nsample, cloud)
            L.check_async(block=True)
            for row, at in enumerate(chunk):
                pick = idx[row].long()
                out[at] = tuple(t[pick] for t in scans[at])
    return out


# ---- data_prep.py:48-92 ------------------------------------------------------------------------------------------------------------------

def prepare_scans(dataset_path, out_path, nsample=30000, batch=1, scans=None, device=None, log=None):
    """The __main__ of data_prep.py.  For every scan under <dataset_path>/mesh/scans (sorted by name: the reference's os.listdir order is not
    defined; or the names of `scans`) reads <scan>/<scan>_vh_clean_2.ply and the labels of collect_label under <dataset_path>/label/scans,
    downsamples to nsample points and writes <out_path>/mesh/scans/<scan>.ply, <out_path>/label/scans/sem_<scan>.txt and group_<scan>.txt.
    `batch` scans are read, sampled (downsample_scans(..., batch)) and written at a time.  Where the reference prints Error!, a line with the
    scan's conflict count goes to stderr.  -> [(scan, points read, points written, conflicts)]"""
    device = torch.device("cuda" if device is None else device)
    batch = int(batch)
    if batch < 1:
        raise ValueError("prepare_scans: batch must be positive, got %d" % batch)
    mesh_path, label_path = os.path.join(dataset_path, "mesh/scans"), os.path.join(dataset_path, "label/scans")
    names = sorted(os.listdir(mesh_path)) if scans is None else [str(v) for v in scans]
    out_mesh, out_label = os.path.join(out_path, "mesh/scans"), os.path.join(out_path, "label/scans")
    os.makedirs(out_mesh, exist_ok=True)
    os.makedirs(out_label, exist_ok=True)
    log = (lambda line: print(line, flush=True)) if log is None else log
    report = []
    for lo in range(0, len(names), batch):
        window, loaded = names[lo:lo + batch], []
        for scan in window:
            scene = io_util.read_color_ply(os.path.join(mesh_path, scan, scan + "_vh_clean_2.ply"))
            sem, ins, conflicts = collect_label(label_path, scan, device)
            if sem.shape[0] != scene.shape[0]:
                raise ValueError("prepare_scans: %s: %d vertices in the mesh, %d labels" % (scan, scene.shape[0], sem.shape[0]))
            if conflicts:
                print("Error! %s: %d (segment, objectId) pairs name a segment that was already labelled" % (scan, conflicts), file=sys.stderr, flush=True)
            xyz = torch.from_numpy(np.ascontiguousarray(scene[:, :3], dtype=np.float32)).to(device)
            color = torch.from_numpy(np.ascontiguousarray(scene[:, 3:6]).astype(np.uint8)).to(device)
            loaded.append((xyz, color, sem, ins))
            report.append([scan, scene.shape[0], 0, conflicts])
        for at, (xyz, color, sem, ins) in enumerate(downsample_scans(loaded, nsample, batch)):
            scan = window[at]
            rows = np.concatenate((xyz.cpu().numpy(), color.cpu().numpy().astype(np.float32)), 1)
            io_util.write_color_ply(rows, os.path.join(out_mesh, scan + ".ply"))
            io_util.write_label_txt(sem.cpu().numpy(), os.path.join(out_label, "sem_" + scan + ".txt"))
            io_util.write_label_txt(ins.cpu().numpy(), os.path.join(out_label, "group_" + scan + ".txt"))
            report[lo + at][2] = rows.shape[0]
            log("Scene " + str(lo + at) + " done!")
    return [tuple(r) for r in report]


# ---- dataset.py:38-125 -------------------------------------------------------------------------------------------------------------------

def cache_chunks(sizes, batch):
    """the chunks of build_cache's seed rule: for every distinct point count in order of first appearance, the list indices of the scenes of
    that count in list order, at most `batch` to a chunk -> [[list index, ...], ...], ordered by their first scene"""
    by_size = {}
    for at, n in enumerate(sizes):
        by_size.setdefault(int(n), []).append(at)
    chunks = [members[lo:lo + batch] for members in by_size.values() for lo in range(0, len(members), batch)]
    return sorted(chunks, key=lambda chunk: chunk[0])


def build_cache(mesh_path, label_path, list_path, npoint=18000, npoint_ins=512, seed=0, batch=8, device=None):
    """dataset.py:38-125 on prepare_scans' output.  list_path: a file of scan names, one per line; per name <mesh_path>/<name>.ply,
    <label_path>/group_<name>.txt and sem_<name>.txt -> {"pc", "color" (S, npoint, 3) float32 (color = uint8 / 255), "group_label", "seg_label"
    (S, npoint) int32, "pc_ins" (S, G, npoint_ins, 3) float32 with G the list's largest ngroup and zero rows beyond a scene's, "ngroup" (S,)
    int32}, on the host: what tools/train.py --cache loads once torch.save has written it.
    Instances are drawn from the un-resampled scene (:110), so a scene of more than 32768 points -- fps_segments' limit -- raises ValueError:
    downsample it first (prepare_scans' nsample = 30000 does).  Chunks and seeds: the module's docstring.  max_groups of remap_labels is the
    chunk's max(group) + 1 and the chunk's ngroup sizes pc_ins, each read back once per chunk: this is preparation, not the step."""
    device = torch.device("cuda" if device is None else device)
    npoint, npoint_ins, seed, batch = int(npoint), int(npoint_ins), int(seed), int(batch)
    if npoint < 1 or npoint_ins < 1 or batch < 1:
        raise ValueError("build_cache: npoint, npoint_ins and batch must be positive, got %d, %d and %d" % (npoint, npoint_ins, batch))
    names = [name for name in io_util.read_txt(list_path) if name]
    if not names:
        raise ValueError("build_cache: %s names no scan" % list_path)
    scenes = []
    for name in names:
        rows = io_util.read_color_ply(os.path.join(mesh_path, name + ".ply"))
        group = io_util.read_label_txt(os.path.join(label_path, "group_" + name + ".txt")).astype(np.int32)
        seg = io_util.read_label_txt(os.path.join(label_path, "sem_" + name + ".txt")).astype(np.int32)
        n = rows.shape[0]
        if n < 1 or group.shape[0] != n or seg.shape[0] != n:
            raise ValueError("build_cache: %s: %d points, %d group labels, %d semantic labels" % (name, n, group.shape[0], seg.shape[0]))
        if n > FPS_SEGMENTS_MAX_N:
            raise ValueError("build_cache: %s has %d points; fps_segments, which draws the instances from the whole scene, takes at most %d "
                             "(downsample the scan first: tools/data_prep.py)" % (name, n, FPS_SEGMENTS_MAX_N))
        scenes.append((rows[:, :3].astype(np.float32), rows[:, 3:6].astype(np.float32) / 255.0, group, seg))
    total = len(scenes)
    pc = torch.empty((total, npoint, 3), dtype=torch.float32)
    color = torch.empty((total, npoint, 3), dtype=torch.float32)
    group_label = torch.empty((total, npoint), dtype=torch.int32)
    seg_label = torch.empty((total, npoint), dtype=torch.int32)
    ngroup = torch.empty(total, dtype=torch.int32)
    sets = [None] * total
    with torch.no_grad():
        for chunk in cache_chunks([s[0].shape[0] for s in scenes], batch):
            stack = lambda k: torch.from_numpy(np.stack([scenes[at][k] for at in chunk])).to(device)
            cur_pc, cur_color, cur_group, cur_seg = stack(0), stack(1), stack(2), stack(3)
            chunk_seed = seed + chunk[0]
            new_group, new_seg, cur_ngroup = remap_labels(cur_group, cur_seg, max(int(cur_group.max()) + 1, 1))
            res = resample_scene(cur_pc, cur_color, new_group, new_seg, npoint, chunk_seed)
            pc_ins = instance_point_sets(cur_pc, new_group, int(cur_ngroup.max()), npoint_ins, chunk_seed).cpu()
            L.check_async(block=True)
            at = torch.tensor(chunk)
            pc[at], color[at] = res[0].cpu(), res[1].cpu()
            group_label[at], seg_label[at] = res[2].int().cpu(), res[3].int().cpu()
            ngroup[at] = cur_ngroup.cpu()
            for row, i in enumerate(chunk):
                sets[i] = pc_ins[row]
    widest = max(s.shape[0] for s in sets)
    all_ins = torch.zeros((total, widest, npoint_ins, 3), dtype=torch.float32)
    for i, s in enumerate(sets):
        all_ins[i, :s.shape[0]] = s
    return {"pc": pc, "color": color, "group_label": group_label, "seg_label": seg_label, "pc_ins": all_ins, "ngroup": ngroup}
