"""A restatement of the loops of the reference's data_prep.py and of its label writer, written from the reference's text for the tests of
gspn_amd/data_prep.py and gspn_amd/io_util.py, and the writers of the files those tests read -- a struct-packed binary PLY in ScanNet's
layout (alpha column, face element) and the three label files of a scan -- which use nothing of gspn_amd.io_util."""
import json
import os
import struct

import numpy as np


# ---- data_prep.py:25-40 ------------------------------------------------------------------------------------------------------------------

def collect_label_loop(seg_indices, seg_groups):
    """segIndices (n,) and aggregation.json's segGroups -> (labels (n,) int64, the number of Error! lines).  Every vertex starts at -1; the
    groups in file order, the segments of a group in order: every vertex of the segment takes the group's objectId, and a line is printed
    when one of them was no longer -1."""
    seg_indices = np.asarray(seg_indices)
    out = np.zeros(seg_indices.shape) - 1
    errors = 0
    for group in seg_groups:
        for segment in group["segments"]:
            at = np.where(seg_indices == segment)
            if not all(out[at] == -1):
                errors += 1
            out[at] = group["objectId"]
    return out.astype(np.int64), errors


def pairs_of(seg_groups):
    """segGroups flattened in file order -> (segments, objectIds)"""
    return ([s for g in seg_groups for s in g["segments"]], [g["objectId"] for g in seg_groups for _ in g["segments"]])


def label_lines(label):
    """the bytes io_util.write_label_txt writes: '{0}\\n' per label"""
    return "".join("{0}\n".format(int(v)) for v in label).encode("ascii")


# ---- files in ScanNet's layout -----------------------------------------------------------------------------------------------------------

def write_binary_ply(path, xyz, color, label=None, faces=4, comments=("VCGLIB generated",)):
    """binary little-endian PLY as ScanNet's _vh_clean_2.ply: x y z float, red green blue alpha uchar, label ushort when given (its
    .labels.ply), then `faces` triangles in a face element with a list property"""
    n = xyz.shape[0]
    head = ["ply", "format binary_little_endian 1.0"] + ["comment " + c for c in comments] + ["element vertex %d" % n]
    head += ["property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue",
             "property uchar alpha"]
    if label is not None:
        head.append("property ushort label")
    head += ["comment between the elements", "element face %d" % faces, "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        for i in range(n):
            f.write(struct.pack("<fffBBBB", float(xyz[i, 0]), float(xyz[i, 1]), float(xyz[i, 2]), int(color[i, 0]), int(color[i, 1]),
                                int(color[i, 2]), 255))
            if label is not None:
                f.write(struct.pack("<H", int(label[i])))
        for k in range(faces):
            f.write(struct.pack("<Biii", 3, k % n, (k + 1) % n, (k + 2) % n))


def write_scan(root, scan, xyz, color, sem, seg_indices, seg_groups):
    """one scan under <root>/mesh/scans and <root>/label/scans, the five files data_prep.py reads"""
    mesh, label = os.path.join(root, "mesh/scans", scan), os.path.join(root, "label/scans", scan)
    os.makedirs(mesh, exist_ok=True)
    os.makedirs(label, exist_ok=True)
    write_binary_ply(os.path.join(mesh, scan + "_vh_clean_2.ply"), xyz, color)
    write_binary_ply(os.path.join(label, scan + "_vh_clean_2.labels.ply"), xyz, color, sem)
    with open(os.path.join(label, scan + ".aggregation.json"), "w") as f:
        json.dump({"sceneId": "scannet." + scan, "segGroups": seg_groups}, f)
    with open(os.path.join(label, scan + "_vh_clean_2.0.010000.segs.json"), "w") as f:
        json.dump({"sceneId": scan, "segIndices": [int(v) for v in seg_indices]}, f)


def labelled_scan(n, ngroup, seed, sem_of_group, twice=0):
    """a seeded scan of n points: cloud_d (a tenth duplicates), colours, about 6 segments per group plus segments in no group;
    group g has objectId g and semantic label sem_of_group[g].  twice: that many segments are named a second time, by the last group."""
    from gspn_amd import synth
    rng = np.random.default_rng(seed)
    xyz = synth.cloud_d(n, seed)
    color = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    nseg = 6 * ngroup + 3
    seg_indices = rng.integers(0, nseg, n) * 7 + 2                                # sparse ids
    owner = rng.integers(0, ngroup + 1, nseg)                                     # == ngroup: in no group
    seg_groups = [{"id": g, "objectId": g, "segments": [int(s) * 7 + 2 for s in np.nonzero(owner == g)[0]], "label": "thing"}
                  for g in range(ngroup)]
    for s in rng.choice(np.nonzero(owner < ngroup - 1)[0], twice, replace=False):
        seg_groups[-1]["segments"].append(int(s) * 7 + 2)
    ins, _ = collect_label_loop(seg_indices, seg_groups)
    sem = np.where(ins >= 0, np.asarray(sem_of_group)[np.maximum(ins, 0)], 0).astype(np.int64)
    return xyz, color, sem, seg_indices, seg_groups
