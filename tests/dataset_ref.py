"""A numpy restatement of the compute of the reference's dataset.py -- the label remap (:48-56, 64-84), the scene and instance resampling
(:89-105, 107-118) and the batch assembly with augmentation and boxes (:168-188) -- written from the reference's text for the tests of
gspn_amd/dataset.py, and the seeded scenes those tests run on.  The FPS is the CPU oracle's (oracle/gspn_oracle.c) on each host-compacted
instance, as the reference feeds its own kernel; where the reference draws with np.random.choice the draws are the documented ones of
gspn_roi_rand32 (tests/roi_ref.rand32)."""
import numpy as np

from oracle import oracle as O
from tests import roi_ref as RR

VALID_CLASS_IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
SCENE_STREAM = 0xFFFFFFFE


def padding_draws(seed, scene, a, ndraw, count):
    """draw t = 0..ndraw-1 of stream (scene, a): (uint64(rand32(seed, scene, a, t)) * count) >> 32"""
    return RR.rank_of(RR.rand32(seed, scene, a, np.arange(ndraw)), count)


# ---- :48-56, 64-84 -----------------------------------------------------------------------------------------------------------------

def remap_labels(group, seg):
    """one scene: group, seg (N,) int -> group_label, seg_label (N,) int64, ngroup"""
    table = np.zeros(40, np.int64)
    table[VALID_CLASS_IDS] = np.arange(1, len(VALID_CLASS_IDS) + 1)
    seg = np.array(seg, np.int64)
    seg[(seg >= 40) | (seg < 0)] = 0
    seg = table[seg]
    ngroup = int(group.max()) + 1
    target = np.zeros(1 + max(ngroup, 0), np.int64)                 # target[i + 1]: new id of group i; target[0]: of label -1
    count = 0
    for i in range(ngroup):
        members = group == i
        if members.sum() == 0:
            continue
        if int(np.round(np.mean(seg[members]))) != 0:               # float64 mean, half to even
            count += 1
            target[i + 1] = count
    return target[np.asarray(group, np.int64) + 1], seg, count + 1


# ---- :89-105 -----------------------------------------------------------------------------------------------------------------------

def resample_choice(pc, npoint, seed, scene):
    """one scene: the indices dataset.py:89-105 keeps, in order"""
    n = pc.shape[0]
    if npoint < n:
        return O.farthest_point_sample(npoint, pc[None])[0].astype(np.int64)
    return np.concatenate((np.arange(n), padding_draws(seed, scene, SCENE_STREAM, npoint - n, n)))


# ---- :107-118 ----------------------------------------------------------------------------------------------------------------------

def instance_sets(pc, label, ngroup, m, seed):
    """pc (B, N, 3), label (B, N) -> idx (B, ngroup, m) int32 (-1: background / empty), pts (B, ngroup, m, 3), count (B, ngroup) int32"""
    b = pc.shape[0]
    idx = -np.ones((b, ngroup, m), np.int32)
    pts = np.zeros((b, ngroup, m, 3), np.float32)
    count = np.zeros((b, ngroup), np.int32)
    for s in range(b):
        for j in range(ngroup):
            members = np.nonzero(label[s] == j)[0]
            c = len(members)
            count[s, j] = c
            if j == 0 or c == 0:
                continue
            if m < c:
                choice = O.farthest_point_sample(m, pc[s][members][None])[0]
            else:
                choice = np.concatenate((np.arange(c), padding_draws(seed, s, j, m - c, c)))
            idx[s, j] = members[choice]
            pts[s, j] = pc[s][idx[s, j]]
    return idx, pts, count


# ---- :168-188 ----------------------------------------------------------------------------------------------------------------------

def rigid(x, rotation, translation):
    """np.matmul(x, R) + t in float64, then the float32 of the placeholder the result is fed to.  x (..., 3) of one scene."""
    return (np.matmul(x.reshape(-1, 3).astype(np.float64), rotation) + translation.reshape(1, 3)).astype(np.float32).reshape(x.shape)


def boxes(pc_ins):
    """pc_ins (..., M, 3) -> (..., 6): [(max + min) / 2, max - min]"""
    hi, lo = pc_ins.max(-2), pc_ins.min(-2)
    return np.concatenate(((hi + lo) / 2, hi - lo), -1).astype(np.float32)


def group_indicator(ngroup_valid, ngroup):
    return (np.arange(ngroup)[None, :] < np.asarray(ngroup_valid)[:, None]).astype(np.int32)


# ---- the scenes of tests/test_gpu_dataset.py ---------------------------------------------------------------------------------------

SIZES = ([300, 17000, 9000, 4500, 1300, 600, 68], [20000, 1800, 400, 64, 10, 0, 2500, 7994])


def labelled_scene(n, sizes, ngroup, seed, lattice):
    """one scene of n points whose group j has sizes[j] points (0 past the list), labels shuffled over the scene by a seeded permutation.
    lattice: every instance's points on a 12^3 grid of pitch 0.25 (exact distances, ties everywhere); else synth.cloud_d."""
    from gspn_amd import synth
    rng = np.random.default_rng(seed)
    sizes = list(sizes) + [0] * (ngroup - len(sizes))
    assert sum(sizes) == n
    label = np.repeat(np.arange(ngroup), sizes)[rng.permutation(n)]
    pc = synth.cloud_d(n, seed)
    if lattice:
        for j, c in enumerate(sizes):
            pc[label == j] = (rng.integers(0, 12, (c, 3)) * 0.25).astype(np.float32)
    return pc, label.astype(np.int64)
