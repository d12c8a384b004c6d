"""The compute of the reference's dataset.py on the device: from a labelled scan to the inputs of rpointnet() -- pc_ins, bbox_ins,
group_indicator -- without its per-instance session.run loop.

  remap_labels         :48-56, 64-84   semantic labels to 0..18, valid groups renumbered 1..count (plain torch; CPU tensors allowed)
  resample_scene       :89-105         every scene to npoint points (farthest_point_sample, or duplicates drawn with replacement)
  fps_segments         :107-118        EVERY instance of every scene to npoint_ins points in one call: gspn_inverse_lists over the labels,
  instance_point_sets                  then gspn_fps_segments (csrc/sampling_segments.hip), one workgroup per (scene, group)
  augment_and_box      :168-188        group_indicator, rotation about z + translation, bbox_ins

The reference compacts curpc[curgroup == j] on the host and runs its FPS kernel once per instance at b = 1; here the compaction is the
stable partition of gspn_inverse_lists and the picks are those of that kernel on each compacted instance (ties on the compacted position).
Where the reference draws with np.random (the duplicates of :101, :117) the stream is gspn_roi_rand32 (include/gspn_hip.h) read from a
one-element int64 device tensor, as in roi.py: a captured call draws afresh once the caller has added to that tensor.  Reading the PLY / txt
files (:28-36, 57-63) and composing these functions into the cache of :38-125 is gspn_amd/data_prep.py (build_cache) over
gspn_amd/io_util.py.  No CPU fallback for the kernel-backed ops."""
import math

import torch

from . import _lib as L
from . import invlists
from .roi import seed_tensor
from .spn_boxes import points_bbox
from .tf_sampling import farthest_point_sample, gather_point

__all__ = ["fps_segments", "instance_point_sets", "resample_scene", "remap_labels", "augment_and_box", "VALID_CLASS_IDS", "SCENE_STREAM"]

VALID_CLASS_IDS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)           # :48
SCENE_STREAM = 0xFFFFFFFE          # `a` of the draws of resample_scene in gspn_roi_rand32(seed, scene, a, t): no group has this number

_INT_DTYPES = (torch.int32, torch.int64)


def _labels(t, name, shape=None):
    """an integer label tensor (B, N); ValueError otherwise"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype not in _INT_DTYPES:
        raise ValueError("%s must be int32 or int64, got %s" % (name, t.dtype))
    if t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError("%s must be %s, got %s" % (name, "(B, N)" if shape is None else tuple(shape), tuple(t.shape)))
    return t


def _cloud(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != torch.float32:
        raise ValueError("%s must be torch.float32, got %s" % (name, t.dtype))
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("%s must be (B, N, 3), got %s" % (name, tuple(t.shape)))
    return t


# ---- gspn_roi_rand32 in torch: int64 arithmetic wraps modulo 2^64 like the generator's uint64; only the right shifts need a mask ----

def _s64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


_M1, _M2, _GOLD = _s64(0xBF58476D1CE4E5B9), _s64(0x94D049BB133111EB), _s64(0x9E3779B97F4A7C15)


def _shr(z, k):
    return (z >> k) & ((1 << (64 - k)) - 1)


def _mix(z):
    z = z ^ _shr(z, 30)
    z = z * _M1
    z = z ^ _shr(z, 27)
    z = z * _M2
    return z ^ _shr(z, 31)


def _rand_rank(seed, scenes, a, draws, count):
    """(uint64(gspn_roi_rand32(seed, scene, a, t)) * count) >> 32 for scene < scenes, t < draws -> (scenes, draws) int64.  seed: a
    one-element int64 tensor; everything stays on its device."""
    dev = seed.device
    st = _mix(seed.reshape(1) + _GOLD * torch.arange(1, scenes + 1, dtype=torch.int64, device=dev))
    word = torch.arange(draws, dtype=torch.int64, device=dev) | _s64(int(a) << 32)
    r32 = _shr(_mix(st.unsqueeze(1) ^ word), 32)
    return (r32 * int(count)) >> 32                                                        # r32 < 2^32, count < 2^31: no overflow


# ---- :107-118 ----------------------------------------------------------------------------------------------------------------------

def fps_segments(pc, group_label, ngroup, npoint_ins, seed=0):
    """dataset.py:107-118 for a batch of scenes.  pc (B, N, 3), group_label (B, N) int (0 = background; labels outside [0, ngroup) belong to
    no group) -> idx (B, ngroup, npoint_ins) int32 indices into the scene, pts (B, ngroup, npoint_ins, 3) = pc[idx], count (B, ngroup)
    int32 = the group sizes.  Per group of c points, members in ascending point index:
      group 0 and empty groups    idx -1, pts 0 (:108-109)
      c > npoint_ins              farthest point sampling of the compacted instance pc[label == j], as the reference's kernel picks (:111-113)
      c == npoint_ins             the members in order (:114-115)
      c < npoint_ins              the members, then draws with replacement from gspn_roi_rand32(seed, scene, group, t) (:116-118)
    seed: an int or a one-element int64 device tensor (roi.seed_tensor).  N <= 32768.  Captures in a graph when seed is a tensor."""
    pc, group_label = _cloud(pc, "pc"), _labels(group_label, "group_label")
    if tuple(group_label.shape) != tuple(pc.shape[:2]):
        raise ValueError("fps_segments: pc must be (B, N, 3) and group_label (B, N), got %s and %s" % (tuple(pc.shape), tuple(group_label.shape)))
    g, m = int(ngroup), int(npoint_ins)
    if g < 1 or m < 1:
        raise ValueError("fps_segments: ngroup and npoint_ins must be positive, got %d and %d" % (g, m))
    pc = L.need(pc.detach(), torch.float32, 3, "pc")
    label = L.need(group_label.int(), torch.int32, 2, "group_label")
    b, n, _ = pc.shape
    seed = seed_tensor(seed, pc.device)
    order, offsets = invlists.inverse_lists(label, g)
    lib = L.lib()
    ws_bytes = int(lib.gspn_fps_segments_ws_bytes(b, n, g))
    if ws_bytes < 0:
        L.check(ws_bytes, "fps_segments")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pc.device)
    idx = torch.empty((b, g, m), dtype=torch.int32, device=pc.device)
    pts = torch.empty((b, g, m, 3), dtype=torch.float32, device=pc.device)
    count = torch.empty((b, g), dtype=torch.int32, device=pc.device)
    with torch.cuda.device(pc.device):
        L.check(lib.gspn_fps_segments(b, n, g, m, L.ptr(seed), L.ptr(pc), L.ptr(order), L.ptr(offsets), L.ptr(ws), L.ptr(idx), L.ptr(pts),
                                      L.ptr(count), L.stream()), "fps_segments")
    return idx, pts, count


def instance_point_sets(pc, group_label, ngroup, npoint_ins, seed=0):
    """pc_ins (B, ngroup, npoint_ins, 3) of rpointnet(): dataset.py:107-118 with the zero padding of :171-172 -- ngroup is the batch's
    (the dataset's) maximum, and the groups a scene does not have are empty, hence rows of zeros like the background's."""
    return fps_segments(pc, group_label, ngroup, npoint_ins, seed)[1]


# ---- :89-105 -----------------------------------------------------------------------------------------------------------------------

def resample_scene(pc, color, group_label, seg_label, npoint, seed=0):
    """dataset.py:89-105 for a batch of scenes of equal size.  pc, color (B, N, 3), group_label, seg_label (B, N) -> the same four with
    npoint points.  N > npoint: the points farthest_point_sample(npoint, pc) picks (:90-94); N == npoint: copies; N < npoint: all points
    in order, then npoint - N duplicates, draw t of scene s being point (uint64(gspn_roi_rand32(seed, s, 0xFFFFFFFE, t)) * N) >> 32
    (:101-105 with np.random.choice).  seed as in fps_segments."""
    pc, color = _cloud(pc, "pc"), _cloud(color, "color")
    b, n, _ = pc.shape
    group_label, seg_label = _labels(group_label, "group_label", (b, n)), _labels(seg_label, "seg_label", (b, n))
    if tuple(color.shape) != (b, n, 3):
        raise ValueError("resample_scene: color must be %s, got %s" % ((b, n, 3), tuple(color.shape)))
    npoint = int(npoint)
    if npoint < 1:
        raise ValueError("resample_scene: npoint must be positive, got %d" % npoint)
    pc = L.need(pc.detach(), torch.float32, 3, "pc")
    if n == npoint:
        return pc.clone(), color.clone(), group_label.clone(), seg_label.clone()
    if n > npoint:
        choice = farthest_point_sample(npoint, pc)
        new_pc = gather_point(pc, choice)
        choice = choice.long()
    else:
        seed = seed_tensor(seed, pc.device)
        draws = _rand_rank(seed, b, SCENE_STREAM, npoint - n, n)
        choice = torch.cat((torch.arange(n, dtype=torch.int64, device=pc.device).expand(b, n), draws), 1)
        new_pc = torch.gather(pc, 1, choice.unsqueeze(-1).expand(-1, -1, 3))
    return (new_pc, torch.gather(color, 1, choice.unsqueeze(-1).expand(-1, -1, 3)), torch.gather(group_label, 1, choice),
            torch.gather(seg_label, 1, choice))


# ---- :48-56, 64-84 -----------------------------------------------------------------------------------------------------------------

def remap_labels(group, seg, max_groups):
    """dataset.py:48-56, 64-84.  group, seg (B, N) int, the raw instance and semantic labels of a scan; max_groups: a static bound on the
    group ids (the reference's np.max(curgroup) + 1) -> group_label, seg_label (B, N) int64, ngroup (B,) int32 on the inputs' device.
    seg outside [0, 40) goes to 0, then through the VALID_CLASS_IDS table to 0..18.  A group is valid when it has points and
    round(mean(seg_label of its points)) != 0, the mean in float64 and rounded half to even as numpy does; valid groups are renumbered
    1..count in ascending original id, every other point -- -1 and ids >= max_groups included -- gets 0.  ngroup = count + 1 (group 0 is
    the background).  Plain torch, no host synchronisation; runs on CPU tensors too."""
    group, seg = _labels(group, "group"), _labels(seg, "seg", group.shape)
    g = int(max_groups)
    if g < 1:
        raise ValueError("remap_labels: max_groups must be positive, got %d" % g)
    dev = group.device
    table = torch.zeros(40, dtype=torch.int64, device=dev)
    table[torch.tensor(VALID_CLASS_IDS, device=dev)] = torch.arange(1, len(VALID_CLASS_IDS) + 1, device=dev)
    seg = seg.long()
    seg_label = table[torch.where((seg < 0) | (seg >= 40), torch.zeros_like(seg), seg)]
    group = group.long()
    inside = (group >= 0) & (group < g)
    gi = group.clamp(0, g - 1)
    members = torch.zeros((group.shape[0], g), dtype=torch.int64, device=dev).scatter_add_(1, gi, inside.long())
    seg_sum = torch.zeros((group.shape[0], g), dtype=torch.int64, device=dev).scatter_add_(1, gi, seg_label * inside)
    mean = seg_sum.double() / members.clamp(min=1).double()
    valid = (members > 0) & (torch.round(mean) != 0)
    new_id = torch.cumsum(valid.long(), 1) * valid
    group_label = torch.where(inside, torch.gather(new_id, 1, gi), torch.zeros_like(group))
    return group_label, seg_label, (valid.sum(1) + 1).int()


# ---- :168-188 ----------------------------------------------------------------------------------------------------------------------

def _rigid(x, rotation, translation):
    """(x.double() @ R + t).float() for x (B, ..., 3): numpy's float64 product, rounded by the reference's float32 placeholder"""
    shape = x.shape
    x = x.double().reshape(shape[0], -1, 3)
    r = rotation.unsqueeze(1)                                            # (B, 1, 3, 3)
    y = (x[..., 0:1] * r[:, :, 0, :] + x[..., 1:2] * r[:, :, 1, :]) + x[..., 2:3] * r[:, :, 2, :]
    return (y + translation.unsqueeze(1)).float().reshape(shape)


def augment_and_box(pc, pc_ins, ngroup_valid, rotation=None, translation=None, seed=0):
    """dataset.py:168-188.  pc (B, N, 3), pc_ins (B, G, M, 3), ngroup_valid: (B,) int tensor (remap_labels' ngroup) or an int ->
    pc, pc_ins augmented, group_indicator (B, G) int32 (1 for the first ngroup_valid groups, :169-170), bbox_ins (B, G, 6).
    rotation (B, 3, 3) and translation (B, 3), float64 as numpy makes them (:127-134, :181): x -> (x.double() @ R + t).float(), applied to
    every row of pc_ins as in the reference, the all-zero rows included.  With None, the angle (uniform in [0, 2 pi)) and the N(0, 1)
    translation come from a torch.Generator seeded with `seed` -- an int, or the VALUE of a one-element int64 tensor read at call time,
    which synchronises: that form does not capture in a graph (pass rotation and translation there).
    bbox_ins = [(max + min) / 2, max - min] over each row of the augmented pc_ins (:186-188), by gspn_points_bbox."""
    pc, pc_ins = _cloud(pc, "pc"), L.need(pc_ins, torch.float32, 4, "pc_ins")
    pc = L.need(pc, torch.float32, 3, "pc")
    b, g = pc_ins.shape[:2]
    if pc_ins.shape[3] != 3 or pc.shape[0] != b:
        raise ValueError("augment_and_box: pc must be (B, N, 3) and pc_ins (B, G, M, 3), got %s and %s" % (tuple(pc.shape), tuple(pc_ins.shape)))
    dev = pc.device
    if isinstance(ngroup_valid, torch.Tensor):
        if ngroup_valid.dtype not in _INT_DTYPES or tuple(ngroup_valid.shape) != (b,):
            raise ValueError("augment_and_box: ngroup_valid must be a (B,) int tensor or an int, got %s %s" % (ngroup_valid.dtype, tuple(ngroup_valid.shape)))
        valid = ngroup_valid.to(dev).long().unsqueeze(1)
    else:
        valid = int(ngroup_valid)
    group_indicator = (torch.arange(g, device=dev).unsqueeze(0).expand(b, g) < valid).int()
    if rotation is None or translation is None:
        gen = torch.Generator().manual_seed(int(seed.item()) if isinstance(seed, torch.Tensor) else int(seed))
        angle = torch.rand(b, generator=gen, dtype=torch.float64) * (2 * math.pi)
        drawn_t = torch.randn((b, 3), generator=gen, dtype=torch.float64)
        if rotation is None:
            cos, sin, zero, one = torch.cos(angle), torch.sin(angle), torch.zeros(b, dtype=torch.float64), torch.ones(b, dtype=torch.float64)
            rotation = torch.stack((cos, sin, zero, -sin, cos, zero, zero, zero, one), 1).reshape(b, 3, 3)      # :131-133
        if translation is None:
            translation = drawn_t
    rotation, translation = torch.as_tensor(rotation), torch.as_tensor(translation)
    if tuple(rotation.shape) != (b, 3, 3) or tuple(translation.shape) != (b, 3):
        raise ValueError("augment_and_box: rotation must be (B, 3, 3) and translation (B, 3), got %s and %s"
                         % (tuple(rotation.shape), tuple(translation.shape)))
    rotation, translation = rotation.to(dev, torch.float64), translation.to(dev, torch.float64)
    pc, pc_ins = _rigid(pc, rotation, translation), _rigid(pc_ins, rotation, translation)
    return pc, pc_ins, group_indicator, points_bbox(pc_ins)
