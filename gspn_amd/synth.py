"""Synthetic point clouds of SURVEY.md section 8(d): U (uniform), D (duplicates: tie stress, mirrors
dataset.py:100-105), S (room-like surfaces), and spn_batch: a labelled scene batch for the shape proposal stage.
numpy.random.default_rng(seed), float32."""
import numpy as np


def cloud_u(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def cloud_d(n, seed, frac=0.1):
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3), dtype=np.float32)
    k = max(1, int(n * frac))
    src = rng.integers(0, max(1, n - k), size=k)
    x[n - k:] = x[src]
    return x


def cloud_s(n, seed):
    """points on the faces of an 8x6x3 m room plus 20 random boxes"""
    rng = np.random.default_rng(seed)
    ext = np.array([8.0, 6.0, 3.0], np.float32)
    boxes = [(np.zeros(3, np.float32), ext)]
    for _ in range(20):
        lo = rng.random(3).astype(np.float32) * ext * 0.8
        sz = (rng.random(3).astype(np.float32) * 0.9 + 0.1).astype(np.float32)
        boxes.append((lo, sz))
    which = rng.integers(0, len(boxes), size=n)
    face = rng.integers(0, 6, size=n)
    uv = rng.random((n, 3), dtype=np.float32)
    los = np.stack([bx[0] for bx in boxes])[which]          # (n, 3) float32
    szs = np.stack([bx[1] for bx in boxes])[which]
    pts = (los + uv * szs).astype(np.float32)
    ax = face // 2
    rows = np.arange(n)
    pts[rows, ax] = los[rows, ax] + np.where(face % 2 == 1, szs[rows, ax], np.float32(0.0)).astype(np.float32)
    return pts


def scan_vertices(pc, seg_label, group_label, v, seed, jitter=0.01):
    """A synthetic scan around one scene: pc (n, 3) f32, seg_label, group_label (n,) -> xyz (v, 3) f32, seg_label, group_label (v,) i32.
    The first n rows are the scene as it is -- the network's scene is a subset of its scan's vertices, as in real data --, the other
    v - n are seeded scene points moved by `jitter` * N(0, 1) per axis, which inherit their point's labels."""
    pc = np.asarray(pc, np.float32)
    n = pc.shape[0]
    if pc.shape != (n, 3) or len(seg_label) != n or len(group_label) != n or v < n:
        raise ValueError("scan_vertices: pc (n, 3) with n labels of each kind and v >= n expected, got %s, %d, %d and v = %d"
                         % (pc.shape, len(seg_label), len(group_label), v))
    rng = np.random.default_rng(7919 * int(seed) + 3)
    parent = rng.integers(0, n, size=v - n)
    moved = (pc[parent] + np.float32(jitter) * rng.standard_normal((v - n, 3)).astype(np.float32)).astype(np.float32)
    at = np.concatenate((np.arange(n), parent))
    return (np.concatenate((pc, moved)), np.asarray(seg_label)[at].astype(np.int32), np.asarray(group_label)[at].astype(np.int32))


def scan_segments(xyz, seg_label, group_label, cell, seed):
    """A synthetic over-segmentation of a scan: xyz (v, 3) f32, seg_label, group_label (v,), cell > 0 -> raw segment ids (v,) int64.
    Segments are nested inside (seg_label, group_label): within one instance a segment is the vertices of one cube of side `cell` of the
    coordinates (floor(xyz / cell)).  The ids are seeded: increasing with gaps of 1 to 4, then handed to the segments in shuffled
    order, as a real file's ids are sparse and unordered (segments.compact_segments is there to be exercised)."""
    xyz = np.asarray(xyz, np.float32)
    v = xyz.shape[0]
    if xyz.shape != (v, 3) or len(seg_label) != v or len(group_label) != v or not cell > 0:
        raise ValueError("scan_segments: xyz (v, 3) with v labels of each kind and cell > 0 expected, got %s, %d, %d and cell = %r"
                         % (xyz.shape, len(seg_label), len(group_label), cell))
    cubes = np.floor(xyz.astype(np.float64) / float(cell)).astype(np.int64)
    keys = np.concatenate((np.asarray(seg_label, np.int64).reshape(v, 1), np.asarray(group_label, np.int64).reshape(v, 1), cubes), axis=1)
    _, inverse = np.unique(keys, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    k = int(inverse.max()) + 1 if v else 0
    rng = np.random.default_rng(104729 * int(seed) + 11)
    ids = np.cumsum(rng.integers(1, 5, size=k))                      # k different ids with gaps
    return rng.permutation(ids)[inverse].astype(np.int64)


def scan_faces(xyz, seg_label, group_label, cell, seed, bridges=0):
    """A synthetic mesh over a scan: xyz (v, 3) f32, seg_label, group_label (v,), cell > 0 -> faces (F, 3) int32 in seeded order.
    The vertices of every (seg_label, group_label) instance form ONE connected piece and no edge joins two instances: an instance's
    vertices are ordered by their cube of side `cell` (scan_segments' cubes) and in seeded order inside a cube, a triangle strip runs
    over that order (an instance of two vertices gets one degenerate face, of one vertex none), and half as many seeded triangles again
    join vertices at most 8 places apart in it.  bridges: that many more faces (a, b, b), each ONE edge between two instances, all
    different -- real meshes join a chair to its floor; needs two instances."""
    xyz = np.asarray(xyz, np.float32)
    v = xyz.shape[0]
    if xyz.shape != (v, 3) or len(seg_label) != v or len(group_label) != v or not cell > 0 or bridges < 0:
        raise ValueError("scan_faces: xyz (v, 3) with v labels of each kind, cell > 0 and bridges >= 0 expected, got %s, %d, %d, cell = %r, "
                         "bridges = %r" % (xyz.shape, len(seg_label), len(group_label), cell, bridges))
    rng = np.random.default_rng(15485863 * int(seed) + 17)
    cubes = np.floor(xyz.astype(np.float64) / float(cell)).astype(np.int64)
    keys = np.concatenate((np.asarray(seg_label, np.int64).reshape(v, 1), np.asarray(group_label, np.int64).reshape(v, 1)), axis=1)
    _, inst = np.unique(keys, axis=0, return_inverse=True)
    inst = inst.reshape(-1)
    order = np.lexsort((rng.random(v), cubes[:, 2], cubes[:, 1], cubes[:, 0], inst))       # by instance, then cube, then seeded
    at = inst[order]
    pos = np.arange(v)
    first = np.concatenate(([True], at[1:] != at[:-1])) if v else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, pos, 0)) if v else pos                   # where each vertex's instance starts in `order`
    count = np.bincount(at, minlength=1)[at] if v else pos
    stop = start + count                                                                    # and where it stops
    strip = pos[pos + 2 < stop]
    faces = [np.stack((order[strip], order[strip + 1], order[strip + 2]), axis=1)]
    pair = pos[first & (count == 2)]
    faces.append(np.stack((order[pair], order[pair + 1], order[pair + 1]), axis=1) if pair.size else np.zeros((0, 3), np.int64))
    extra = rng.permutation(v)[:v // 2]
    j, k = rng.integers(1, 9, size=extra.size), rng.integers(1, 9, size=extra.size)
    inside = (extra + j + k < stop[extra]) if extra.size else np.zeros(0, bool)
    extra, j, k = extra[inside], j[inside], k[inside]
    faces.append(np.stack((order[extra], order[extra + j], order[extra + j + k]), axis=1) if extra.size else np.zeros((0, 3), np.int64))
    if bridges:
        if v == 0 or at[-1] == at[0]:
            raise ValueError("scan_faces: bridges need two instances")
        seen, rows = set(), []
        while len(rows) < bridges:
            a, b = (int(x) for x in rng.integers(0, v, size=2))
            if inst[a] != inst[b] and (min(a, b), max(a, b)) not in seen:
                seen.add((min(a, b), max(a, b)))
                rows.append((a, b, b))
        faces.append(np.array(rows, np.int64))
    faces = np.concatenate(faces)
    return np.ascontiguousarray(faces[rng.permutation(faces.shape[0])].astype(np.int32))


def batch(kind, b, n, seed0=0):
    f = {"U": cloud_u, "D": cloud_d, "S": cloud_s}[kind]
    return np.stack([f(n, seed0 + i) for i in range(b)]).astype(np.float32)


def spn_batch(kind, b, n, ngroup, nsmp_ins, ncat, seed0=0, invalid=(), stray=0.0):
    """Inputs of rpointnet() (models/model_rpointnet.py:1051) on synthetic clouds: a dict of
      pc, color (b,n,3) f32; group_label (b,n) i64 -- the nearest of one seeded centre per group not listed in `invalid`, a fraction
      `stray` of the points labelled with an invalid group instead (the reference allows it: such a seed gets a zero instance feature);
      group_indicator (b,ngroup) f32 (0 for the invalid groups); seg_label (b,n) i64 -- one category in [0, ncat) per group, about a quarter
      of the groups background (0); pc_ins (b,ngroup,nsmp_ins,3) f32 -- nsmp_ins points of each valid group drawn with replacement, zeros
      for the others; bbox_ins (b,ngroup,6) f32 -- (centre, size) of pc_ins, zeros for the others; smpw (b,n) f32 with about 30 % zeros."""
    out = {k: [] for k in ("pc", "color", "group_label", "group_indicator", "seg_label", "pc_ins", "bbox_ins", "smpw")}
    f = {"U": cloud_u, "D": cloud_d, "S": cloud_s}[kind]
    valid = np.array([g for g in range(ngroup) if g not in set(invalid)])
    bad = np.array(sorted(set(invalid)), dtype=np.int64)
    for i in range(b):
        rng = np.random.default_rng(1000003 * (seed0 + i) + 17)
        pc = f(n, seed0 + i)
        centres = pc[rng.choice(n, size=min(len(valid), n), replace=False)]
        label = valid[((pc[:, None, :] - centres[None, :, :]) ** 2).sum(-1).argmin(1)]
        if len(bad) and stray > 0:
            s = rng.random(n) < stray
            label[s] = bad[rng.integers(0, len(bad), size=int(s.sum()))]
        cat = rng.integers(1, ncat, size=ngroup) * (rng.random(ngroup) >= 0.25)
        ins = np.zeros((ngroup, nsmp_ins, 3), np.float32)
        box = np.zeros((ngroup, 6), np.float32)
        for g in valid:
            members = np.nonzero(label == g)[0]
            if len(members) == 0:
                members = np.array([0])
            ins[g] = pc[members[rng.integers(0, len(members), size=nsmp_ins)]]
            hi, lo = ins[g].max(0), ins[g].min(0)
            box[g] = np.concatenate([(hi + lo) / 2, hi - lo])
        ind = np.ones(ngroup, np.float32)
        ind[bad] = 0.0
        out["pc"].append(pc)
        out["color"].append(rng.random((n, 3), dtype=np.float32))
        out["group_label"].append(label.astype(np.int64))
        out["group_indicator"].append(ind)
        out["seg_label"].append(cat[label].astype(np.int64))
        out["pc_ins"].append(ins)
        out["bbox_ins"].append(box)
        out["smpw"].append((rng.random(n, dtype=np.float32) * (rng.random(n) >= 0.3)).astype(np.float32))
    return {k: np.stack(v) for k, v in out.items()}
