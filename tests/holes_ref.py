"""The numpy restatement of mask holes, written from the rule and never from the kernels: the box of a row over its set
vertices with finite coordinates, the candidates inside it by float compares, a plain union-find (components_ref.row_components_ref) over
the edges whose two ends are candidates, what each component borders, and the fill rule in float64.  Shared by the CPU tests, which hold
it against a brute-force search, and the GPU tests, which hold the library against it bit for bit."""
import numpy as np

from tests.components_ref import edges_ref, row_components_ref


def row_candidates_ref(row_set, xyz):
    """row_set (V,) bool, xyz (V, 3) float32 -> (V,) bool: the unset vertices inside the closed box of the set vertices whose three
    coordinates are finite; all False when there is no such vertex"""
    xyz = np.asarray(xyz, np.float32)
    boxed = row_set & np.isfinite(xyz).all(axis=1)
    if not boxed.any():
        return np.zeros(row_set.shape[0], bool)
    lo, hi = xyz[boxed].min(axis=0), xyz[boxed].max(axis=0)
    with np.errstate(invalid="ignore"):
        inside = ((lo <= xyz) & (xyz <= hi)).all(axis=1)              # IEEE compares: -0.0 == +0.0, a NaN is never inside
    return inside & ~row_set


def row_holes_ref(row_set, xyz, edges, max_vertices, max_share):
    """-> label (V,) int32, holes: [(root, size)] of the components filled, info: {root: (size, open, touches)} of every candidate component"""
    v = row_set.shape[0]
    cand = row_candidates_ref(row_set, xyz)
    comp = row_components_ref(cand, edges)                            # the smallest vertex of the candidate component, -1 elsewhere
    label = np.where(row_set, -2, comp).astype(np.int32)
    size = np.bincount(comp[comp >= 0], minlength=v)
    is_open, touches = np.zeros(v, bool), np.zeros(v, bool)
    both = np.concatenate((edges, edges[:, ::-1]))
    both = both[both[:, 0] != both[:, 1]]
    u, w = both[:, 0], both[:, 1]
    from_cand = cand[u]
    touches[comp[u[from_cand & row_set[w]]]] = True
    is_open[comp[u[from_cand & ~row_set[w] & ~cand[w]]]] = True
    points_in = int(row_set.sum())
    info, holes = {}, []
    for root in np.flatnonzero(size > 0).tolist():
        s = int(size[root])
        info[root] = (s, bool(is_open[root]), bool(touches[root]))
        if not is_open[root] and touches[root] and s <= int(max_vertices) and np.float64(s) <= np.float64(max_share) * np.float64(points_in):
            holes.append((root, s))
    return label, holes, info


def hole_fill_ref(masks, faces, xyz, max_vertices, max_share=1.0, info=False):
    """masks (R, V) uint8, faces (F, 3), xyz (V, 3) -> out (R, V) uint8, mask_points, nholes, nfilled (R,) int32, label (R, V) int32; with
    info=True also the list of every row's {root: (size, open, touches)}"""
    masks = np.asarray(masks)
    r, v = masks.shape
    edges = edges_ref(faces, v)
    out = np.zeros((r, v), np.uint8)
    label = np.zeros((r, v), np.int32)
    nholes, nfilled, infos = np.zeros(r, np.int32), np.zeros(r, np.int32), []
    for k in range(r):
        row_set = masks[k] != 0
        label[k], holes, row_info = row_holes_ref(row_set, xyz, edges, max_vertices, max_share)
        roots = np.array([root for root, _ in holes], np.int64)
        out[k] = row_set | np.isin(label[k], roots)
        nholes[k], nfilled[k] = len(holes), sum(s for _, s in holes)
        infos.append(row_info)
    points = ((masks != 0).sum(axis=1) + nfilled).astype(np.int32)
    got = (out, points, nholes, nfilled, label)
    return got + (infos,) if info else got
