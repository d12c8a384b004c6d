"""The numpy restatement of mask components, written from the rule and never from the kernels: the edges of the faces, a
plain union-find over the edges of each row whose two ends are set in it, the sizes, and the keep rule in float64.  Shared by the CPU
tests, which hold it against a brute-force search, and the GPU tests, which hold the library against it bit for bit."""
import numpy as np


def edges_ref(faces, v):
    """faces (F, 3) integers -> (E, 2) int64: {a,b}, {b,c}, {a,c} of every face, an edge with an end outside [0, v) left out"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [0, 2]]))
    return e[((e >= 0) & (e < v)).all(axis=1)]


def row_components_ref(row_set, edges):
    """row_set (V,) bool, edges (E, 2) -> comp (V,) int32: the smallest vertex of the vertex's component, -1 where it is not set"""
    v = row_set.shape[0]
    parent = list(range(v))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for u, w in edges[row_set[edges[:, 0]] & row_set[edges[:, 1]]].tolist():
        a, b = find(u), find(w)
        if a != b:
            parent[max(a, b)] = min(a, b)                            # the smaller root stays: a tree's root is its minimum
    comp = np.full(v, -1, np.int32)
    at = np.flatnonzero(row_set)
    comp[at] = [find(x) for x in at.tolist()]
    return comp


def mask_components_ref(masks, faces):
    """masks (R, V) uint8, faces (F, 3) -> comp (R, V) int32, ncomp (R,) int32, largest (R,) int32"""
    masks = np.asarray(masks)
    r, v = masks.shape
    edges = edges_ref(faces, v)
    comp = np.stack([row_components_ref(masks[k] != 0, edges) for k in range(r)]) if r else np.zeros((0, v), np.int32)
    ncomp = np.array([np.unique(c[c >= 0]).size for c in comp], np.int32)
    largest = np.array([np.bincount(c[c >= 0], minlength=1).max() for c in comp], np.int32)
    return comp, ncomp, largest


def component_filter_ref(masks, faces, min_vertices, min_share):
    """-> out (R, V) uint8, mask_points (R,) int32, ncomp (R,) int32, nkept (R,) int32"""
    comp, ncomp, largest = mask_components_ref(masks, faces)
    r, v = comp.shape
    out = np.zeros((r, v), np.uint8)
    nkept = np.zeros(r, np.int32)
    for k in range(r):
        size = np.bincount(comp[k][comp[k] >= 0], minlength=v)
        kept = (size > 0) & (size >= int(min_vertices)) & (size.astype(np.float64) >= np.float64(min_share) * np.float64(largest[k]))
        nkept[k] = kept.sum()
        out[k] = (comp[k] >= 0) & kept[np.maximum(comp[k], 0)]
    return out, out.sum(axis=1).astype(np.int32), ncomp, nkept
