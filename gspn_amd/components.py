"""Mask components (ours: the reference stops at the network's points): the connected components of every mask row on the
scan's mesh, and the rows with their small components dropped.  A scan is R mask rows of V bytes, any nonzero byte set, and F triangles
faces (F, 3) int32.  The edges of a face (a, b, c) are {a,b}, {b,c}, {a,c}; an edge with an end outside [0, V) is ignored.  The components
of row k are those of its set vertices under the edges whose two ends are both set in row k: two set regions that touch only through an
unset vertex are separate, and rows are independent.  comp[k][x] is the smallest vertex of x's component, -1 where x is not set.  A
component of s vertices is kept iff s >= min_vertices and float64(s) >= min_share * float64(largest component of the row): one double
multiply and a non-strict compare.  gspn_mask_components / gspn_mask_component_filter (csrc/components.hip): a lock-free union-find over
a vertex-major bit table, integer atomics only, the same bits on every call.  No CPU fallback."""
import numpy as np
import torch

from . import _lib as L
from ._args import _on_device, _out_like, _parameters, _typed, _workspace, _ws_typed

__all__ = ["COMPONENTS_MAX_R", "COMPONENTS_MAX_V", "COMPONENTS_MAX_F", "mesh_faces", "mask_components", "component_filter"]

COMPONENTS_MAX_R = 1024             # GSPN_MASK_COMPONENTS_MAX_R of include/gspn_hip.h: scene_rank's limit
COMPONENTS_MAX_V = 1 << 24          # GSPN_MASK_COMPONENTS_MAX_V
COMPONENTS_MAX_F = 1 << 26          # GSPN_MASK_COMPONENTS_MAX_F


def mesh_faces(faces, v):
    """faces: an integer tensor or array (F, 3), F >= 0; v: the scan's vertex count -> a contiguous (F, 3) int32 tensor on the device (a
    tensor that is one already comes back as it is).  Raises ValueError for another shape, a dtype that is not an integer's, or a negative
    index; an index >= v is allowed and ignored by the ops, as the rule says.  One read-back (the sign check): once per scan."""
    v = int(v)
    if v < 0:
        raise ValueError("mesh_faces: v must not be negative, got %d" % v)
    if isinstance(faces, np.ndarray):
        if faces.dtype.kind not in "iu":
            raise ValueError("mesh_faces: faces must hold integers, got %s" % faces.dtype)
        faces = torch.from_numpy(np.ascontiguousarray(faces.astype(np.int64, copy=False)))
    if not isinstance(faces, torch.Tensor):
        raise TypeError("faces must be a torch.Tensor or a numpy array")
    if faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise ValueError("mesh_faces: faces must hold integers, got %s" % faces.dtype)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("mesh_faces: faces must be (F, 3), got %s" % (tuple(faces.shape),))
    if faces.numel() and (int(faces.min()) < 0 or int(faces.max()) >= 1 << 31):
        raise ValueError("mesh_faces: a vertex index is negative or beyond int32")
    if not faces.is_cuda:
        if not torch.cuda.is_available():
            raise L.GspnHipError("faces is on %s: gspn_amd runs on ROCm devices only (no CPU fallback)" % faces.device)
        faces = faces.cuda()
    return faces.int().contiguous()


def _checked(masks, faces, ws, what):
    """the shape and dtype checks and the limits the two ops share -> masks, faces, ws, r, v, f: nothing has touched the library"""
    masks = _typed(masks, torch.uint8, 2, "masks")
    faces = _typed(faces, torch.int32, 2, "faces")
    r, v = masks.shape
    if faces.shape[1] != 3:
        raise ValueError("%s: expected masks (R, V) and faces (F, 3), got %s and %s" % (what, tuple(masks.shape), tuple(faces.shape)))
    if min(r, v) <= 0:
        raise ValueError("%s: empty input, masks %s" % (what, tuple(masks.shape)))
    return masks, faces, _ws_typed(ws), r, v, faces.shape[0]


def _limits(r, v, f, what):
    if r > COMPONENTS_MAX_R or v > COMPONENTS_MAX_V or f > COMPONENTS_MAX_F:
        raise NotImplementedError("%s: R <= %d, V <= %d and F <= %d (got %d, %d and %d)"
                                  % (what, COMPONENTS_MAX_R, COMPONENTS_MAX_V, COMPONENTS_MAX_F, r, v, f))


def mask_components(masks, faces, ws=None):
    """masks (R, V) uint8, any nonzero byte set; faces (F, 3) int32 (mesh_faces), F may be 0: every set vertex is then its own component;
    ws: a 16-byte aligned uint8 device tensor of at least gspn_mask_components_ws_bytes(R, V, F) bytes (it need not be initialised; a
    caller that owns it can capture the call in a graph), or None
    -> comp (R, V) int32: the smallest vertex of the vertex's component in its row, -1 where the vertex is not set; ncomp (R,) int32: the
    components of each row; largest (R,) int32: the vertex count of the largest, 0 for an empty row.  ncomp is never negative (-1 would
    mark a row in which a bounded loop of the kernels ran out, which a correct build cannot do).  Raises ValueError for shapes, dtypes, an
    empty input or a short or misplaced ws, NotImplementedError for R > 1024, V > 2^24 or F > 2^26, all before anything has run."""
    masks, faces, ws, r, v, f = _checked(masks, faces, ws, "mask_components")
    _limits(r, v, f, "mask_components")
    masks, faces = _on_device(masks=masks, faces=faces)
    dev = masks.device
    ws = _workspace(ws, int(L.lib().gspn_mask_components_ws_bytes(r, v, f)), dev, "mask_components")
    comp = torch.empty((r, v), dtype=torch.int32, device=dev)
    ncomp = torch.empty((r,), dtype=torch.int32, device=dev)
    largest = torch.empty((r,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_mask_components(r, v, f, L.ptr(masks), L.ptr(faces) if f else L.ptr(None), L.ptr(ws), L.ptr(comp), L.ptr(ncomp),
                                             L.ptr(largest), L.stream()), "mask_components")
    return comp, ncomp, largest


def component_filter(masks, faces, *, min_vertices, min_share=0.0, out=None, ws=None):
    """masks and faces as in mask_components; min_vertices: an int >= 1, no default; min_share: a Python float (a double) in [0, 1]; out:
    a (R, V) uint8 device tensor to write, masks itself allowed, or None; ws: at least gspn_mask_component_filter_ws_bytes(R, V, F)
    bytes, or None
    -> out (R, V) uint8 of 0 and 1: the vertices whose component is kept; mask_points (R,) int32: the set bytes of each row of out;
       ncomp, nkept (R,) int32: the components of each row, and those kept.
    min_share = 1 keeps the largest component(s) alone, ties included; min_vertices = 1 with min_share = 0 is the identity up to the
    normalisation of a nonzero byte to 1.  Raises as mask_components does, and ValueError for a parameter outside its range."""
    masks, faces, ws, r, v, f = _checked(masks, faces, ws, "component_filter")
    min_vertices, min_share = _parameters(min_vertices, min_share, "component_filter")
    out = _out_like(out, (r, v), None, "component_filter")
    _limits(r, v, f, "component_filter")
    masks, faces = _on_device(masks=masks, faces=faces)
    dev = masks.device
    out = _out_like(out, (r, v), dev, "component_filter")
    ws = _workspace(ws, int(L.lib().gspn_mask_component_filter_ws_bytes(r, v, f)), dev, "component_filter")
    mask_points = torch.empty((r,), dtype=torch.int32, device=dev)
    ncomp = torch.empty((r,), dtype=torch.int32, device=dev)
    nkept = torch.empty((r,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_mask_component_filter(r, v, f, L.ptr(masks), L.ptr(faces) if f else L.ptr(None), min_vertices, min_share,
                                                   L.ptr(ws), L.ptr(out), L.ptr(mask_points), L.ptr(ncomp), L.ptr(nkept), L.stream()),
                "component_filter")
    return out, mask_points, ncomp, nkept
