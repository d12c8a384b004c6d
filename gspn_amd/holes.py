"""Mask holes (ours: the reference stops at the network's points): the gaps a mask row encloses on the scan's mesh are
filled.  The mirror of components.component_filter.  A scan is R mask rows of V bytes, any nonzero byte set, F triangles faces (F, 3) int32
with the edges and the range rule of components, and the vertices xyz (V, 3) float32.  For row k the box is the closed axis-aligned box
over its set vertices whose three coordinates are finite; a candidate is an unset vertex inside it (float compares: -0.0 is +0.0, a NaN
is never inside); the candidate components are those of the candidates under the edges whose two ends are both candidates.  A candidate
component is open iff an edge joins it to an unset vertex outside the box, and touches iff an edge joins it to a set vertex; one of s
vertices is a hole iff it is not open, it touches, s <= max_vertices and float64(s) <= max_share * float64(set vertices of the row).  The
floor beyond the object is open and a floating fragment inside the box touches nothing: neither is filled.  gspn_mask_hole_fill
(csrc/components.hip): the union-find of the components over the candidates and one more pass over the faces, integer atomics only, the
same bits on every call.  No CPU fallback."""
import torch

from . import _lib as L
from ._args import _hole_parameters, _on_device, _out_like, _typed, _workspace, _ws_typed

__all__ = ["HOLE_FILL_MAX_R", "HOLE_FILL_MAX_V", "HOLE_FILL_MAX_F", "hole_fill"]

HOLE_FILL_MAX_R = 1024              # GSPN_MASK_HOLE_FILL_MAX_R of include/gspn_hip.h
HOLE_FILL_MAX_V = 1 << 24           # GSPN_MASK_HOLE_FILL_MAX_V
HOLE_FILL_MAX_F = 1 << 26           # GSPN_MASK_HOLE_FILL_MAX_F


def hole_fill(masks, faces, xyz, *, max_vertices, max_share=1.0, out=None, ws=None, label=False):
    """masks (R, V) uint8, any nonzero byte set; faces (F, 3) int32 (components.mesh_faces), F may be 0: then there are no holes; xyz
    (V, 3) float32, contiguous, on the masks' device; max_vertices: an int >= 0, no default; max_share: a Python float (a double) in
    [0, 1]; out: a (R, V) uint8 device tensor to write, masks itself allowed, or None; ws: a 16-byte aligned uint8 device tensor of at
    least gspn_mask_hole_fill_ws_bytes(R, V, F) bytes (it need not be initialised; a caller that owns it can capture the call in a graph),
    or None; label: also return the labels
    -> out (R, V) uint8 of 0 and 1: the set vertices and those of the holes; mask_points (R,) int32: the set bytes of each row of out;
       nholes, nfilled (R,) int32: the holes filled in each row, and their vertices; with label=True also label (R, V) int32: -2 where the
       vertex is set, -1 where it is unset and no candidate, else the smallest vertex of its candidate component.
    nholes is never negative (-1 would mark a row in which a bounded loop of the kernels ran out, which a correct build cannot do).
    max_vertices = 0 is the identity up to the normalisation of a nonzero byte to 1.  Raises ValueError for shapes, dtypes, an empty
    input, a parameter outside its range or a short or misplaced ws or out, NotImplementedError for R > 1024, V > 2^24 or F > 2^26, all
    before anything has run."""
    masks = _typed(masks, torch.uint8, 2, "masks")
    faces = _typed(faces, torch.int32, 2, "faces")
    xyz = _typed(xyz, torch.float32, 2, "xyz")
    r, v = masks.shape
    if faces.shape[1] != 3 or tuple(xyz.shape) != (v, 3):
        raise ValueError("hole_fill: expected masks (R, V), faces (F, 3) and xyz (V, 3), got %s, %s and %s"
                         % (tuple(masks.shape), tuple(faces.shape), tuple(xyz.shape)))
    if min(r, v) <= 0:
        raise ValueError("hole_fill: empty input, masks %s" % (tuple(masks.shape),))
    ws, f = _ws_typed(ws), faces.shape[0]
    max_vertices, max_share = _hole_parameters(max_vertices, max_share, "hole_fill")
    out = _out_like(out, (r, v), None, "hole_fill")
    if r > HOLE_FILL_MAX_R or v > HOLE_FILL_MAX_V or f > HOLE_FILL_MAX_F:
        raise NotImplementedError("hole_fill: R <= %d, V <= %d and F <= %d (got %d, %d and %d)"
                                  % (HOLE_FILL_MAX_R, HOLE_FILL_MAX_V, HOLE_FILL_MAX_F, r, v, f))
    masks, faces, xyz = _on_device(masks=masks, faces=faces, xyz=xyz)
    dev = masks.device
    if faces.device != dev or xyz.device != dev:
        raise ValueError("hole_fill: faces and xyz must be on the masks' device %s" % dev)
    out = _out_like(out, (r, v), dev, "hole_fill")
    ws = _workspace(ws, int(L.lib().gspn_mask_hole_fill_ws_bytes(r, v, f)), dev, "hole_fill")
    mask_points = torch.empty((r,), dtype=torch.int32, device=dev)
    nholes = torch.empty((r,), dtype=torch.int32, device=dev)
    nfilled = torch.empty((r,), dtype=torch.int32, device=dev)
    labels = torch.empty((r, v), dtype=torch.int32, device=dev) if label else None
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_mask_hole_fill(r, v, f, L.ptr(masks), L.ptr(faces) if f else L.ptr(None), L.ptr(xyz), max_vertices, max_share,
                                            L.ptr(ws), L.ptr(out), L.ptr(mask_points), L.ptr(nholes), L.ptr(nfilled), L.ptr(labels),
                                            L.stream()), "hole_fill")
    return (out, mask_points, nholes, nfilled, labels) if label else (out, mask_points, nholes, nfilled)
