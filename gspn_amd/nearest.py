"""nearest_point: the nearest known point of every query, exact, over a cell grid that gspn_nearest_point (csrc/nearest.hip)
builds once per call in a workspace in global memory.  The result is the first column of three_nn on the same inputs, bit for bit: the
unfused fp32 (dx*dx + dy*dy) + dz*dz, the lowest index among equal distances, (+inf, 0) for a query that nothing finite is near.  Made for
a scan's vertices against a scene's points (lift.vertex_tables): known sets beyond three_nn's 8192-point LDS grid, up to 2^24 points.
Non-differentiable.  No CPU fallback."""
import torch

from . import _lib as L
from ._args import _on_device, _typed, _workspace, _ws_typed

__all__ = ["NEAREST_MAX_M", "nearest_point"]

NEAREST_MAX_M = 1 << 24       # GSPN_NEAREST_MAX_M of include/gspn_hip.h


def nearest_point(xyz1, xyz2, ws=None):
    """xyz1 (b, n, 3) float32: the queries; xyz2 (b, m, 3) float32: the known points of each scene; ws: a uint8 device tensor of at least
    gspn_nearest_point_ws_bytes(b, m) bytes to build the grid in (it need not be initialised; a caller that owns it can capture the call
    in a graph), or None -> dist (b, n) float32: the squared distance to the nearest known point, idx (b, n) int32: its index, the lowest
    among equal distances; (+inf, 0) where no distance is finite.  Raises ValueError on shapes or dtypes that do not fit or m == 0,
    NotImplementedError for m > 2^24, both before anything has run."""
    xyz1 = _typed(xyz1, torch.float32, 3, "xyz1")
    xyz2 = _typed(xyz2, torch.float32, 3, "xyz2")
    if xyz1.shape[2] != 3 or xyz2.shape[2] != 3 or xyz1.shape[0] != xyz2.shape[0]:
        raise ValueError("nearest_point: expected xyz1 (b, n, 3) and xyz2 (b, m, 3), got %s and %s" % (tuple(xyz1.shape), tuple(xyz2.shape)))
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if m <= 0:
        raise ValueError("nearest_point: no known points, xyz2 %s" % (tuple(xyz2.shape),))
    if m > NEAREST_MAX_M:
        raise NotImplementedError("nearest_point: m <= %d (got %d)" % (NEAREST_MAX_M, m))
    ws = _ws_typed(ws)
    xyz1, xyz2 = _on_device(xyz1=xyz1, xyz2=xyz2)
    dev = xyz1.device
    dist = torch.empty((b, n), dtype=torch.float32, device=dev)
    idx = torch.empty((b, n), dtype=torch.int32, device=dev)
    if b == 0 or n == 0:
        return dist, idx
    ws = _workspace(ws, int(L.lib().gspn_nearest_point_ws_bytes(b, m)), dev, "nearest_point")
    with torch.cuda.device(dev):
        L.check(L.lib().gspn_nearest_point(b, n, m, L.ptr(xyz1), L.ptr(xyz2), L.ptr(ws), L.ptr(dist), L.ptr(idx), L.stream()), "nearest_point")
    return dist, idx
