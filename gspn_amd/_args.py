"""The argument rules the stage modules share (predict, evaluate, nearest, lift, segments, mask_nms, components, holes): each checks dtypes, ranks and
shapes first, so that a tensor that does not fit raises ValueError wherever it lives, then the limits (NotImplementedError), and only then
touches the device and the library.  Private to the package."""
import torch

from . import _lib as L


def _typed(t, dtype, ndim, name):
    """the dtype and rank rules of L.need without its device rule: the shape rules are checked between the two, so that a tensor that
    does not fit raises ValueError wherever it lives"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s must be %d-D, got shape %s" % (name, ndim, tuple(t.shape)))
    return t.detach()


def _on_device(**named):
    """L.need's device rule and contiguity, for tensors whose dtype and shape have been checked"""
    return [L.need(t, t.dtype, None, name) for name, t in named.items()]


def _ws_typed(ws):
    """ws=: None, or a 1-D uint8 tensor; where it lives is _workspace's to check"""
    return None if ws is None else _typed(ws, torch.uint8, 1, "ws")


def _workspace(ws, need, dev, what):
    """a new workspace of `need` bytes for None, else ws itself, which must be contiguous, 16-byte aligned, long enough and on dev"""
    if ws is None:
        return torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    if ws.numel() < need or not ws.is_contiguous() or ws.device != dev or ws.data_ptr() % 16:
        raise ValueError("%s: ws must be a contiguous, 16-byte aligned uint8 tensor of at least %d bytes on %s" % (what, need, dev))
    return ws


def _out_like(out, shape, dev, what):
    """The out= rule of the mask stages: a uint8 tensor shaped like masks, contiguous, on the masks' device; it may be masks itself.
    dev None: the half before the device is touched -> out, its dtype and shape checked, or None.  With dev: the half after -> out, which
    must be contiguous and on dev, or a new tensor for None."""
    if dev is None:
        if out is not None:
            out = _typed(out, torch.uint8, len(shape), "out")
            if tuple(out.shape) != tuple(shape):
                raise ValueError("%s: out must be %s like masks, got %s" % (what, tuple(shape), tuple(out.shape)))
        return out
    if out is None:
        return torch.empty(tuple(shape), dtype=torch.uint8, device=dev)
    if not out.is_cuda or out.device != dev or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous tensor on %s" % (what, dev))
    return out


def _parameters(min_vertices, min_share, what):
    """the component filter's parameters (components.component_filter, lift.scan_predictions, tester.Tester) -> (int, float); ValueError
    for min_vertices < 1 or a min_share outside [0, 1]"""
    if isinstance(min_vertices, bool) or int(min_vertices) != min_vertices:
        raise ValueError("%s: min_vertices must be an integer, got %r" % (what, min_vertices))
    min_vertices, min_share = int(min_vertices), float(min_share)
    if min_vertices < 1 or min_vertices >= 1 << 31:
        raise ValueError("%s: min_vertices must be at least 1, got %d" % (what, min_vertices))
    if not 0.0 <= min_share <= 1.0:                                                 # a NaN fails both
        raise ValueError("%s: min_share must lie in [0, 1], got %r" % (what, min_share))
    return min_vertices, min_share


def _hole_parameters(max_vertices, max_share, what):
    """the hole fill's parameters (hole_fill, lift.scan_predictions, tester.Tester) -> (int, float); ValueError for max_vertices < 0 or a
    max_share outside [0, 1]"""
    if isinstance(max_vertices, bool) or int(max_vertices) != max_vertices:
        raise ValueError("%s: max_vertices must be an integer, got %r" % (what, max_vertices))
    max_vertices, max_share = int(max_vertices), float(max_share)
    if max_vertices < 0 or max_vertices >= 1 << 31:
        raise ValueError("%s: max_vertices must not be negative, got %d" % (what, max_vertices))
    if not 0.0 <= max_share <= 1.0:                                                 # a NaN fails both
        raise ValueError("%s: max_share must lie in [0, 1], got %r" % (what, max_share))
    return max_vertices, max_share
