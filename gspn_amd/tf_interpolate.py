"""Drop-in for tf_ops/3d_interpolation/tf_interpolate.py (CPU-only ops in the reference; on-device here)."""
import torch

from . import _lib as L
from . import invlists


def three_nn(xyz1, xyz2, order=None):
    """tf_interpolate.py:8-18 -- xyz1 (b,n,3) unknown, xyz2 (b,m,3) known ->
    dist (b,n,3) SQUARED distances, idx (b,n,3) int32.  Non-differentiable.
    order (extension): (b,n) int32, a permutation of range(n) per scene -- the order in which the unknown points are handed to the
    threads.  The result does not depend on it; a spatially coherent order (farthest_point_sample(..., return_order=True)) lets the
    64 queries of a wave agree on which known points are worth an exact evaluation (171 -> 108 us at 8 x 32768 <- 2048)."""
    xyz1 = L.need(xyz1.detach(), torch.float32, 3, "xyz1")
    xyz2 = L.need(xyz2.detach(), torch.float32, 3, "xyz2")
    if xyz1.shape[2] != 3:
        raise ValueError("ThreeNN expects (b,n,3) xyz1 shape")                              # tf_interpolate.cpp:163
    if xyz2.shape[2] != 3 or xyz2.shape[0] != xyz1.shape[0]:
        raise ValueError("ThreeNN expects (b,m,3) xyz2 shape")                              # tf_interpolate.cpp:168
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    dist = torch.empty((b, n, 3), dtype=torch.float32, device=xyz1.device)
    idx = torch.empty((b, n, 3), dtype=torch.int32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        if order is not None:
            order = L.need(order, torch.int32, 2, "order")
            if tuple(order.shape) != (b, n):
                raise ValueError("three_nn: order must be (b,n)")
            L.check(L.lib().gspn_threenn_ordered(b, n, m, L.ptr(xyz1), L.ptr(xyz2), L.ptr(order), L.ptr(dist), L.ptr(idx), L.stream()), "three_nn")
        else:
            L.check(L.lib().gspn_threenn(b, n, m, L.ptr(xyz1), L.ptr(xyz2), L.ptr(dist), L.ptr(idx), L.stream()), "three_nn")
    return dist, idx


class _ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx, weight):
        b, m, c = points.shape
        n = idx.shape[1]
        out = torch.empty((b, n, c), dtype=torch.float32, device=points.device)
        with torch.cuda.device(points.device):
            L.check(L.lib().gspn_threeinterpolate(b, m, c, n, L.ptr(points), L.ptr(idx), L.ptr(weight), L.ptr(out), L.stream()), "three_interpolate")
        ctx.save_for_backward(idx, weight)
        ctx.idx_obj = idx                    # the caller's tensor OBJECT: with the opt-in cache the inverse lists of the gradient are kept on it (invlists.py)
        ctx.m = m
        return out

    @staticmethod
    def backward(ctx, grad_out):
        # tf_interpolate.py:29-34 -> [three_interpolate_grad(points, idx, weight, grad_out), None, None]
        idx, weight = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        b, n, c = grad_out.shape
        g = torch.empty((b, ctx.m, c), dtype=torch.float32, device=grad_out.device)
        with torch.cuda.device(grad_out.device):
            if invlists.ATOMIC_GRADS or n == 0:
                L.check(L.lib().gspn_threeinterpolate_grad(b, n, c, ctx.m, L.ptr(grad_out), L.ptr(idx), L.ptr(weight), L.ptr(g), L.stream()),
                        "three_interpolate_grad")
            else:
                # a gather through the inverse lists of idx: contributions added in ascending (j, t) -- the order of the reference's own
                # sequential loop (tf_interpolate.cpp:131-153), bit for bit; no atomics, no zero fill
                order, offsets = invlists.cached_inverse_lists(ctx.idx_obj if ctx.idx_obj._version == idx._version else idx, ctx.m)
                L.check(L.lib().gspn_fp_concat_grad_csr(b, n, ctx.m, c, 0, c, L.ptr(grad_out), L.ptr(order), L.ptr(offsets), L.ptr(weight), L.ptr(g),
                                                        None, L.stream()), "three_interpolate_grad(csr)")
        return g, None, None


def three_interpolate(points, idx, weight):
    """tf_interpolate.py:19-28 -- points (b,m,c), idx (b,n,3) int32, weight (b,n,3) -> (b,n,c).
    Gradient flows to `points` only (no gradient to idx/weight, as in the reference)."""
    points = L.need(points, torch.float32, 3, "points")
    idx = L.need(idx, torch.int32, 3, "idx")
    weight = L.need(weight.detach(), torch.float32, 3, "weight")
    b = points.shape[0]
    if idx.shape[0] != b or idx.shape[2] != 3:
        raise ValueError("ThreeInterpolate expects (b,n,3) idx shape")                      # tf_interpolate.cpp:199
    if tuple(weight.shape) != tuple(idx.shape):
        raise ValueError("ThreeInterpolate expects (b,n,3) weight shape")                   # tf_interpolate.cpp:203
    return _ThreeInterpolate.apply(points, idx, weight)


MAX_NESTED_LEVELS = 8          # gspn_threenn_nested keeps one top-3 list per level in registers


def three_nn_nested(xyz1, xyz2, local, order=None):
    """three_nn of the queries xyz1 (b,n,3) against L <= 8 subsets of one known cloud xyz2 (b,m,3), in ONE scan of xyz2 (extension).
    local (L,b,m) int32: the index of known point k inside level l, or -1 where k is not in level l (nested_local_maps builds it from FPS
    indices).  Returns dist (L,b,n,3) squared distances and idx (L,b,n,3) int32 in each level's own indexing -- for every level bit-equal
    to three_nn(xyz1, <xyz2 of that level>), ties and levels of fewer than three points included.  order: as in three_nn."""
    xyz1 = L.need(xyz1.detach(), torch.float32, 3, "xyz1")
    xyz2 = L.need(xyz2.detach(), torch.float32, 3, "xyz2")
    local = L.need(local, torch.int32, 3, "local")
    if xyz1.shape[2] != 3:
        raise ValueError("ThreeNN expects (b,n,3) xyz1 shape")
    if xyz2.shape[2] != 3 or xyz2.shape[0] != xyz1.shape[0]:
        raise ValueError("ThreeNN expects (b,m,3) xyz2 shape")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    nl = local.shape[0]
    if tuple(local.shape[1:]) != (b, m) or nl < 1:
        raise ValueError("three_nn_nested: local must be (L, b, m) with L >= 1")
    if nl > MAX_NESTED_LEVELS:
        raise NotImplementedError("three_nn_nested: at most %d levels" % MAX_NESTED_LEVELS)
    if order is not None:
        order = L.need(order, torch.int32, 2, "order")
        if tuple(order.shape) != (b, n):
            raise ValueError("three_nn_nested: order must be (b,n)")
    dist = torch.empty((nl, b, n, 3), dtype=torch.float32, device=xyz1.device)
    idx = torch.empty((nl, b, n, 3), dtype=torch.int32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        L.check(L.lib().gspn_threenn_nested(b, n, m, nl, L.ptr(xyz1), L.ptr(xyz2), L.ptr(local), L.ptr(order), L.ptr(dist), L.ptr(idx), L.stream()),
                "three_nn_nested")
    return dist, idx


def nested_members(fps_chain):
    """fps_chain: [fps_2 (b,n_2) indexing level 1, fps_3 (b,n_3) indexing level 2, ...] -- the FPS indices of each level into the one before.
    Returns, per level 2.., its points as indices into level 1: [fps_2, fps_2[fps_3], fps_2[fps_3][fps_4], ...] (int64)."""
    out, cur = [], None
    for f in fps_chain:
        f = f.long()
        cur = f if cur is None else torch.gather(cur, 1, f)
        out.append(cur)
    return out


def nested_local_maps(m, fps_chain, prefixes=()):
    """The `local` argument of three_nn_nested for level 1 (m points) and its subsets: level 0 is level 1 itself, then one level per entry of
    fps_chain (at least one; composed by nested_members), then one level per count p in `prefixes` (the first p points of level 1: the FPS
    prefixes).  Returns local (L, b, m) int32 with local[l, s, members_l[s, i]] = i and -1 elsewhere.  Small int tensors: torch index ops
    (no host synchronisation, so it may run inside a captured graph)."""
    fps_chain = list(fps_chain)
    if not fps_chain:
        raise ValueError("nested_local_maps: at least one FPS index tensor")
    b, device = fps_chain[0].shape[0], fps_chain[0].device
    members = [torch.arange(m, device=device).expand(b, m)] + nested_members(fps_chain)
    members += [torch.arange(p, device=device).expand(b, p) for p in prefixes]
    local = torch.full((len(members), b, m), -1, dtype=torch.int32, device=device)
    for l, mem in enumerate(members):
        if mem.shape[1] > m:
            raise ValueError("nested_local_maps: level %d has more points than level 1" % l)
        local[l].scatter_(1, mem, torch.arange(mem.shape[1], dtype=torch.int32, device=device).expand(b, -1).contiguous())
    return local
