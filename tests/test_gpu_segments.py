"""GPU tests of gspn_amd.segments (csrc/segments.hip) against the numpy restatement in tests/segments_ref.py.  Every
comparison is for equal bits: the counts are integers and the threshold is one double multiply.  Sizes at the edges of the 16-byte vector,
the 256-lane workgroup, the 1024-vertex apply tile and the 8-row apply group; ties; ids out of range; in place; the workspace contract;
capture; rows beyond 2^31 bytes; the label vote; the declines; and a constructed case in which the vote provably restores the ground truth."""
import ctypes

import numpy as np
import pytest
import torch

from tests import segments_ref as ref

pytestmark = pytest.mark.gpu

V_EDGES = (1, 15, 16, 17, 255, 256, 257, 1023, 1025, 4099)
BYTES = np.array([0, 1, 2, 255], np.uint8)
OUTSIDE = lambda s: np.array([-1, -5, s, s + 1, 2 ** 31 - 1], np.int64)        # noqa: E731


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


def make_masks(rng, r, v, density=0.4):
    m = BYTES[rng.integers(1, 4, size=(r, v))] * (rng.random((r, v)) < density).astype(np.uint8)
    if r >= 3:
        m[0] = 0                                                      # a row that is all zero
        m[1] = BYTES[rng.integers(1, 4, size=v)]                      # and one that is all set
    return m


def vote(masks, seg, s, th=0.5, **kw):
    from gspn_amd.segments import segment_vote
    out, points = segment_vote(dev(masks), dev(seg, np.int32), s, th, **kw)
    assert out.dtype == torch.uint8 and points.dtype == torch.int32
    return out.cpu().numpy(), points.cpu().numpy()


def same(got, want, what):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), "%s: %d mask bytes differ" % (what, int((got[0] != want[0]).sum()))
    assert np.array_equal(got[1], want[1]), "%s: mask_points %s, expected %s" % (what, got[1], want[1])


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", V_EDGES)
def test_the_vote_equals_the_restatement_at_the_tile_and_vector_edges(v):
    rng = np.random.default_rng(1000 + v)
    for r in (1, 3, 100):
        masks = make_masks(rng, r, v)
        for s in (1, 2, 7, v):
            seg = rng.integers(0, s, size=v)
            want = ref.fast_segment_vote_ref(masks, seg, s)
            same(vote(masks, seg, s), want, "V %d R %d S %d" % (v, r, s))
            if r >= 3:
                assert not want[0][0].any() and want[1][0] == 0       # an all-zero row stays all zero
                assert want[0][1].all() and want[1][1] == v           # an all-set row stays all set


def test_singleton_segments_are_the_identity_on_the_normalised_masks():
    v = 70001
    rng = np.random.default_rng(2)
    masks = make_masks(rng, 3, v, 0.3)
    seg = rng.permutation(v)
    got = vote(masks, seg, v)
    assert np.array_equal(got[0], (masks != 0).astype(np.uint8)) and np.array_equal(got[1], (masks != 0).sum(1))
    none = vote(masks, np.full(v, -1), 0)                             # no segmented vertex at all
    assert np.array_equal(none[0], got[0]) and np.array_equal(none[1], got[1])


def test_five_segments_under_heavy_contention():
    v = 70001
    rng = np.random.default_rng(3)
    masks = make_masks(rng, 4, v, 0.5)
    masks[3] = masks[3] * (rng.random(v) < 0.9)
    seg = rng.integers(0, 5, size=v)
    same(vote(masks, seg, 5), ref.fast_segment_vote_ref(masks, seg, 5), "V 70001 S 5")


# ---- ties ----------------------------------------------------------------------------------------------------------------------------------
def test_ties_on_segments_exactly_half_set():
    sizes = [2, 4, 6, 10, 64, 130, 1000]
    seg = np.concatenate([np.full(n, g) for g, n in enumerate(sizes)])
    masks = np.concatenate([np.r_[np.full(n // 2, 255), np.zeros(n // 2)] for n in sizes]).astype(np.uint8)[None]
    order = np.random.default_rng(5).permutation(seg.size)
    seg, masks = seg[order], np.ascontiguousarray(masks[:, order])
    expect = {0.5: 0, 0.0: 1, 0.3: 1, 1.0 / 3.0: 1, 0.999: 0}          # exactly half set is not set at 0.5; at 0 any vote sets
    for th, bit in expect.items():
        got = vote(masks, seg, len(sizes), th)
        same(got, ref.segment_vote_ref(masks, seg, len(sizes), th), "half set at %r" % th)
        assert (got[0] == bit).all() and got[1][0] == bit * seg.size


def test_ties_at_a_quarter():
    sizes = [4, 8, 12]
    seg = np.concatenate([np.full(n, g) for g, n in enumerate(sizes)])
    masks = np.concatenate([np.r_[np.full(n // 4, 1), np.zeros(n - n // 4)] for n in sizes]).astype(np.uint8)[None]
    got = vote(masks, seg, 3, 0.25)
    same(got, ref.segment_vote_ref(masks, seg, 3, 0.25), "a quarter set at 0.25")
    assert not got[0].any()                                           # 1 > 0.25 * 4 is false: a strict compare
    masks[0, [3, 11, 23]] = 7                                         # one more vote in every segment: now strictly above a quarter
    got = vote(masks, seg, 3, 0.25)
    same(got, ref.segment_vote_ref(masks, seg, 3, 0.25), "one above a quarter")
    assert got[0].all()


# ---- ids out of range ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v,s", ((257, 7), (4099, 100)))
def test_ids_out_of_range_keep_their_normalised_byte(v, s):
    rng = np.random.default_rng(6)
    masks = make_masks(rng, 3, v)
    seg = rng.integers(0, s, size=v).astype(np.int64)
    odd = rng.random(v) < 0.2
    seg[odd] = OUTSIDE(s)[rng.integers(0, 5, size=int(odd.sum()))]
    got = vote(masks, seg, s)
    same(got, ref.segment_vote_ref(masks, seg, s), "V %d S %d with ids out of range" % (v, s))
    assert np.array_equal(got[0][:, odd], (masks[:, odd] != 0).astype(np.uint8))
    inside = ~odd                                                     # and they did not vote: the others alone give the same bits
    alone = vote(np.ascontiguousarray(masks[:, inside]), seg[inside], s)
    assert np.array_equal(got[0][:, inside], alone[0])


# ---- in place, workspace, capture ----------------------------------------------------------------------------------------------------------
def case(v=4099, r=11, s=37, seed=7):
    rng = np.random.default_rng(seed)
    masks = make_masks(rng, r, v)
    seg = rng.integers(-2, s + 2, size=v)
    return masks, seg, s


def test_out_may_be_masks():
    from gspn_amd.segments import segment_vote
    masks, seg, s = case()
    m, g = dev(masks), dev(seg, np.int32)
    want = segment_vote(m, g, s)
    out, points = segment_vote(m, g, s, out=m)
    assert out.data_ptr() == m.data_ptr() and torch.equal(out, want[0]) and torch.equal(points, want[1])
    same((out.cpu().numpy(), points.cpu().numpy()), ref.segment_vote_ref(masks, seg, s), "in place")
    other = torch.full_like(m, 9)
    out, points = segment_vote(dev(masks), g, s, out=other)
    assert out.data_ptr() == other.data_ptr() and torch.equal(other, want[0]) and torch.equal(points, want[1])


def test_the_workspace_need_not_be_initialised_and_must_be_large_enough():
    from gspn_amd import _lib
    from gspn_amd.segments import segment_label_vote, segment_vote
    masks, seg, s = case()
    r, v = masks.shape
    m, g = dev(masks), dev(seg, np.int32)
    want = segment_vote(m, g, s)
    need = int(_lib.lib().gspn_segment_vote_ws_bytes(r, v, s))
    assert need >= 4 * (r + 1) * s + 8 * r * ((s + 63) // 64)
    for fill in (0xFF, 0x00):
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        for _ in range(2):                                            # and what the first call left changes nothing for the second
            got = segment_vote(m, g, s, ws=ws)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError, match="ws must be"):
        segment_vote(m, g, s, ws=torch.empty((need - 1,), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="ws must be"):
        segment_vote(m, g, s, ws=torch.empty((need + 16,), dtype=torch.uint8, device="cuda")[1:])      # not 16-byte aligned
    with pytest.raises(ValueError, match="ws must be"):
        segment_vote(m, g, s, ws=torch.empty((need,), dtype=torch.uint8))                               # not on the device
    labels = dev(np.random.default_rng(8).integers(-1, 20, size=v), np.int32)
    want_l = segment_label_vote(labels, g, s, 19)
    need_l = int(_lib.lib().gspn_segment_label_vote_ws_bytes(v, s, 19))
    assert need_l >= 4 * s * 19 + 4 * s
    for fill in (0xFF, 0x00):
        ws = torch.full((need_l,), fill, dtype=torch.uint8, device="cuda")
        for _ in range(2):
            assert torch.equal(segment_label_vote(labels, g, s, 19, ws=ws), want_l)
    with pytest.raises(ValueError, match="ws must be"):
        segment_label_vote(labels, g, s, 19, ws=torch.empty((need_l - 1,), dtype=torch.uint8, device="cuda"))


def test_the_calls_capture_with_a_caller_owned_workspace():
    from gspn_amd import _lib
    from gspn_amd.segments import segment_label_vote, segment_vote
    inputs = [case(seed=20 + k) for k in range(3)]
    label_inputs = [np.random.default_rng(30 + k).integers(-1, 20, size=4099) for k in range(3)]
    masks, seg, s = inputs[0]
    r, v = masks.shape
    m, g, lab = dev(masks), dev(seg, np.int32), dev(label_inputs[0], np.int32)
    ws = torch.empty((int(_lib.lib().gspn_segment_vote_ws_bytes(r, v, s)),), dtype=torch.uint8, device="cuda")
    ws_l = torch.empty((int(_lib.lib().gspn_segment_label_vote_ws_bytes(v, s, 19)),), dtype=torch.uint8, device="cuda")
    segment_vote(m, g, s, ws=ws)                                      # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = segment_vote(m, g, s, ws=ws)
        out_l = segment_label_vote(lab, g, s, 19, ws=ws_l)
    for (nm, ns, _), nl in zip(inputs[1:], label_inputs[1:]):
        m.copy_(torch.from_numpy(nm))
        g.copy_(torch.from_numpy(ns.astype(np.int32)))
        lab.copy_(torch.from_numpy(nl.astype(np.int32)))
        graph.replay()
        torch.cuda.synchronize()
        eager = segment_vote(m.clone(), g.clone(), s)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        assert torch.equal(out_l, segment_label_vote(lab.clone(), g.clone(), s, 19))
        same((out[0].cpu().numpy(), out[1].cpu().numpy()), ref.fast_segment_vote_ref(nm, ns, s), "replay")


# ---- rows beyond 2^31 bytes ----------------------------------------------------------------------------------------------------------------
def test_row_offsets_are_64_bit():
    from gspn_amd.segments import segment_vote
    r, v, s = 1024, (1 << 21) + 3, 32768                              # 2 GiB of masks that never reach the host
    gen = torch.Generator(device="cuda").manual_seed(9)
    seg = torch.randint(-3, s + 3, (v,), generator=gen, device="cuda", dtype=torch.int32)
    inside = (seg >= 0) & (seg < s)
    ids = seg.long().clamp(0, s - 1)
    size = torch.bincount(ids[inside], minlength=s).double()
    masks = torch.zeros((r, v), dtype=torch.uint8, device="cuda")
    rows, expected = (0, 511, 1023), {}
    for k in rows:
        own = torch.rand((v,), generator=gen, device="cuda") < 0.5
        # segments below s / 2 are pushed clearly to one side, so that both outcomes are well represented
        own = torch.where(inside & (ids < s // 4), torch.ones_like(own), own)
        own = torch.where(inside & (ids >= s // 4) & (ids < s // 2), torch.zeros_like(own), own)
        masks[k] = own.to(torch.uint8) * 255
        cnt = torch.bincount(ids[inside & own], minlength=s).double()
        bit = cnt > 0.5 * size
        expected[k] = torch.where(inside, bit[ids], own).to(torch.uint8)
    out, points = segment_vote(masks, seg, s, out=masks)
    assert out.data_ptr() == masks.data_ptr()
    for k in rows:
        assert torch.equal(out[k], expected[k]) and int(points[k]) == int(expected[k].sum())
        assert 0 < int(points[k]) < v
    for lo, hi in ((1, 511), (512, 1023)):
        assert not bool(out[lo:hi].any()) and not bool(points[lo:hi].any())


# ---- the label vote ------------------------------------------------------------------------------------------------------------------------
def label_vote(labels, seg, s, c, **kw):
    from gspn_amd.segments import segment_label_vote
    out = segment_label_vote(dev(labels, np.int32), dev(seg, np.int32), s, c, **kw)
    assert out.dtype == torch.int32
    return out.cpu().numpy()


@pytest.mark.parametrize("v", V_EDGES)
def test_the_label_vote_equals_the_restatement(v):
    rng = np.random.default_rng(3000 + v)
    for c in (1, 2, 19, 64):
        for s in (1, 2, 7, v):
            seg = rng.integers(-1, s + 1, size=v)                     # -1 and S among them
            labels = rng.integers(-1, c + 1, size=v)                  # -1 and C among them: they do not vote
            got = label_vote(labels, seg, s, c)
            assert np.array_equal(got, ref.segment_label_vote_ref(labels, seg, s, c)), "V %d C %d S %d" % (v, c, s)


def test_label_ties_unvoted_segments_and_labels_out_of_range():
    c = 19
    #          two-way tie: 7, 3    three-way tie: 9, 4, 2       no voter: -1, 19     a clear winner over strays    unsegmented
    seg = np.array([0, 0, 0, 0,      1, 1, 1, 1, 1, 1, 1,         2, 2, 2,             3, 3, 3, 3, 3,                -1, 4, 5, 2 ** 31 - 1])
    labels = np.array([7, 3, 3, 7,   9, 4, 2, 9, 2, 4, -1,        -1, 19, 19,          5, 19, 5, 0, -1,              8, 19, 6, -7])
    want = np.array([3, 3, 3, 3,     2, 2, 2, 2, 2, 2, 2,         -1, 19, 19,          5, 5, 5, 5, 5,                8, 19, 6, -7])
    order = np.random.default_rng(10).permutation(seg.size)
    got = label_vote(labels[order], seg[order], 4, c)
    assert np.array_equal(ref.segment_label_vote_ref(labels[order], seg[order], 4, c), want[order])
    assert np.array_equal(got, want[order])
    big = np.random.default_rng(11)                                   # the same ties at scale: every label equally often in every segment
    s, per = 50, 4
    seg = np.repeat(np.arange(s), c * per)
    labels = np.tile(np.repeat(np.arange(c), per), s)
    order = big.permutation(seg.size)
    assert not label_vote(labels[order], seg[order], s, c).any()      # the lowest label, 0, wins every tie
    lifted = labels.copy()
    lifted[labels == 0] = -1                                          # 0 no longer votes: 1 wins, the -1 vertices take it too
    assert (label_vote(lifted[order], seg[order], s, c) == 1).all()


# ---- declines ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_decline_before_anything_is_launched():
    from gspn_amd import _lib as L
    lib = L.lib()
    r, v, s, c = 3, 100, 7, 19
    masks = torch.zeros((r, v), dtype=torch.uint8, device="cuda")
    seg = torch.zeros((v,), dtype=torch.int32, device="cuda")
    labels = torch.zeros((v,), dtype=torch.int32, device="cuda")
    ws = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((r, v), 9, dtype=torch.uint8, device="cuda")
    points = torch.full((r,), -9, dtype=torch.int32, device="cuda")
    out_l = torch.full((v,), -9, dtype=torch.int32, device="cuda")
    p, null, st = L.ptr, ctypes.c_void_p(0), L.stream()
    off = ctypes.c_void_p(ws.data_ptr() + 8)

    def sv(r=r, v=v, s=s, masks=p(masks), seg=p(seg), th=0.5, ws=p(ws), out=p(out), points=p(points)):
        return lib.gspn_segment_vote(r, v, s, masks, seg, th, ws, out, points, st)

    def sl(v=v, s=s, c=c, labels=p(labels), seg=p(seg), ws=p(ws), out=p(out_l)):
        return lib.gspn_segment_label_vote(v, s, c, labels, seg, ws, out, st)

    ARG, UNS = -1, -2
    for kw in (dict(r=-1), dict(v=-1), dict(s=-1), dict(masks=null), dict(seg=null), dict(ws=null), dict(out=null), dict(points=null),
               dict(th=float("nan")), dict(th=-0.001), dict(th=1.0), dict(th=1.5), dict(th=float("inf"))):
        assert sv(**kw) == ARG, kw
    for kw in (dict(v=(1 << 24) + 1), dict(r=65536), dict(s=(1 << 24) + 1), dict(r=100, s=(1 << 28) // 101 + 1), dict(ws=off)):
        assert sv(**kw) == UNS, kw
    for kw in (dict(v=-1), dict(s=-1), dict(c=0), dict(c=-3), dict(labels=null), dict(seg=null), dict(ws=null), dict(out=null)):
        assert sl(**kw) == ARG, kw
    for kw in (dict(v=(1 << 24) + 1), dict(s=(1 << 24) + 1), dict(s=1 << 20, c=257), dict(ws=off)):
        assert sl(**kw) == UNS, kw
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and bool((points == -9).all()) and bool((out_l == -9).all()) and bool((ws == 0x5A).all())     # nothing ran
    wsb, wlb = lib.gspn_segment_vote_ws_bytes, lib.gspn_segment_label_vote_ws_bytes
    assert wsb(r, v, s) > 0 and wlb(v, s, c) > 0
    for args in ((-1, v, s), (r, -1, s), (r, v, -1), (r, (1 << 24) + 1, s), (65536, v, s), (r, v, (1 << 24) + 1), (100, v, (1 << 28) // 101 + 1)):
        assert wsb(*args) == 0, args
    for args in ((-1, s, c), (v, -1, c), (v, s, 0), ((1 << 24) + 1, s, c), (v, (1 << 24) + 1, c), (v, 1 << 20, 257)):
        assert wlb(*args) == 0, args
    assert wsb(100, v, (1 << 28) // 101) > 0                          # the largest table is legal (not launched here: 1 GiB of counters)
    assert sv(r=0) == 0 and sv(v=0) == 0 and sl(v=0) == 0             # nothing to do is no error


def test_the_wrappers_decline_before_the_library_is_touched():
    from gspn_amd.segments import segment_label_vote, segment_vote
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")              # noqa: E731
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32, device="cuda")                   # noqa: E731
    with pytest.raises(NotImplementedError):
        segment_vote(u8(1, (1 << 24) + 1), i32((1 << 24) + 1), 4)
    with pytest.raises(NotImplementedError):
        segment_vote(u8(65536, 2), i32(2), 4)
    with pytest.raises(NotImplementedError):
        segment_vote(u8(1, 2), i32(2), (1 << 24) + 1)
    with pytest.raises(NotImplementedError):
        segment_vote(u8(100, 2), i32(2), (1 << 28) // 101 + 1)
    with pytest.raises(NotImplementedError):
        segment_label_vote(i32((1 << 24) + 1), i32((1 << 24) + 1), 4, 19)
    with pytest.raises(NotImplementedError):
        segment_label_vote(i32(2), i32(2), (1 << 24) + 1, 19)
    with pytest.raises(NotImplementedError):
        segment_label_vote(i32(2), i32(2), 1 << 20, 257)
    for th in (float("nan"), -0.1, 1.0):
        with pytest.raises(ValueError, match="vote_th"):
            segment_vote(u8(1, 2), i32(2), 4, th)
    with pytest.raises(ValueError, match="num_classes"):
        segment_label_vote(i32(2), i32(2), 4, 0)
    with pytest.raises(ValueError, match="out must be"):
        segment_vote(u8(2, 4), i32(4), 4, out=u8(2, 5))
    with pytest.raises(ValueError, match="out must be"):
        segment_vote(u8(2, 4), i32(4), 4, out=u8(4, 2).t())


# ---- compaction on the device --------------------------------------------------------------------------------------------------------------
def test_compact_segments_on_the_device():
    from gspn_amd.segments import compact_segments
    raw = np.array([40, -7, 40, 3, (1 << 26) - 1, 3, -1, 1000, 0], np.int64)
    seg, s = compact_segments(torch.from_numpy(raw).cuda())
    assert s == 5 and seg.dtype == torch.int32 and seg.is_cuda and seg.tolist() == [2, -1, 2, 1, 4, 1, -1, 3, 0]


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------------
def test_the_vote_restores_a_ground_truth_that_is_a_union_of_segments():
    """6 instances, each a union of synth.scan_segments segments.  The input row of an instance is its ground truth with every fifth vertex
    of each of its segments cleared and every fifth vertex of each segment of the next instance set: at most a fifth of any segment is
    flipped, so at 0.5 the vote is the ground truth byte for byte, and AP goes from below 1 to 1."""
    from gspn_amd import synth
    from gspn_amd.evaluate import MIN_REGION_SIZE, InstanceAP
    from gspn_amd.segments import compact_segments, segment_vote
    rng = np.random.default_rng(12)
    n_ins, per = 6, 700
    centres = np.array([[2.0 * g, 0.0, 0.0] for g in range(n_ins)], np.float32)
    xyz = np.concatenate([centres[g] + rng.random((per, 3), dtype=np.float32) for g in range(n_ins)])
    group = np.repeat(np.arange(n_ins), per).astype(np.int32)
    sem = (group + 1).astype(np.int32)                                 # one class per instance, none of them class 0
    order = rng.permutation(xyz.shape[0])
    xyz, group, sem = xyz[order], group[order], sem[order]
    raw = synth.scan_segments(xyz, sem, group, 0.5, seed=13)
    seg, s = compact_segments(torch.from_numpy(raw).cuda())
    seg_np = seg.cpu().numpy()
    assert s >= 8 * n_ins and np.bincount(group).min() >= MIN_REGION_SIZE
    place = np.zeros(xyz.shape[0], np.int64)                           # the position of every vertex inside its segment
    for g in range(s):
        at = np.nonzero(seg_np == g)[0]
        place[at] = np.arange(at.size)
        assert np.unique(group[at]).size == 1                         # nested: the ground truth is a union of segments
    fifth = place % 5 == 4
    truth = np.stack([(group == g) for g in range(n_ins)]).astype(np.uint8)
    noisy = truth.copy()
    for g in range(n_ins):
        noisy[g][(group == g) & fifth] = 0
        noisy[g][(group == (g + 1) % n_ins) & fifth] = 255
    iou = [(noisy[g].astype(bool) & truth[g].astype(bool)).sum() / (noisy[g].astype(bool) | truth[g].astype(bool)).sum() for g in range(n_ins)]
    assert max(iou) < 0.9 and min(iou) > 0.5                          # the input misses the 0.9 overlap, so its AP is below 1
    voted, points = segment_vote(torch.from_numpy(noisy).cuda(), seg, s)
    assert np.array_equal(voted.cpu().numpy(), truth) and points.tolist() == [per] * n_ins

    def all_ap(masks):
        metric = InstanceAP(n_ins + 1, label_map=None)
        cls = torch.arange(1, n_ins + 1, dtype=torch.int32, device="cuda")[None]
        conf = torch.linspace(0.9, 0.4, n_ins, device="cuda")[None]
        count = torch.tensor([n_ins], dtype=torch.int32, device="cuda")
        metric.add(masks[None], cls, conf, count, torch.from_numpy(sem).cuda()[None], torch.from_numpy(group).cuda()[None], n_ins)
        return metric.compute()["all_ap"]

    before, after = all_ap(torch.from_numpy((noisy != 0).astype(np.uint8)).cuda()), all_ap(voted)
    print("all_ap: %.4f on the input masks, %.4f on the voted ones (IoU of the inputs %.3f to %.3f)" % (before, after, min(iou), max(iou)))
    assert after == 1.0 and before < 1.0
