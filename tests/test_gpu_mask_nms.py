"""GPU tests of gspn_amd.mask_nms (csrc/mask_nms.hip) against the numpy restatement in tests/mask_nms_ref.py.  Every
comparison is for equal bits: the counts are integers and the threshold is one double multiply.  Sizes at the edges of the 16-byte vector,
the 64-bit word and the 32-row pair tile; the rule's corner cases written out; in place; the workspace contract; capture; rows beyond 2^31
bytes with overlaps known in closed form; the declines; and a constructed case in which the stage provably repairs the AP."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mask_nms_ref as ref

pytestmark = pytest.mark.gpu

V_EDGES = (1, 15, 16, 63, 64, 65, 127, 1000, 1027)
R_EDGES = (1, 2, 31, 32, 33, 100)                                     # the pair tile is 32 rows
BYTES = np.array([0, 1, 2, 255], np.uint8)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


def make_masks(rng, r, v, density=0.4):
    """rows that overlap at every level: each is a random subset of one of three parents, so IoUs spread over (0, 1); set bytes of 1, 2 and
    255; with three rows or more, one empty, one all set and one whose only set byte is the last"""
    parents = rng.random((3, v)) < 0.6
    m = BYTES[rng.integers(1, 4, size=(r, v))] * (parents[rng.integers(0, 3, size=r)] & (rng.random((r, v)) < rng.choice([density, 0.9], size=(r, 1))))
    m = m.astype(np.uint8)
    if r >= 5:
        m[r // 2] = 0
    if r >= 3:
        m[r - 1] = BYTES[rng.integers(1, 4, size=v)]
        m[r - 2] = 0
        m[r - 2, v - 1] = 255
    return m


def overlaps(masks, **kw):
    from gspn_amd.mask_nms import mask_overlaps
    sizes, inter = mask_overlaps(dev(masks), **kw)
    assert sizes.dtype == torch.int32 and inter.dtype == torch.int32
    return sizes.cpu().numpy(), inter.cpu().numpy()


def nms(masks, count=None, labels=None, iou_th=0.5, **kw):
    from gspn_amd.mask_nms import mask_nms
    out, keep, points = mask_nms(dev(masks), None if count is None else dev(count, np.int32), None if labels is None else dev(labels, np.int32),
                                 iou_th=iou_th, **kw)
    assert out.dtype == torch.uint8 and keep.dtype == torch.uint8 and points.dtype == torch.int32
    return out.cpu().numpy(), keep.cpu().numpy(), points.cpu().numpy()


def same(got, want, what):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), "%s: %d mask bytes differ" % (what, int((got[0] != want[0]).sum()))
    assert np.array_equal(got[1], want[1]), "%s: keep %s, expected %s" % (what, got[1], want[1])
    assert np.array_equal(got[2], want[2]), "%s: mask_points %s, expected %s" % (what, got[2], want[2])


# ---- packing -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", V_EDGES)
def test_the_overlaps_and_the_nms_equal_the_restatement_at_the_vector_and_word_edges(v):
    rng = np.random.default_rng(1000 + v)
    for r in (1, 3, 7, 40):                                           # odd v: every row after the first starts unaligned
        masks = make_masks(rng, r, v)
        sizes, inter = overlaps(masks)
        want_s, want_i = ref.mask_overlaps_ref(masks)
        assert np.array_equal(sizes, want_s) and np.array_equal(inter, want_i), "V %d R %d" % (v, r)
        assert np.array_equal(inter, inter.T) and np.array_equal(np.diagonal(inter), sizes)
        if r >= 3:
            assert sizes[r - 1] == v and sizes[r - 2] == 1 and inter[r - 2, r - 1] == 1 and (r < 5 or sizes[r // 2] == 0)
        labels = rng.integers(0, 3, size=r)
        for th in (0.0, 0.3, 0.5):
            same(nms(masks, iou_th=th), ref.mask_nms_ref(masks, iou_th=th), "V %d R %d at %r" % (v, r, th))
            same(nms(masks, labels=labels, iou_th=th), ref.mask_nms_ref(masks, labels=labels, iou_th=th), "V %d R %d at %r with labels" % (v, r, th))


# ---- tiling --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", R_EDGES)
def test_the_row_counts_at_the_edges_of_the_pair_tile(r):
    rng = np.random.default_rng(2000 + r)
    for v in (257, 4099 + r):                                         # one word chunk and two
        masks = make_masks(rng, r, v)
        sizes, inter = overlaps(masks)
        want_s, want_i = ref.mask_overlaps_ref(masks)
        assert np.array_equal(sizes, want_s) and np.array_equal(inter, want_i), "R %d V %d" % (r, v)
        labels = rng.integers(0, 4, size=r)
        same(nms(masks, iou_th=0.25), ref.mask_nms_ref(masks, iou_th=0.25), "R %d V %d" % (r, v))
        same(nms(masks, labels=labels, iou_th=0.25), ref.mask_nms_ref(masks, labels=labels, iou_th=0.25), "R %d V %d with labels" % (r, v))


def test_two_scenes_with_their_own_counts():
    rng = np.random.default_rng(3)
    r, v = 37, 1027
    masks = np.stack([make_masks(rng, r, v), make_masks(rng, r, v), make_masks(rng, r, v), make_masks(rng, r, v)])
    labels = rng.integers(0, 3, size=(4, r))
    sizes, inter = overlaps(masks)
    for s in range(4):
        want = ref.mask_overlaps_ref(masks[s])
        assert np.array_equal(sizes[s], want[0]) and np.array_equal(inter[s], want[1])
    for count in ([0, r + 5], [20, r], [-3, 1], [r, 0]):
        count = count + [5, 33]
        got = nms(masks, count=count, labels=labels, iou_th=0.3)
        want = ref.mask_nms_batch_ref(masks, count, labels, 0.3)
        same(got, want, "counts %s" % (count,))
        for s, n in enumerate(count):                                 # rows at or beyond the count: not kept, untouched apart from the normalisation
            live = min(max(n, 0), r)
            assert not got[1][s, live:].any() and np.array_equal(got[0][s, live:], (masks[s, live:] != 0).astype(np.uint8))
            assert np.array_equal(got[2][s, live:], (masks[s, live:] != 0).sum(1))
    assert want[1][0].sum() < r                                       # and below it something was suppressed


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def rows(v, *sets):
    m = np.zeros((len(sets), v), np.uint8)
    for k, s in enumerate(sets):
        m[k, list(s)] = BYTES[1 + k % 3]
    return m


def test_identical_rows_leave_the_first():
    m = rows(70, range(5, 40), range(5, 40), range(5, 40), range(50, 60), range(50, 60))
    got = nms(m, iou_th=0.9)
    same(got, ref.mask_nms_ref(m, iou_th=0.9), "identical rows")
    assert got[1].tolist() == [1, 0, 0, 1, 0] and got[2].tolist() == [35, 0, 0, 10, 0] and not got[0][[1, 2, 4]].any()


def test_a_suppressed_row_suppresses_nobody():
    a, b, c = range(0, 100), range(40, 140), range(80, 180)           # IoU(A, B) = IoU(B, C) = 60 / 140, IoU(A, C) = 20 / 180
    m = rows(200, a, b, c)
    got = nms(m, iou_th=0.4)
    same(got, ref.mask_nms_ref(m, iou_th=0.4), "chain")
    assert got[1].tolist() == [1, 0, 1] and got[2].tolist() == [100, 0, 100]       # B alone would have suppressed C: C stays
    assert nms(m[1:], iou_th=0.4)[1].tolist() == [1, 0]                             # and B alone does suppress C


def test_an_iou_exactly_at_the_threshold_does_not_suppress():
    m = rows(9, (0, 1, 2), (1, 2, 3))                                 # inter 2, union 4
    assert nms(m, iou_th=0.5)[1].tolist() == [1, 1]
    assert nms(m, iou_th=0.4999999999999999)[1].tolist() == [1, 0]
    m = rows(300, range(0, 200), range(100, 250))                     # inter 100, union 250: 0.4 is not a double, 0.4 * 250 rounds to 100.0
    want = ref.mask_nms_ref(m, iou_th=0.4)
    same(nms(m, iou_th=0.4), want, "inter 100, union 250 at 0.4")
    assert want[1].tolist() == [1, int(not 100.0 > 0.4 * 250.0)]


def test_one_shared_vertex_suppresses_at_zero_and_empty_rows_do_nothing():
    m = rows(130, range(0, 64), (), (63, 64, 129), (), range(70, 80))
    got = nms(m, iou_th=0.0)
    same(got, ref.mask_nms_ref(m, iou_th=0.0), "at zero")
    assert got[1].tolist() == [1, 1, 0, 1, 1] and got[2].tolist() == [64, 0, 0, 0, 10]      # the empty rows are kept and empty


def test_labels_against_no_labels_on_the_same_masks():
    m = rows(100, range(0, 50), range(0, 50), range(0, 49), range(60, 90), range(61, 90))
    assert nms(m, iou_th=0.5)[1].tolist() == [1, 0, 0, 1, 0]
    labels = [3, 4, 3, -1, -1]
    got = nms(m, labels=labels, iou_th=0.5)
    same(got, ref.mask_nms_ref(m, labels=labels, iou_th=0.5), "with labels")
    assert got[1].tolist() == [1, 1, 0, 1, 0]                         # row 1 has another label; negative labels are labels like any other
    assert nms(m, labels=[1, 2, 3, 4, 5], iou_th=0.0)[1].tolist() == [1] * 5


# ---- in place, workspace, capture ----------------------------------------------------------------------------------------------------------
def case(b=2, r=41, v=4099, seed=7):
    rng = np.random.default_rng(seed)
    masks = np.stack([make_masks(rng, r, v) for _ in range(b)])
    return masks, rng.integers(0, r + 3, size=b), rng.integers(0, 3, size=(b, r))


def test_out_may_be_masks():
    from gspn_amd.mask_nms import mask_nms
    masks, count, labels = case()
    m, c, lab = dev(masks), dev(count, np.int32), dev(labels, np.int32)
    want = mask_nms(m, c, lab, iou_th=0.3)
    same(tuple(t.cpu().numpy() for t in want), ref.mask_nms_batch_ref(masks, count, labels, 0.3), "out of place")
    out, keep, points = mask_nms(m, c, lab, iou_th=0.3, out=m)
    assert out.data_ptr() == m.data_ptr() and torch.equal(out, want[0]) and torch.equal(keep, want[1]) and torch.equal(points, want[2])
    other = torch.full((2, 41, 4099), 9, dtype=torch.uint8, device="cuda")
    out, keep, points = mask_nms(dev(masks), c, lab, iou_th=0.3, out=other)
    assert out.data_ptr() == other.data_ptr() and torch.equal(other, want[0]) and torch.equal(keep, want[1])
    one = mask_nms(dev(masks[0]), c[0], lab[0], iou_th=0.3)           # 2-D inputs mean one scene
    assert one[0].shape == (41, 4099) and one[1].shape == (41,) and all(torch.equal(one[k], want[k][0]) for k in range(3))


def test_the_workspace_need_not_be_initialised_and_must_be_large_enough():
    from gspn_amd import _lib
    from gspn_amd.mask_nms import mask_nms, mask_overlaps
    masks, count, labels = case()
    b, r, v = masks.shape
    m, c, lab = dev(masks), dev(count, np.int32), dev(labels, np.int32)
    want, want_o = mask_nms(m, c, lab, iou_th=0.3), mask_overlaps(m)
    need, need_o = int(_lib.lib().gspn_mask_nms_ws_bytes(b, r, v)), int(_lib.lib().gspn_mask_overlaps_ws_bytes(b, r, v))
    words = (v + 63) // 64
    assert need_o == (8 * b * r * words + 15) // 16 * 16 and need >= need_o + 4 * b * r + 4 * b * r * r
    for fill in (0xFF, 0x00):
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")        # exactly _ws_bytes
        ws_o = torch.full((need_o,), fill, dtype=torch.uint8, device="cuda")
        for _ in range(2):                                            # and what the first call left changes nothing for the second
            got, got_o = mask_nms(m, c, lab, iou_th=0.3, ws=ws), mask_overlaps(m, ws=ws_o)
            assert all(torch.equal(got[k], want[k]) for k in range(3)) and all(torch.equal(got_o[k], want_o[k]) for k in range(2))
    for short in (lambda: mask_nms(m, c, lab, iou_th=0.3, ws=torch.empty((need - 1,), dtype=torch.uint8, device="cuda")),
                  lambda: mask_overlaps(m, ws=torch.empty((need_o - 1,), dtype=torch.uint8, device="cuda")),
                  lambda: mask_nms(m, c, lab, iou_th=0.3, ws=torch.empty((need + 16,), dtype=torch.uint8, device="cuda")[1:]),       # not 16-byte aligned
                  lambda: mask_nms(m, c, lab, iou_th=0.3, ws=torch.empty((need,), dtype=torch.uint8))):                              # not on the device
        with pytest.raises(ValueError, match="ws must be"):
            short()


def test_two_calls_give_identical_bits():
    from gspn_amd.mask_nms import mask_nms, mask_overlaps
    masks, count, labels = case(b=3, r=100, v=18001, seed=8)
    m, c, lab = dev(masks), dev(count, np.int32), dev(labels, np.int32)
    first, first_o = mask_nms(m, c, lab, iou_th=0.5), mask_overlaps(m)
    for _ in range(3):
        again, again_o = mask_nms(m, c, lab, iou_th=0.5), mask_overlaps(m)
        assert all(torch.equal(a, f) for a, f in zip(again + again_o, first + first_o))
    same(tuple(t.cpu().numpy() for t in first), ref.mask_nms_batch_ref(masks, count, labels, 0.5), "3 x 100 x 18001")


def test_the_calls_capture_with_a_caller_owned_workspace():
    from gspn_amd import _lib
    from gspn_amd.mask_nms import mask_nms, mask_overlaps
    inputs = [case(seed=20 + k) for k in range(3)]
    masks, count, labels = inputs[0]
    b, r, v = masks.shape
    m, c, lab = dev(masks), dev(count, np.int32), dev(labels, np.int32)
    ws = torch.empty((int(_lib.lib().gspn_mask_nms_ws_bytes(b, r, v)),), dtype=torch.uint8, device="cuda")
    ws_o = torch.empty((int(_lib.lib().gspn_mask_overlaps_ws_bytes(b, r, v)),), dtype=torch.uint8, device="cuda")
    mask_nms(m, c, lab, iou_th=0.3, ws=ws)                            # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mask_nms(m, c, lab, iou_th=0.3, ws=ws)
        out_o = mask_overlaps(m, ws=ws_o)
    for nm, nc, nl in inputs[1:]:
        m.copy_(torch.from_numpy(nm))
        c.copy_(torch.from_numpy(nc.astype(np.int32)))                # the count is read on the device: a replay sees the new one
        lab.copy_(torch.from_numpy(nl.astype(np.int32)))
        graph.replay()
        torch.cuda.synchronize()
        same(tuple(t.cpu().numpy() for t in out), ref.mask_nms_batch_ref(nm, nc, nl, 0.3), "replay")
        want_o = [ref.mask_overlaps_ref(nm[s]) for s in range(b)]
        assert np.array_equal(out_o[0].cpu().numpy(), np.stack([w[0] for w in want_o]))
        assert np.array_equal(out_o[1].cpu().numpy(), np.stack([w[1] for w in want_o]))


# ---- rows beyond 2^31 bytes ----------------------------------------------------------------------------------------------------------------
def test_row_offsets_are_64_bit():
    """1024 rows of 2^21 + 3 bytes, 2 GiB that never reach the host.  Row k sets one range [lo_k, hi_k), so size = hi - lo and inter =
    max(0, min(hi_i, hi_j) - max(lo_i, lo_j)) in closed form.  Byte 2^31 of the tensor is vertex V - 3072 of row 1023: rows 1022 and 1023
    straddle it and run into the last, ragged word (V = 64 * 32768 + 3), row 1021 starts on it, row 1020 is the two vertices around it; row
    0 is all set, row 511 is the last 3 vertices."""
    from gspn_amd.mask_nms import mask_nms, mask_overlaps
    r, v = 1024, (1 << 21) + 3
    k = np.arange(r, dtype=np.int64)
    lo = (k * 2039) % (v - 70000)
    hi = lo + 1 + (k * 7919) % 60000
    lo[0], hi[0] = 0, v
    lo[511], hi[511] = v - 3, v
    lo[1020:], hi[1020:] = [v - 3073, v - 3072, v - 4000, v - 5000], [v - 3071, v, v - 1, v]
    masks = torch.zeros((r, v), dtype=torch.uint8, device="cuda")
    for j in range(r):
        masks[j, lo[j]:hi[j]] = int(BYTES[1 + j % 3])
    assert 1023 * v + lo[1023] < (1 << 31) == 1023 * v + lo[1021] < 1023 * v + hi[1023]
    size = hi - lo
    inter = np.maximum(0, np.minimum(hi[:, None], hi[None, :]) - np.maximum(lo[:, None], lo[None, :]))
    got_s, got_i = mask_overlaps(masks)
    assert np.array_equal(got_s.cpu().numpy(), size) and np.array_equal(got_i.cpu().numpy(), inter)
    supp, _ = ref.greedy_ref(size, inter, None, None, 0.3)
    assert 10 < supp.sum() < r - 10 and supp[1020:].any() and not supp[1020:].all()
    out, keep, points = mask_nms(masks, iou_th=0.3, out=masks)
    assert out.data_ptr() == masks.data_ptr()
    assert np.array_equal(keep.cpu().numpy(), (~supp).astype(np.uint8)) and np.array_equal(points.cpu().numpy(), np.where(supp, 0, size))
    at = torch.arange(v, device="cuda")[None]
    dlo, dhi, dkeep = dev(lo)[:, None], dev(hi)[:, None], dev(~supp)[:, None]
    for j in range(0, r, 128):                                        # every byte of the result, 128 rows at a time
        want = ((at >= dlo[j:j + 128]) & (at < dhi[j:j + 128]) & dkeep[j:j + 128]).to(torch.uint8)
        assert torch.equal(out[j:j + 128], want), "rows %d.." % j


# ---- declines ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_decline_before_anything_is_launched():
    from gspn_amd import _lib as L
    lib = L.lib()
    b, r, v = 2, 3, 100
    masks = torch.zeros((b, r, v), dtype=torch.uint8, device="cuda")
    count = torch.full((b,), r, dtype=torch.int32, device="cuda")
    labels = torch.zeros((b, r), dtype=torch.int32, device="cuda")
    ws = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((b, r, v), 9, dtype=torch.uint8, device="cuda")
    keep = torch.full((b, r), 9, dtype=torch.uint8, device="cuda")
    points = torch.full((b, r), -9, dtype=torch.int32, device="cuda")
    sizes = torch.full((b, r), -9, dtype=torch.int32, device="cuda")
    inter = torch.full((b, r, r), -9, dtype=torch.int32, device="cuda")
    p, null, st = L.ptr, ctypes.c_void_p(0), L.stream()
    off = ctypes.c_void_p(ws.data_ptr() + 8)

    def mn(b=b, r=r, v=v, masks=p(masks), count=p(count), labels=p(labels), th=0.5, ws=p(ws), out=p(out), keep=p(keep), points=p(points)):
        return lib.gspn_mask_nms(b, r, v, masks, count, labels, th, ws, out, keep, points, st)

    def mo(b=b, r=r, v=v, masks=p(masks), ws=p(ws), sizes=p(sizes), inter=p(inter)):
        return lib.gspn_mask_overlaps(b, r, v, masks, ws, sizes, inter, st)

    ARG, UNS = -1, -2
    for kw in (dict(b=-1), dict(r=-1), dict(v=-1), dict(masks=null), dict(count=null), dict(ws=null), dict(out=null), dict(keep=null),
               dict(points=null), dict(th=float("nan")), dict(th=-0.001), dict(th=1.0), dict(th=1.5), dict(th=float("inf"))):
        assert mn(**kw) == ARG, kw
    for kw in (dict(r=1025), dict(v=(1 << 24) + 1), dict(b=65536), dict(ws=off)):
        assert mn(**kw) == UNS, kw
    for kw in (dict(b=-1), dict(r=-1), dict(v=-1), dict(masks=null), dict(ws=null), dict(sizes=null), dict(inter=null)):
        assert mo(**kw) == ARG, kw
    for kw in (dict(r=1025), dict(v=(1 << 24) + 1), dict(b=65536), dict(ws=off)):
        assert mo(**kw) == UNS, kw
    assert mn(b=0) == mn(r=0) == mn(v=0) == mo(b=0) == mo(r=0) == mo(v=0) == 0                          # nothing to do is no error
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and bool((keep == 9).all()) and bool((points == -9).all()) and bool((ws == 0x5A).all())           # nothing ran
    assert bool((sizes == -9).all()) and bool((inter == -9).all())
    nb, ob = lib.gspn_mask_nms_ws_bytes, lib.gspn_mask_overlaps_ws_bytes
    assert nb(b, r, v) > ob(b, r, v) > 0
    for args in ((-1, r, v), (b, -1, v), (b, r, -1), (0, r, v), (b, 0, v), (b, r, 0), (b, 1025, v), (b, r, (1 << 24) + 1), (65536, r, v)):
        assert nb(*args) == 0 and ob(*args) == 0, args
    assert mn(labels=null) == 0                                       # labels may be null: that call runs
    torch.cuda.synchronize()
    assert bool((keep == 1).all()) and not bool(out.any())


def test_the_wrappers_decline_before_the_library_is_touched():
    from gspn_amd.mask_nms import mask_nms, mask_overlaps
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")              # noqa: E731
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")             # noqa: E731
    for bad in (u8(1025, 2), u8(1, (1 << 24) + 1)):
        with pytest.raises(NotImplementedError):
            mask_nms(bad, iou_th=0.5)
        with pytest.raises(NotImplementedError):
            mask_overlaps(bad)
    for th in (float("nan"), -0.1, 1.0):
        with pytest.raises(ValueError, match="iou_th"):
            mask_nms(u8(2, 4), iou_th=th)
    with pytest.raises(TypeError):
        mask_nms(u8(2, 4))                                            # no default: the caller states the threshold
    with pytest.raises(ValueError, match="out must be"):
        mask_nms(u8(2, 4), iou_th=0.5, out=u8(2, 5))
    with pytest.raises(ValueError, match="out must be"):
        mask_nms(u8(2, 4), iou_th=0.5, out=u8(4, 2).t())
    with pytest.raises(ValueError, match="count must be"):
        mask_nms(u8(3, 2, 4), i32(2), iou_th=0.5)
    with pytest.raises(ValueError, match="labels must be"):
        mask_nms(u8(3, 2, 4), None, i32(3, 3), iou_th=0.5)


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------------
def test_the_stage_removes_duplicates_that_cost_ap():
    """6 instances, each a union of synth.scan_segments segments.  Row 2i is the ground truth of instance i, row 2i + 1 the same with every
    seventh vertex cleared (IoU 6/7 with row 2i and with the ground truth), ranked behind it, with the same label; two instances share
    each of three classes.  On the input the duplicate of a class's first instance is a false positive ranked above the true positive of
    its second, at every threshold; the NMS at 0.5 empties it, and every ground truth is left with one prediction at IoU 1: AP, AP50 and
    AP25 are exactly 1.  (With one class per instance the input would score 1 as well: a false positive behind a class's last true
    positive costs the benchmark's AP nothing.  With two instances a class the recall steps, 0.5 and 1, are exact in binary, so the 1.0 is
    exact; with three the benchmark's own sum of thirds gives 0.9999999999999998 for a perfect prediction.)"""
    from gspn_amd import synth
    from gspn_amd.evaluate import MIN_REGION_SIZE, InstanceAP
    from gspn_amd.mask_nms import mask_nms
    from gspn_amd.segments import compact_segments
    rng = np.random.default_rng(12)
    n_ins, per = 6, 700
    centres = np.array([[2.0 * g, 0.0, 0.0] for g in range(n_ins)], np.float32)
    xyz = np.concatenate([centres[g] + rng.random((per, 3), dtype=np.float32) for g in range(n_ins)])
    group = np.repeat(np.arange(n_ins), per).astype(np.int32)
    sem = (group // 2 + 1).astype(np.int32)                            # classes 1, 2 and 3, two instances each
    order = rng.permutation(xyz.shape[0])
    xyz, group, sem = xyz[order], group[order], sem[order]
    seg, s = compact_segments(torch.from_numpy(synth.scan_segments(xyz, sem, group, 0.5, seed=13)).cuda())
    seg_np = seg.cpu().numpy()
    assert s >= 8 * n_ins and np.bincount(group).min() >= MIN_REGION_SIZE
    rows_ = []
    for g in range(n_ins):
        members = np.unique(seg_np[group == g])
        assert all(np.unique(group[seg_np == m]).size == 1 for m in members)      # the instance is a union of segments
        truth = np.isin(seg_np, members)
        assert np.array_equal(truth, group == g)
        copy = truth.copy()
        copy[np.nonzero(truth)[0][6::7]] = False                      # every seventh vertex of the instance cleared
        rows_ += [truth, copy]
    masks = torch.from_numpy(np.stack(rows_).astype(np.uint8) * 255).cuda()
    cls = (torch.arange(n_ins, dtype=torch.int32, device="cuda") // 2 + 1).repeat_interleave(2)
    count = torch.tensor(2 * n_ins, dtype=torch.int32, device="cuda")
    out, keep, points = mask_nms(masks, count, cls, iou_th=0.5)
    assert keep.tolist() == [1, 0] * n_ins and points.tolist() == [per, 0] * n_ins
    assert torch.equal(out[0::2], (masks[0::2] != 0).to(torch.uint8)) and not bool(out[1::2].any())

    def figures(m):
        metric = InstanceAP(4, label_map=None)
        conf = torch.linspace(0.9, 0.4, 2 * n_ins, device="cuda")[None]
        metric.add(m[None], cls[None], conf, count[None], torch.from_numpy(sem).cuda()[None], torch.from_numpy(group).cuda()[None], n_ins)
        res = metric.compute()
        return res["all_ap"], res["all_ap_50%"], res["all_ap_25%"]

    before, after = figures((masks != 0).to(torch.uint8)), figures(out)
    print("AP / AP50 / AP25: %.4f / %.4f / %.4f on the input rows, %.4f / %.4f / %.4f behind the NMS" % (before + after))
    assert after == (1.0, 1.0, 1.0)
    assert all(x < 1.0 for x in before)
