"""GPU tests of mask holes (gspn_amd/holes.py, csrc/components.hip), bit for bit against the numpy restatement
(tests/holes_ref.py, written from the rule).  The vertex counts put the rows at every misalignment of the aligned 16-byte reads and
stores, the row counts are the word edges of the two vertex-major tables."""
import ctypes

import numpy as np
import pytest
import torch

from tests import holes_ref as ref
from tests.components_ref import edges_ref

pytestmark = pytest.mark.gpu

V_EDGES = (1, 15, 16, 17, 63, 64, 65, 1023, 1025, 4095)
R_EDGES = (1, 33, 64, 65, 129)                                        # the tables have ceil(R / 64) words per vertex
BYTES = np.array([1, 2, 255], np.uint8)
RULES = ((6, 1.0), (40, 1.0), (40, 0.25), (0, 1.0))                   # (max_vertices, max_share)
HEIGHTS = np.array([0.0, 0.005, 0.01], np.float32)                    # a thin height noise: many vertices on the box's z faces too


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).cuda()


def path_faces(order):
    """one degenerate face (a, b, b) per edge of the path through `order`: exactly those edges"""
    order = np.asarray(order)
    return np.stack((order[:-1], order[1:], order[1:]), axis=1).astype(np.int32)


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------
def make_scene(rng, v):
    """A triangulated w x h lattice with integer x and y, so that many candidates lie exactly on a box face, the vertex indices shuffled;
    the vertices the lattice leaves over are loose fragments, chains of three joined to nothing else, somewhere over the lattice.
    -> xyz (v, 3) float32, faces (F, 3) int32, at (h, w): the vertex of a lattice point"""
    n = max(1, v - v // 8)
    w = int(np.ceil(np.sqrt(n)))
    h = n // w
    if h == 0:
        w, h = n, 1
    order = rng.permutation(v)
    at = order[:w * h].reshape(h, w)
    xyz = np.zeros((v, 3), np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    xyz[at, 0], xyz[at, 1] = xs, ys
    loose = order[w * h:]
    xyz[loose, 0], xyz[loose, 1] = rng.integers(0, w, size=loose.size), rng.integers(0, h, size=loose.size)
    xyz[:, 2] = HEIGHTS[rng.integers(0, 3, size=v)]
    a, b, c, d = at[:-1, :-1].ravel(), at[:-1, 1:].ravel(), at[1:, :-1].ravel(), at[1:, 1:].ravel()
    faces = [np.stack((a, b, c), axis=1), np.stack((b, d, c), axis=1)]
    if h == 1 and w > 1:
        faces.append(path_faces(at[0]))
    for k in range(0, loose.size - 2, 3):
        faces.append(loose[k:k + 3][None])
    faces.append(np.array([[0, 0, 0], [v, 0, v - 1], [-(1 << 31), 0, (1 << 31) - 1], [v - 1, -1, 0]]))       # no edge inside [0, v) but 0 - (v - 1)
    faces = np.concatenate(faces)
    faces = np.concatenate((faces, faces[:5]))
    return xyz, faces[rng.permutation(faces.shape[0])].astype(np.int32), at


def make_rows(rng, r, v, at):
    """rows of frames, frames with a gap, U shapes and filled rectangles with two vertices knocked out, one to three a row, three in ten
    pushed against the lattice's border; set bytes of 1, 2 and 255; from three rows on, row 1 is empty and the last row all set"""
    h, w = at.shape
    on = np.zeros((r, v), bool)
    for k in range(r):
        for _ in range(int(rng.integers(1, 4))):
            ww, hh = int(rng.integers(min(3, w), min(w, 14) + 1)), int(rng.integers(min(3, h), min(h, 14) + 1))
            x0, y0 = int(rng.integers(0, w - ww + 1)), int(rng.integers(0, h - hh + 1))
            if rng.random() < 0.3:
                x0 = (0, w - ww)[int(rng.integers(0, 2))]
            if rng.random() < 0.3:
                y0 = (0, h - hh)[int(rng.integers(0, 2))]
            box = at[y0:y0 + hh, x0:x0 + ww]
            shape = np.ones(box.shape, bool)
            kind = int(rng.integers(0, 4))
            if kind < 3:
                shape[1:-1, 1:-1] = False                             # a frame
            if kind == 1 and ww > 2:
                shape[0, int(rng.integers(1, ww - 1))] = False        # with a gap
            if kind == 2:
                side = int(rng.integers(0, 4))                        # a U: a frame without the inside of one side
                (shape[0], shape[-1], shape[:, 0], shape[:, -1])[side][1:-1] = False
            if kind == 3:
                shape.ravel()[rng.integers(0, shape.size, size=2)] = False
            on[k, box[shape]] = True
    if r >= 3:
        on[1] = False
        on[-1] = True
    return (BYTES[rng.integers(0, 3, size=(r, v))] * on).astype(np.uint8)


def filled(masks, faces, xyz, max_vertices, max_share=1.0, label=True, **kw):
    from gspn_amd.holes import hole_fill
    got = hole_fill(dev(masks), dev(faces, np.int32).reshape(-1, 3), dev(xyz, np.float32), max_vertices=max_vertices, max_share=max_share,
                    label=label, **kw)
    assert [t.dtype for t in got] == [torch.uint8] + [torch.int32] * (4 if label else 3) and got[0].shape == masks.shape
    return tuple(t.cpu().numpy() for t in got)


def same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:5].tolist())


def check(masks, faces, xyz, what, rules=RULES):
    """the op with its labels against the restatement; nholes >= 0 everywhere -> the restatement's info of the last rule"""
    for mv, share in rules:
        want = ref.hole_fill_ref(masks, faces, xyz, mv, share, info=True)
        got = filled(masks, faces, xyz, mv, share)
        assert (got[2] >= 0).all(), what
        same(got, want[:5], "%s fill(%d, %r)" % (what, mv, share))
    return want


# ---- the sizes -----------------------------------------------------------------------------------------------------------------------------
SEEN = {"filled": 0, "open": 0, "closed, touches nothing": 0, "closed, touches, too large": 0}


def tally(want, max_vertices):
    """what the restatement alone says the case holds"""
    for row in want[5]:
        for s, is_open, touches in row.values():
            SEEN["open"] += is_open
            SEEN["closed, touches nothing"] += not is_open and not touches
            SEEN["closed, touches, too large"] += not is_open and touches and s > max_vertices
    SEEN["filled"] += int(want[2].sum())


def sweep_cases(only=V_EDGES):
    for v in only:
        rng = np.random.default_rng(2000 + v)
        xyz, faces, at = make_scene(rng, v)
        for r in R_EDGES:
            yield v, r, make_rows(rng, r, v, at), faces, xyz, (RULES if r in (1, 65) else RULES[:1])


def test_the_sweep_spreads_over_the_four_kinds_on_the_restatement():
    """no device call: a sweep that the reference alone does not spread over a filled hole, an open component, a closed component that
    touches nothing and a closed touching one over the size limit proves nothing"""
    for key in SEEN:
        SEEN[key] = 0
    for v, r, masks, faces, xyz, rules in sweep_cases():
        if v <= 1025 or r <= 33:                                      # (enough for the tally: the restatement is slow)
            tally(ref.hole_fill_ref(masks, faces, xyz, rules[0][0], rules[0][1], info=True), rules[0][0])
    print("the sweep on the restatement:", SEEN)
    assert all(n >= 1 for n in SEEN.values()), SEEN


@pytest.mark.parametrize("v", V_EDGES)
def test_the_op_equals_the_restatement_at_the_vector_and_word_edges(v):
    for _, r, masks, faces, xyz, rules in sweep_cases((v,)):
        check(masks, faces, xyz, "R %d V %d" % (r, v), rules=rules)


def test_no_faces_is_the_identity():
    rng = np.random.default_rng(3)
    xyz, faces, at = make_scene(rng, 1000)
    masks = make_rows(rng, 5, 1000, at)
    none = np.zeros((0, 3), np.int32)
    want = check(masks, none, xyz, "F = 0", rules=RULES[1:2])
    out, points, nholes, nfilled, label = filled(masks, none, xyz, 40)
    assert np.array_equal(out, (masks != 0).astype(np.uint8)) and not nholes.any() and not nfilled.any()
    assert np.array_equal(points, (masks != 0).sum(1)) and (label[masks != 0] == -2).all() and want[2].sum() == 0
    # faces that name no edge at all: the same
    same(filled(masks, np.array([[5, 5, 5], [-1, 2000, 1000], [3, -4, 3]], np.int32), xyz, 40), (out, points, nholes, nfilled, label), "no edge")


def test_faces_out_of_range_and_degenerate_faces():
    rng = np.random.default_rng(4)
    v = 777
    xyz, faces, at = make_scene(rng, v)
    more = np.concatenate((faces, rng.integers(-3, v + 3, size=(40, 3)), np.repeat(rng.integers(0, v, size=(20, 1)), 3, axis=1),
                           path_faces(rng.integers(0, v, size=30)))).astype(np.int32)
    check(make_rows(rng, 7, v, at), more, xyz, "odd faces", rules=RULES[:2])


# ---- the shapes of the graph -----------------------------------------------------------------------------------------------------------------
def test_a_hole_that_is_a_path_of_5000_candidates_in_shuffled_order():
    """Two paths of 5000 candidates along x, each closed at both ends by set vertices.  The first is a hole.  The second has one more
    edge, from its vertex of the largest index to an unset vertex outside the box: it comes out open as a whole, which needs the mark
    pass to read final roots."""
    rng = np.random.default_rng(11)
    n = 5000
    v = 2 * (n + 2) + 1 + n
    order = rng.permutation(v)
    first, second, outside, pad = order[:n + 2], order[n + 2:2 * n + 4], order[2 * n + 4], order[2 * n + 5:]
    xyz = np.zeros((v, 3), np.float32)                                # (pad: n set vertices on no edge at the origin, for the share rule)
    xyz[first, 0] = np.arange(n + 2)
    xyz[second, 0], xyz[second, 1] = np.arange(n + 2), 1.0
    xyz[outside] = (10.0, 5.0, 0.0)
    far = second[1:-1][np.argmax(second[1:-1])]
    faces = np.concatenate((path_faces(first), path_faces(second), np.array([[far, outside, outside]], np.int32)))
    faces = faces[rng.permutation(faces.shape[0])]
    masks = np.zeros((2, v), np.uint8)
    masks[:, [first[0], first[-1], second[0], second[-1]]] = 255
    masks[:, pad] = 2
    masks[1, second[1:-1]] = 1                                        # row 1: the second path is set, its only hole is the first
    for mv in (n, n - 1):
        want = ref.hole_fill_ref(masks, faces, xyz, mv)
        got = filled(masks, faces, xyz, mv)
        same(got, want, "paths, max_vertices %d" % mv)
        assert got[2].tolist() == [int(mv == n)] * 2 and got[3].tolist() == [n * (mv == n)] * 2
        assert (got[4][0, first[1:-1]] == first[1:-1].min()).all() and (got[4][0, second[1:-1]] == second[1:-1].min()).all()
        assert not got[0][0, second[1:-1]].any() and got[0][0, first[1:-1]].all() == (mv == n) and got[4][0, outside] == -1


# ---- the coordinates -------------------------------------------------------------------------------------------------------------------------
def ring_scene():
    """a 7 x 7 lattice in index order; row 0 the ring of the middle 5 x 5 (a 3 x 3 hole), row 1 the same with vertex 24, the centre, set"""
    ys, xs = np.mgrid[0:7, 0:7]
    at = np.arange(49).reshape(7, 7)
    xyz = np.stack((xs.ravel(), ys.ravel(), np.zeros(49)), axis=1).astype(np.float32)
    a, b, c, d = at[:-1, :-1].ravel(), at[:-1, 1:].ravel(), at[1:, :-1].ravel(), at[1:, 1:].ravel()
    faces = np.concatenate((np.stack((a, b, c), axis=1), np.stack((b, d, c), axis=1))).astype(np.int32)
    masks = np.zeros((2, 49), np.uint8)
    ring = np.ones((5, 5), bool)
    ring[1:-1, 1:-1] = False
    masks[:, at[1:6, 1:6][ring]] = 1
    masks[1, 24] = 7
    return masks, faces, xyz, at


def test_the_coordinates():
    masks, faces, xyz, at = ring_scene()
    inner = at[2:5, 2:5].ravel()
    out, points, nholes, nfilled, label = check(masks, faces, xyz, "the ring")[:5]
    got = filled(masks, faces, xyz, 40)
    assert got[2].tolist() == [1, 1] and got[3].tolist() == [9, 8] and got[0][:, inner].all() and got[1].tolist() == [25, 25]
    assert (got[4][0, inner] == inner.min()).all() and got[4][0, 0] == -1 and got[4][0, at[1, 1]] == -2       # every candidate is ON a box face in z
    # -0.0 against +0.0: the ring at +0.0 in z and at x = 0 after the shift, the inside at -0.0
    signed = xyz.copy()
    signed[:, 0] -= 1.0
    signed[inner, 2] = -0.0
    signed[at[1:6, 1], 0] = -0.0
    same(filled(masks, faces, signed, 40), ref.hole_fill_ref(masks, faces, signed, 40), "signed zeros")
    assert filled(masks, faces, signed, 40)[2].tolist() == [1, 1]
    # an offset of 5e5: float32 holds the integers there
    far = xyz + np.float32(5e5)
    same(filled(masks, faces, far, 40), ref.hole_fill_ref(masks, faces, far, 40), "offset")
    assert filled(masks, faces, far, 40)[3].tolist() == [9, 8]
    # all set vertices at one point: the box is that point, and a candidate is an unset vertex exactly there
    point = xyz.copy()
    point[masks[0] != 0] = (3.0, 3.0, 0.0)
    got = filled(masks, faces, point, 40)
    same(got, ref.hole_fill_ref(masks, faces, point, 40), "one point")
    assert (got[4][0] >= 0).sum() == 1 and got[4][0, 24] == 24 and got[2].tolist() == [0, 0]                  # the centre's neighbours are outside: open
    # NaN and inf on set vertices leave them out of the box; on unset vertices they are never inside
    for bad in (np.nan, np.inf, -np.inf):
        odd = xyz.copy()
        odd[at[1, 3], 1] = bad                                        # a set vertex of the ring: the box is unchanged by the others
        odd[at[3, 3], 0] = bad                                        # the centre: no candidate in row 0, so its neighbours are open
        odd[0, 2] = bad
        got = filled(masks, faces, odd, 40)
        same(got, ref.hole_fill_ref(masks, faces, odd, 40), "non-finite %r" % bad)
        assert got[2].tolist() == [0, 1] and got[4][0, 24] == -1 and got[4][1, 24] == -2
    none = xyz.copy()
    none[masks[0] != 0, 0] = np.nan                                   # every set vertex of row 0 carries a NaN: no box
    got = filled(masks, faces, none, 40)
    same(got, ref.hole_fill_ref(masks, faces, none, 40), "no box")
    assert (got[4][0][masks[0] == 0] == -1).all() and got[2][0] == 0


# ---- the calling conventions -----------------------------------------------------------------------------------------------------------------
def case(r=41, v=4099, seed=7):
    xyz, faces, at = make_scene(np.random.default_rng(99), v)         # one mesh, masks by the seed
    return make_rows(np.random.default_rng(seed), r, v, at), faces, xyz


def test_out_may_be_masks():
    from gspn_amd.holes import hole_fill
    masks, faces, xyz = case()
    want = ref.hole_fill_ref(masks, faces, xyz, 40)
    m, f, x = dev(masks), dev(faces), dev(xyz)
    got = hole_fill(m, f, x, max_vertices=40, out=m, label=True)
    assert got[0].data_ptr() == m.data_ptr()
    same(tuple(t.cpu().numpy() for t in got), want, "in place")
    assert not np.array_equal(want[0], (masks != 0).astype(np.uint8))  # the case fills something
    other = torch.full_like(m, 77)
    out = hole_fill(dev(masks), f, x, max_vertices=40, out=other)[0]
    assert out.data_ptr() == other.data_ptr() and np.array_equal(other.cpu().numpy(), want[0])               # every byte written


def test_two_calls_give_identical_bits():
    masks, faces, xyz = case(seed=8)
    same(filled(masks, faces, xyz, 30, 0.5), filled(masks, faces, xyz, 30, 0.5), "twice")


def test_the_workspace_need_not_be_initialised_and_must_be_large_enough():
    from gspn_amd import _lib
    from gspn_amd.holes import hole_fill
    masks, faces, xyz = case(seed=9)
    r, v = masks.shape
    m, f, x = dev(masks), dev(faces), dev(xyz)
    need = int(_lib.lib().gspn_mask_hole_fill_ws_bytes(r, v, faces.shape[0]))
    want = ref.hole_fill_ref(masks, faces, xyz, 30, 0.5)
    for poison in (0xFF, 0x00, 0x5A):
        for label in (True, False):                                   # without a label the parents live in the workspace
            ws = torch.full((need + 64,), poison, dtype=torch.uint8, device="cuda")
            got = hole_fill(m, f, x, max_vertices=30, max_share=0.5, ws=ws, label=label)
            same(tuple(t.cpu().numpy() for t in got), want[:len(got)], "ws of %#x" % poison)
            assert (ws[need:] == poison).all()                        # nothing is written behind what the call asked for
    ws = torch.zeros((need + 64,), dtype=torch.uint8, device="cuda")
    for bad in (ws[:need - 1], ws[8:], ws[::2], ws.cpu()):
        with pytest.raises(ValueError, match="ws must be"):
            hole_fill(m, f, x, max_vertices=30, ws=bad)


def test_the_call_captures_with_a_caller_owned_workspace():
    from gspn_amd import _lib
    from gspn_amd.holes import hole_fill
    inputs = [case(seed=20 + k)[0] for k in range(3)]
    _, faces, xyz = case()
    r, v = inputs[0].shape
    m, f, x = dev(inputs[0]), dev(faces), dev(xyz)
    ws = torch.empty((int(_lib.lib().gspn_mask_hole_fill_ws_bytes(r, v, faces.shape[0])),), dtype=torch.uint8, device="cuda")
    hole_fill(m, f, x, max_vertices=40, ws=ws)                        # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = hole_fill(m, f, x, max_vertices=40, ws=ws, label=True)
    for nm in inputs[1:]:
        m.copy_(torch.from_numpy(nm))
        graph.replay()
        torch.cuda.synchronize()
        same(tuple(t.cpu().numpy() for t in got), ref.hole_fill_ref(nm, faces, xyz, 40), "replay")


# ---- rows beyond 2^31 ------------------------------------------------------------------------------------------------------------------------
def test_row_offsets_are_64_bit():
    """129 rows of 2^24 vertices on a line, x = the index: row 128 starts at byte 2^31 of the masks and at element 2^31 of the parents.
    All rows are empty but the first and the last.  The mesh is a set of strips [lo, hi), each a path; a row sets a strip but for gaps
    [a, b) inside it, which are candidate components of b - a vertices whose smallest is a, closed by the strip on both sides.  A strip
    the row does not set at all, inside its box, is a closed component that touches nothing; the unset vertices between the strips are
    candidates on no edge.  About 25 GB with the workspace and the labels; nothing reaches the host but the counters and the two rows."""
    from gspn_amd.holes import hole_fill
    r, v = 129, 1 << 24
    # row -> [(lo, hi, [(a, b), ...])]; the first and the last strip reach the row's two ends
    strips = {0: [(0, 1500, [(100, 130), (700, 1000)]), (70000, 70300, [(70100, 70150)]), (9999000, 10000000, []), (v - 2500, v, [(v - 2000, v - 1960), (v - 50, v - 1)])],
              128: [(0, 1500, [(1, 41)]), (70000, 70300, [(70010, 70020), (70200, 70299)]), (5000000, 5003000, [(5001000, 5001041)]), (v - 2500, v, [(v - 1000, v - 960)])]}
    every = sorted({(lo, hi) for rows in strips.values() for lo, hi, _ in rows})
    faces = np.concatenate([path_faces(np.arange(lo, hi)) for lo, hi in every])
    faces = dev(faces[np.random.default_rng(5).permutation(faces.shape[0])])
    xyz = torch.zeros((v, 3), dtype=torch.float32, device="cuda")
    xyz[:, 0] = torch.arange(v, device="cuda", dtype=torch.float32)   # exact below 2^24
    masks = torch.zeros((r, v), dtype=torch.uint8, device="cuda")
    limit = 41
    want_out, want_label, want = {}, {}, {}
    for k, rows in strips.items():
        label = torch.arange(v, dtype=torch.int32, device="cuda")     # the whole line is inside the box: the strips reach both ends
        for lo, hi in every:
            label[lo:hi] = lo                                         # a strip the row does not set: one component
        out = torch.zeros((v,), dtype=torch.uint8, device="cuda")
        holes = filled_ = 0
        for j, (lo, hi, gaps) in enumerate(rows):
            masks[k, lo:hi] = int(BYTES[j % 3])
            label[lo:hi] = -2
            out[lo:hi] = 1
            for a, b in gaps:
                masks[k, a:b] = 0
                label[a:b] = a
                out[a:b] = int(b - a <= limit)
                holes += int(b - a <= limit)
                filled_ += (b - a) * int(b - a <= limit)
        want_out[k], want_label[k], want[k] = out, label, (holes, filled_, int((masks[k] != 0).sum()) + filled_)
    assert want[0][0] == 2 and want[128][0] == 4                      # gaps of 30 and 40, not 300, 50 and 49 / of 40, 10, 41 and 40, not 99
    out, points, nholes, nfilled, label = hole_fill(masks, faces, xyz, max_vertices=limit, label=True)
    assert nholes.tolist() == [want[0][0]] + [0] * 127 + [want[128][0]] and nfilled.tolist() == [want[0][1]] + [0] * 127 + [want[128][1]]
    assert points.tolist() == [want[0][2]] + [0] * 127 + [want[128][2]]
    for k in strips:
        assert torch.equal(out[k], want_out[k]) and torch.equal(label[k], want_label[k]), k
    for j in range(1, 128, 16):
        assert bool((label[j:min(j + 16, 128)] == -1).all()) and not bool(out[j:min(j + 16, 128)].any()), j
    del label, out
    out, points, nholes, nfilled = hole_fill(masks, faces, xyz, max_vertices=limit, out=masks)          # in place, the parents in the workspace
    assert out.data_ptr() == masks.data_ptr() and nholes.tolist() == [want[0][0]] + [0] * 127 + [want[128][0]]
    assert points.tolist() == [want[0][2]] + [0] * 127 + [want[128][2]]
    for k in strips:
        assert torch.equal(out[k], want_out[k]), k
    assert not bool(out[1:128].any())


# ---- declines --------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_declines_with_device_pointers_and_leaves_the_outputs_alone():
    from gspn_amd import _lib
    lib = _lib.lib()
    masks, faces, xyz = case(r=3, v=100)
    m, f, x = dev(masks), dev(faces), dev(xyz)
    nf = faces.shape[0]
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    label = torch.full((3, 100), 77, dtype=torch.int32, device="cuda")
    a, b, c = (torch.full((3,), 77, dtype=torch.int32, device="cuda") for _ in range(3))
    out = torch.full((3, 100), 77, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                       # noqa: E731
    st, null = _lib.stream(), ctypes.c_void_p(0)
    call = lambda r=3, v=100, mv=5, sh=0.5, w=p(ws), xp=p(x): lib.gspn_mask_hole_fill(r, v, nf, p(m), p(f), xp, mv, sh, w, p(out), p(a), p(b), p(c), p(label), st)   # noqa: E731
    assert call(w=ctypes.c_void_p(ws.data_ptr() + 8)) == -2 and call(r=1025) == -2 and call(v=(1 << 24) + 1) == -2
    assert call(mv=-1) == -1 and call(sh=float("nan")) == -1 and call(sh=1.5) == -1 and call(sh=-0.1) == -1 and call(xp=null) == -1
    assert call(r=1025, mv=-1) == -1                                  # an argument error goes first
    assert call(r=0) == 0 and call(v=0) == 0                          # nothing to do, nothing written
    torch.cuda.synchronize()
    assert (label == 77).all() and (a == 77).all() and (b == 77).all() and (c == 77).all() and (out == 77).all() and not ws.any()
    assert torch.equal(m.cpu(), torch.from_numpy(masks))


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------------------
def test_the_stage_fills_gaps_that_cost_ap50():
    """test_the_stage_drops_islands_that_cost_ap50's scene with gaps instead of islands: 6 synth.scan_faces instances of 700 vertices, two
    to each of three classes, centres 2 apart.  Row i is instance i minus five connected patches of 80 vertices grown over the mesh's
    edges inside it; the patches do not touch one another and none holds one of the instance's six extreme vertices, so the row's box is
    the instance's.  The IoU with the instance is 300 / 700 = 0.43: AP50 0 and AP25 1 on the input rows.  Behind
    hole_fill(max_vertices=80) every row is its instance and AP, AP50 and AP25 are exactly 1; with max_vertices=79 nothing is filled."""
    from gspn_amd import synth
    from gspn_amd.evaluate import MIN_REGION_SIZE, InstanceAP
    from gspn_amd.holes import hole_fill
    rng = np.random.default_rng(12)
    n_ins, per, patches, patch = 6, 700, 5, 80
    centres = np.array([[2.0 * g, 0.0, 0.0] for g in range(n_ins)], np.float32)
    xyz = np.concatenate([centres[g] + rng.random((per, 3), dtype=np.float32) for g in range(n_ins)])
    group = np.repeat(np.arange(n_ins), per).astype(np.int32)
    sem = (group // 2 + 1).astype(np.int32)                            # classes 1, 2 and 3, two instances each
    order = rng.permutation(xyz.shape[0])
    xyz, group, sem = xyz[order], group[order], sem[order]
    v = xyz.shape[0]
    faces = synth.scan_faces(xyz, sem, group, 0.5, seed=13)
    edges = edges_ref(faces, v)
    assert np.bincount(group).min() >= MIN_REGION_SIZE
    nbr = [[] for _ in range(v)]
    for a, b in edges.tolist():
        nbr[a].append(b)
        nbr[b].append(a)

    def grown(allowed, number):
        """`patch` vertices of `allowed` that are connected among themselves: grown from a seeded vertex over the mesh's edges"""
        free = np.flatnonzero(allowed)
        for attempt in range(free.size):                              # (a start in a pocket too small for a patch: the next one)
            start = int(free[(97 * number + attempt) % free.size])
            seen, todo = {start}, [start]
            while todo and len(seen) < patch:
                for w in nbr[todo.pop(0)]:
                    if allowed[w] and w not in seen and len(seen) < patch:
                        seen.add(w)
                        todo.append(w)
            if len(seen) == patch:
                return sorted(seen)
        raise AssertionError("no room for a patch of %d" % patch)

    rows_ = []
    for g in range(n_ins):
        mine = group == g
        allowed = mine.copy()
        at = np.flatnonzero(mine)
        allowed[at[np.concatenate((xyz[at].argmin(axis=0), xyz[at].argmax(axis=0)))]] = False          # the six extreme vertices stay set
        row = mine.copy()
        for j in range(patches):
            cut = grown(allowed, 5 * g + j)
            row[cut] = False
            allowed[cut] = False
            allowed[[w for x in cut for w in nbr[x]]] = False          # the next patch keeps one vertex away from this one
        rows_.append(row)
    masks_np = np.stack(rows_).astype(np.uint8) * 255
    instances = np.stack([group == g for g in range(n_ins)]).astype(np.uint8)
    # the premises, on the restatement
    want = ref.hole_fill_ref(masks_np, faces, xyz, patch, info=True)
    iou = [float(rows_[g].sum()) / per for g in range(n_ins)]
    assert all(0.25 < x < 0.5 for x in iou) and iou[0] == 300 / 700
    assert all(sorted(s for s, _, _ in row.values()) == [patch] * patches and not any(o for _, o, _ in row.values()) for row in want[5])
    assert np.array_equal(want[0], instances) and want[2].tolist() == [patches] * n_ins and want[3].tolist() == [patches * patch] * n_ins
    masks = torch.from_numpy(masks_np).cuda()
    cls = torch.arange(n_ins, dtype=torch.int32, device="cuda") // 2 + 1
    count = torch.tensor(n_ins, dtype=torch.int32, device="cuda")
    got = hole_fill(masks, dev(faces), dev(xyz), max_vertices=patch, label=True)
    same(tuple(t.cpu().numpy() for t in got), want[:5], "gaps")
    out, points, nholes, nfilled, _ = got
    assert nholes.tolist() == [5] * n_ins and nfilled.tolist() == [400] * n_ins and points.tolist() == [per] * n_ins
    assert np.array_equal(out.cpu().numpy(), instances)
    below = hole_fill(masks, dev(faces), dev(xyz), max_vertices=patch - 1)
    assert not below[2].any() and not below[3].any() and np.array_equal(below[0].cpu().numpy(), (masks_np != 0).astype(np.uint8))

    def figures(m):
        metric = InstanceAP(4, label_map=None)
        conf = torch.linspace(0.9, 0.4, n_ins, device="cuda")[None]
        metric.add(m[None], cls[None], conf, count[None], torch.from_numpy(sem).cuda()[None], torch.from_numpy(group).cuda()[None], n_ins)
        res = metric.compute()
        return res["all_ap"], res["all_ap_50%"], res["all_ap_25%"]

    before, after = figures((masks != 0).to(torch.uint8)), figures(out)
    print("AP / AP50 / AP25: %.4f / %.4f / %.4f on the input rows, %.4f / %.4f / %.4f behind the fill" % (before + after))
    assert before[1] == 0.0 and before[2] == 1.0                      # the input rows miss AP50 on every instance and make AP25 on every one
    assert after == (1.0, 1.0, 1.0)
