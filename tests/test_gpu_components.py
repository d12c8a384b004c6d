"""GPU tests of mask components (gspn_amd/components.py, csrc/components.hip), bit for bit against the numpy restatement
(tests/components_ref.py: a plain union-find over the edges of each row, written from the rule).  The vertex counts put the rows at every
misalignment of the aligned 16-byte reads and stores, the row counts are the word edges of the vertex-major table."""
import ctypes

import numpy as np
import pytest
import torch

from tests import components_ref as ref

pytestmark = pytest.mark.gpu

V_EDGES = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097)
R_EDGES = (1, 33, 64, 65, 130)                                        # the table has ceil(R / 64) words per vertex
BYTES = np.array([1, 2, 255], np.uint8)
RULES = ((1, 0.0), (2, 0.0), (5, 0.25), (1, 0.5), (1, 1.0))           # (min_vertices, min_share)


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).cuda()


def make_masks(rng, r, v, densities=(0.15, 0.5, 0.9)):
    """set bytes of 1, 2 and 255; from three rows on, row 1 is empty and the last row all set"""
    on = rng.random((r, v)) < rng.choice(densities, size=(r, 1))
    m = (BYTES[rng.integers(0, 3, size=(r, v))] * on).astype(np.uint8)
    if r >= 3:
        m[1] = 0
        m[-1] = BYTES[rng.integers(0, 3, size=v)]
    return m


def make_mesh(rng, v):
    """a strip over a shuffled order with four faces in ten left out, long-range faces, duplicate and degenerate faces, and ends outside
    [0, v), negative ones and the extremes of int32 among them -- passed straight to the library"""
    o = rng.permutation(v)
    f = [np.stack((o[:-2], o[1:-1], o[2:]), axis=1)[rng.random(v - 2) < 0.6]] if v > 2 else []
    f.append(rng.integers(0, v, size=(v // 4 + 3, 3)))
    f.append(rng.integers(-3, v + 3, size=(7, 3)))
    f.append(np.array([[0, 0, 0], [v, 0, v - 1], [-(1 << 31), 0, (1 << 31) - 1], [v - 1, -1, 0]]))
    f = np.concatenate(f)
    f = np.concatenate((f, f[:5]))
    return f[rng.permutation(f.shape[0])].astype(np.int32)


def path_faces(order):
    """one degenerate face (a, b, b) per edge of the path through `order`: exactly those edges"""
    order = np.asarray(order)
    return np.stack((order[:-1], order[1:], order[1:]), axis=1).astype(np.int32)


def components(masks, faces, **kw):
    from gspn_amd.components import mask_components
    got = mask_components(dev(masks), dev(faces, np.int32).reshape(-1, 3), **kw)
    assert [t.dtype for t in got] == [torch.int32] * 3 and got[0].shape == masks.shape and got[1].shape == got[2].shape == masks.shape[:1]
    return tuple(t.cpu().numpy() for t in got)


def filtered(masks, faces, min_vertices, min_share, **kw):
    from gspn_amd.components import component_filter
    got = component_filter(dev(masks), dev(faces, np.int32).reshape(-1, 3), min_vertices=min_vertices, min_share=min_share, **kw)
    assert [t.dtype for t in got] == [torch.uint8] + [torch.int32] * 3 and got[0].shape == masks.shape
    return tuple(t.cpu().numpy() for t in got)


def same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:5].tolist())


def check(masks, faces, what, rules=RULES):
    """both ops against the restatement; ncomp >= 0 everywhere"""
    got = components(masks, faces)
    assert (got[1] >= 0).all(), what
    same(got, ref.mask_components_ref(masks, faces), what)
    for mv, share in rules:
        out = filtered(masks, faces, mv, share)
        assert (out[2] >= 0).all() and np.array_equal(out[2], got[1]), what
        same(out, ref.component_filter_ref(masks, faces, mv, share), "%s filter(%d, %r)" % (what, mv, share))
    return got


# ---- the sizes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", V_EDGES)
def test_both_ops_equal_the_restatement_at_the_vector_and_word_edges(v):
    rng = np.random.default_rng(1000 + v)
    faces = make_mesh(rng, v)
    for r in R_EDGES:
        check(make_masks(rng, r, v), faces, "R %d V %d" % (r, v), rules=RULES if r in (1, 65) else RULES[2:4])


@pytest.mark.parametrize("r", (33, 130))
def test_an_odd_vertex_count_near_20000(r):
    rng = np.random.default_rng(7 + r)
    v = 20001
    got = check(make_masks(rng, r, v, densities=(0.05, 0.3, 0.6)), make_mesh(rng, v), "R %d V %d" % (r, v), rules=RULES[2:4])
    assert got[1].max() > 100 and got[2].max() > 100                  # many components, and large ones


def test_no_faces_every_set_vertex_is_its_own_component():
    rng = np.random.default_rng(3)
    masks = make_masks(rng, 5, 1000)
    none = np.zeros((0, 3), np.int32)
    comp, ncomp, largest = check(masks, none, "F = 0")
    assert np.array_equal(comp, np.where(masks != 0, np.arange(1000), -1)) and np.array_equal(ncomp, (masks != 0).sum(1))
    assert largest.tolist() == [1, 0, 1, 1, 1]
    out, points, _, nkept = filtered(masks, none, 2, 0.0)             # nothing has two vertices
    assert not out.any() and not points.any() and not nkept.any()
    # faces that name no edge at all: the same
    same(components(masks, np.array([[5, 5, 5], [-1, 2000, 1000], [3, -4, 3]], np.int32)), (comp, ncomp, largest), "faces without an edge")


# ---- the shapes of the graph -----------------------------------------------------------------------------------------------------------------
def test_a_path_through_5000_vertices_in_shuffled_order():
    """one component with the deepest trees and many failed compare-and-swaps; in row 1 every 100th vertex of the path is unset, which
    cuts it in 50 pieces of 99; rows 0 and 1 overlap on their vertices with different components in each"""
    rng = np.random.default_rng(11)
    v = 5003
    order = rng.permutation(5000)                                     # vertices 5000..5002 are on no edge
    faces = path_faces(order)
    faces = faces[rng.permutation(faces.shape[0])]
    masks = np.zeros((3, v), np.uint8)
    masks[0] = 1
    masks[1] = 1
    masks[1, order[99::100]] = 0
    masks[2, order[:2500]] = 255
    comp, ncomp, largest = check(masks, faces, "shuffled path")
    assert ncomp.tolist() == [1 + 3, 50 + 3, 1] and largest.tolist() == [5000, 99, 2500]
    assert (comp[0, :5000] == 0).all() and comp[0, 5000:].tolist() == [5000, 5001, 5002]
    sizes = np.bincount(comp[1][comp[1] >= 0])
    assert sorted(sizes[sizes > 0].tolist()) == [1] * 3 + [99] * 50
    assert comp[2, order[:2500]].tolist() == [order[:2500].min()] * 2500


def test_paths_in_descending_and_ascending_index_order_and_stars():
    v = 6000
    down = path_faces(np.arange(v - 1, -1, -1))                       # the faces listed from the top down
    up = path_faces(np.arange(v))
    star_low = np.stack((np.zeros(v - 1), np.arange(1, v), np.arange(1, v)), axis=1).astype(np.int32)          # the centre is the root
    star_high = np.stack((np.full(v - 1, v - 1), np.arange(v - 1), np.arange(v - 1)), axis=1).astype(np.int32)  # the centre is the largest index
    masks = np.ones((2, v), np.uint8)
    masks[1, 3000] = 0
    for name, faces in (("descending path", down), ("ascending path", up)):
        comp, ncomp, largest = check(masks, faces, name, rules=RULES[3:])
        assert ncomp.tolist() == [1, 2] and largest.tolist() == [v, 3000] and (comp[0] == 0).all()
        assert (comp[1, :3000] == 0).all() and (comp[1, 3001:] == 3001).all()
    comp, ncomp, largest = check(masks, star_low, "star, centre 0", rules=RULES[3:])
    assert ncomp.tolist() == [1, 1] and largest.tolist() == [v, v - 1] and (comp[0] == 0).all()
    masks[1, 3000], masks[1, v - 1] = 1, 0                            # without its centre the star falls apart
    comp, ncomp, largest = check(masks, star_high, "star, centre V - 1", rules=RULES[3:])
    assert ncomp.tolist() == [1, v - 1] and largest.tolist() == [v, 1] and (comp[0] == 0).all()


def test_two_regions_that_touch_only_through_an_unset_vertex_are_separate():
    faces = np.array([[0, 1, 2], [2, 3, 3], [3, 3, 4], [4, 5, 5], [7, 7, 7], [9, 5, 9]], np.int32)
    masks = np.array([[1, 1, 1, 0, 1, 1, 0, 1], [1, 1, 1, 9, 1, 1, 0, 0], [0] * 8], np.uint8)
    comp, ncomp, largest = check(masks, faces, "through an unset vertex")
    assert comp.tolist() == [[0, 0, 0, -1, 4, 4, -1, 7], [0, 0, 0, 0, 0, 0, -1, -1], [-1] * 8]
    assert ncomp.tolist() == [3, 1, 0] and largest.tolist() == [3, 6, 0]
    # a whole triangle has the edge {a, c}: 2 and 4 are joined past an unset 3
    assert components(masks[:1], np.array([[2, 3, 4]], np.int32))[0].tolist() == [[0, 1, 2, -1, 2, 5, -1, 7]]


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def pieces(sizes, gap=1):
    """paths of the given vertex counts one behind the other, `gap` unset vertices between them -> row (V,) uint8, faces"""
    row, faces, at = [], [], 0
    for s in sizes:
        faces.append(path_faces(np.arange(at, at + s)))
        row += [1] * s + [0] * gap
        at += s + gap
    return np.array(row, np.uint8), np.concatenate(faces)


def test_the_keep_rule_at_its_edges():
    row, faces = pieces([6, 3, 2, 6, 1, 4])
    v = row.shape[0]
    masks = np.stack((row, np.zeros(v, np.uint8), row * 255, (row * 7).astype(np.uint8)))
    masks[2, 7:] = 0                                                  # row 2: the first 6 alone
    starts = np.flatnonzero(np.diff(np.concatenate(([0], row))) == 1)

    def kept_sizes(mv, share, k=0):
        out, points, ncomp, nkept = filtered(masks, faces, mv, share)
        same((out, points, ncomp, nkept), ref.component_filter_ref(masks, faces, mv, share), "rule (%d, %r)" % (mv, share))
        assert ncomp.tolist() == [6, 0, 1, 6] and points[1] == nkept[1] == 0 and not out[1].any()          # the empty row
        assert set(np.unique(out).tolist()) <= {0, 1} and np.array_equal(out[3], out[0])                  # any nonzero byte is set
        assert nkept[k] == out[k][starts].sum() and points[k] == out[k].sum()
        return [s for s, at in zip([6, 3, 2, 6, 1, 4], starts) if out[k, at]]

    assert kept_sizes(3, 0.0) == [6, 3, 6, 4]                         # a size equal to min_vertices is kept
    assert kept_sizes(4, 0.0) == [6, 6, 4]                            # one less is dropped
    assert kept_sizes(1, 0.5) == [6, 3, 6, 4]                         # s = 3, largest = 6, min_share = 0.5: kept, the compare is not strict
    assert kept_sizes(1, 0.5000000000000001) == [6, 6, 4]
    assert kept_sizes(1, 1.0) == [6, 6]                               # ties for the largest are all kept
    assert kept_sizes(7, 0.0) == [] and kept_sizes(1, 1.0, k=2) == [6]
    assert kept_sizes(1, 0.0) == [6, 3, 2, 6, 1, 4]                   # the identity ...
    assert np.array_equal(filtered(masks, faces, 1, 0.0)[0], (masks != 0).astype(np.uint8))              # ... up to the normalisation
    assert kept_sizes(5, 2.0 / 3.0) == [6, 6] and kept_sizes(1, 2.0 / 3.0) == ([6, 6, 4] if 4.0 >= 2.0 / 3.0 * 6.0 else [6, 6])


def case(r=41, v=4099, seed=7):
    rng = np.random.default_rng(seed)
    return make_masks(rng, r, v), make_mesh(np.random.default_rng(99), v)          # one mesh, masks by the seed


def test_out_may_be_masks():
    from gspn_amd.components import component_filter
    masks, faces = case()
    want = ref.component_filter_ref(masks, faces, 3, 0.3)
    m, f = dev(masks), dev(faces)
    out, points, ncomp, nkept = component_filter(m, f, min_vertices=3, min_share=0.3, out=m)
    assert out.data_ptr() == m.data_ptr()
    same(tuple(t.cpu().numpy() for t in (out, points, ncomp, nkept)), want, "in place")
    assert not np.array_equal(want[0], (masks != 0).astype(np.uint8))  # the case drops something
    other = torch.full_like(m, 77)
    out = component_filter(dev(masks), f, min_vertices=3, min_share=0.3, out=other)[0]
    assert out.data_ptr() == other.data_ptr() and np.array_equal(other.cpu().numpy(), want[0])           # every byte written


# ---- the library's behaviour ---------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits():
    masks, faces = case(seed=8)
    a, b = components(masks, faces), components(masks, faces)
    same(a, b, "components twice")
    same(filtered(masks, faces, 4, 0.2), filtered(masks, faces, 4, 0.2), "filter twice")


def test_the_workspace_need_not_be_initialised_and_must_be_large_enough():
    from gspn_amd import _lib
    from gspn_amd.components import component_filter, mask_components
    masks, faces = case(seed=9)
    r, v = masks.shape
    m, f = dev(masks), dev(faces)
    need_c = int(_lib.lib().gspn_mask_components_ws_bytes(r, v, faces.shape[0]))
    need_f = int(_lib.lib().gspn_mask_component_filter_ws_bytes(r, v, faces.shape[0]))
    want_c, want_f = ref.mask_components_ref(masks, faces), ref.component_filter_ref(masks, faces, 4, 0.2)
    for poison in (0xFF, 0x00, 0x5A):
        ws = torch.full((need_f + 64,), poison, dtype=torch.uint8, device="cuda")
        same(tuple(t.cpu().numpy() for t in mask_components(m, f, ws=ws[:need_c])), want_c, "components, ws of %#x" % poison)
        ws.fill_(poison)
        same(tuple(t.cpu().numpy() for t in component_filter(m, f, min_vertices=4, min_share=0.2, ws=ws)), want_f, "filter, ws of %#x" % poison)
        assert (ws[need_f:] == poison).all()                          # nothing is written behind what the call asked for
    ws = torch.zeros((need_f + 64,), dtype=torch.uint8, device="cuda")
    for bad in (ws[:need_c - 1], ws[8:], ws[::2], ws.cpu()):
        with pytest.raises(ValueError, match="ws must be"):
            mask_components(m, f, ws=bad)
    for bad in (ws[:need_f - 1], ws[8:], ws[::2]):
        with pytest.raises(ValueError, match="ws must be"):
            component_filter(m, f, min_vertices=4, ws=bad)


def test_the_calls_capture_with_a_caller_owned_workspace():
    from gspn_amd import _lib
    from gspn_amd.components import component_filter, mask_components
    inputs = [case(seed=20 + k)[0] for k in range(3)]
    faces = case()[1]
    r, v = inputs[0].shape
    m, f = dev(inputs[0]), dev(faces)
    ws_c = torch.empty((int(_lib.lib().gspn_mask_components_ws_bytes(r, v, faces.shape[0])),), dtype=torch.uint8, device="cuda")
    ws_f = torch.empty((int(_lib.lib().gspn_mask_component_filter_ws_bytes(r, v, faces.shape[0])),), dtype=torch.uint8, device="cuda")
    mask_components(m, f, ws=ws_c)                                     # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got_c = mask_components(m, f, ws=ws_c)
        got_f = component_filter(m, f, min_vertices=3, min_share=0.25, ws=ws_f)
    for nm in inputs[1:]:
        m.copy_(torch.from_numpy(nm))
        graph.replay()
        torch.cuda.synchronize()
        same(tuple(t.cpu().numpy() for t in got_c), ref.mask_components_ref(nm, faces), "replay, components")
        same(tuple(t.cpu().numpy() for t in got_f), ref.component_filter_ref(nm, faces, 3, 0.25), "replay, filter")


# ---- rows beyond 2^31 ------------------------------------------------------------------------------------------------------------------------
def test_row_offsets_are_64_bit():
    """129 rows of 2^24 vertices: row 128 starts at byte 2^31 of the masks and at element 2^31 of comp.  All rows are empty but the first
    and the last, which carry strips [lo, hi) -- each a path, so one component of hi - lo vertices whose smallest is lo --: at the row's two
    ends, two that touch without an edge between them, a single vertex, and in row 128 one that row 0 does not have.  About 20 GB with
    the workspace, none of which reaches the host."""
    from gspn_amd.components import component_filter, mask_components
    r, v = 129, 1 << 24
    strips = {0: [(0, 1500), (4000, 4003), (70000, 70100), (70100, 70300), (9999999, 10000000), (v - 2500, v)],
              128: [(0, 1000), (4000, 4003), (70000, 70100), (70100, 70300), (5000000, 5003000), (v - 2000, v)]}
    every = sorted({s for rows in strips.values() for s in rows})
    faces = np.concatenate([path_faces(np.arange(lo, hi)) for lo, hi in every if hi - lo > 1])
    faces = dev(faces[np.random.default_rng(5).permutation(faces.shape[0])])
    masks = torch.zeros((r, v), dtype=torch.uint8, device="cuda")
    want = {k: torch.full((v,), -1, dtype=torch.int32, device="cuda") for k in strips}
    for k, rows in strips.items():
        for j, (lo, hi) in enumerate(rows):
            masks[k, lo:hi] = int(BYTES[j % 3])
            want[k][lo:hi] = lo
    comp, ncomp, largest = mask_components(masks, faces)
    assert ncomp.tolist() == [6] + [0] * 127 + [6] and largest.tolist() == [2500] + [0] * 127 + [3000]
    for k in strips:
        assert torch.equal(comp[k], want[k]), k
    for j in range(1, 128, 16):
        assert bool((comp[j:min(j + 16, 128)] == -1).all()), j
    del comp
    out, points, ncomp, nkept = component_filter(masks, faces, min_vertices=100, min_share=0.5, out=masks)        # in place
    assert out.data_ptr() == masks.data_ptr() and ncomp.tolist() == [6] + [0] * 127 + [6]
    assert nkept.tolist() == [2] + [0] * 127 + [2] and points.tolist() == [1500 + 2500] + [0] * 127 + [3000 + 2000]
    keep = {0: [(0, 1500), (v - 2500, v)], 128: [(5000000, 5003000), (v - 2000, v)]}
    for k, rows in keep.items():
        w = torch.zeros((v,), dtype=torch.uint8, device="cuda")
        for lo, hi in rows:
            w[lo:hi] = 1
        assert torch.equal(out[k], w), k
    assert not bool(out[1:128].any())


# ---- declines --------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_decline_with_device_pointers_and_leave_the_outputs_alone():
    from gspn_amd import _lib
    lib = _lib.lib()
    masks, faces = case(r=3, v=100)
    m, f = dev(masks), dev(faces)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    comp = torch.full((3, 100), 77, dtype=torch.int32, device="cuda")
    n, big = torch.full((3,), 77, dtype=torch.int32, device="cuda"), torch.full((3,), 77, dtype=torch.int32, device="cuda")
    out = torch.full((3, 100), 77, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                       # noqa: E731
    st = _lib.stream()
    assert lib.gspn_mask_components(3, 100, faces.shape[0], p(m), p(f), ctypes.c_void_p(ws.data_ptr() + 8), p(comp), p(n), p(big), st) == -2
    assert lib.gspn_mask_components(1025, 100, faces.shape[0], p(m), p(f), p(ws), p(comp), p(n), p(big), st) == -2
    assert lib.gspn_mask_component_filter(3, 100, faces.shape[0], p(m), p(f), 0, 0.5, p(ws), p(out), p(n), p(big), p(n), st) == -1
    assert lib.gspn_mask_component_filter(3, 100, faces.shape[0], p(m), p(f), 1, float("nan"), p(ws), p(out), p(n), p(big), p(n), st) == -1
    assert lib.gspn_mask_component_filter(3, 100, faces.shape[0], p(m), p(f), 1, 1.5, p(ws), p(out), p(n), p(big), p(n), st) == -1
    assert lib.gspn_mask_components(0, 100, 5, p(m), p(f), p(ws), p(comp), p(n), p(big), st) == 0              # nothing to do, nothing written
    assert lib.gspn_mask_component_filter(3, 0, 5, p(m), p(f), 1, 0.5, p(ws), p(out), p(n), p(big), p(n), st) == 0
    torch.cuda.synchronize()
    assert (comp == 77).all() and (n == 77).all() and (big == 77).all() and (out == 77).all() and not ws.any()


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------------------
def test_the_stage_drops_islands_that_cost_ap50():
    """6 synth.scan_faces instances, two to each of three classes.  Row i is instance i plus seven islands of vertices from other
    instances; an island is grown from a seeded vertex over the mesh's edges inside one instance, so it is connected, the islands of a
    row share no vertex, and each -- two that touch included -- is smaller than half the instance, but together they outweigh it: the row's IoU with its instance is below 0.5, and every
    prediction is a false positive at AP50.  Behind component_filter(min_vertices=1, min_share=0.5) every row is its instance, and
    AP, AP50 and AP25 are exactly 1 (two instances a class: the recall steps 0.5 and 1 are exact in binary)."""
    from gspn_amd import synth
    from gspn_amd.components import component_filter
    from gspn_amd.evaluate import MIN_REGION_SIZE, InstanceAP
    rng = np.random.default_rng(12)
    n_ins, per, islands, isle = 6, 700, 7, 120                        # 7 * 120 = 840 > 700, 2 * 120 < 350
    centres = np.array([[2.0 * g, 0.0, 0.0] for g in range(n_ins)], np.float32)
    xyz = np.concatenate([centres[g] + rng.random((per, 3), dtype=np.float32) for g in range(n_ins)])
    group = np.repeat(np.arange(n_ins), per).astype(np.int32)
    sem = (group // 2 + 1).astype(np.int32)                            # classes 1, 2 and 3, two instances each
    order = rng.permutation(xyz.shape[0])
    xyz, group, sem = xyz[order], group[order], sem[order]
    v = xyz.shape[0]
    faces = synth.scan_faces(xyz, sem, group, 0.5, seed=13)
    edges = ref.edges_ref(faces, v)
    assert np.bincount(group).min() >= MIN_REGION_SIZE

    def island(g, number, taken):
        """`isle` vertices of instance g outside `taken` that are connected among themselves: grown from a seeded vertex over the mesh's edges"""
        inside = (group == g) & ~taken
        nbr = {}
        for a, b in edges[inside[edges[:, 0]] & inside[edges[:, 1]]].tolist():
            nbr.setdefault(a, []).append(b)
            nbr.setdefault(b, []).append(a)
        start = int(np.flatnonzero(inside)[(97 * number) % int(inside.sum())])
        seen, todo = {start}, [start]
        while todo and len(seen) < isle:
            for w in nbr.get(todo.pop(0), ()):
                if w not in seen and len(seen) < isle:
                    seen.add(w)
                    todo.append(w)
        assert len(seen) == isle
        return sorted(seen)

    rows_ = []
    for g in range(n_ins):
        row = group == g
        mine = row.copy()
        others = [h for h in range(n_ins) if h != g]
        for j in range(islands):                                      # 7 islands over 5 other instances: two of them carry two, far apart
            row[island(others[j % len(others)], 3 * g + j + 40 * (j // len(others)), row & ~mine)] = True
        rows_.append(row)
    masks_np = np.stack(rows_).astype(np.uint8) * 255
    comp, ncomp, largest = ref.mask_components_ref(masks_np, faces)
    assert largest.tolist() == [per] * n_ins and (ncomp >= 1 + 5).all()                               # the instance is the largest piece of its row
    for g in range(n_ins):
        sizes = np.bincount(comp[g][comp[g] >= 0])
        assert np.sort(sizes[sizes > 0])[-2] < per / 2 and rows_[g].sum() - per == islands * isle > per  # every island below half, together above
    masks = torch.from_numpy(masks_np).cuda()
    cls = torch.arange(n_ins, dtype=torch.int32, device="cuda") // 2 + 1
    count = torch.tensor(n_ins, dtype=torch.int32, device="cuda")
    out, points, got_ncomp, nkept = component_filter(masks, dev(faces), min_vertices=1, min_share=0.5)
    same((out.cpu().numpy(), points.cpu().numpy(), got_ncomp.cpu().numpy(), nkept.cpu().numpy()), ref.component_filter_ref(masks_np, faces, 1, 0.5), "islands")
    assert nkept.tolist() == [1] * n_ins and points.tolist() == [per] * n_ins
    assert np.array_equal(out.cpu().numpy(), np.stack([group == g for g in range(n_ins)]).astype(np.uint8))

    def figures(m):
        metric = InstanceAP(4, label_map=None)
        conf = torch.linspace(0.9, 0.4, n_ins, device="cuda")[None]
        metric.add(m[None], cls[None], conf, count[None], torch.from_numpy(sem).cuda()[None], torch.from_numpy(group).cuda()[None], n_ins)
        res = metric.compute()
        return res["all_ap"], res["all_ap_50%"], res["all_ap_25%"]

    before, after = figures((masks != 0).to(torch.uint8)), figures(out)
    print("AP / AP50 / AP25: %.4f / %.4f / %.4f on the input rows, %.4f / %.4f / %.4f behind the filter" % (before + after))
    iou = [per / float(rows_[g].sum()) for g in range(n_ins)]
    assert max(iou) < 0.5 and before[1] == 0.0                        # the input rows miss AP50 on every instance
    assert after == (1.0, 1.0, 1.0)
