"""GPU tests of the address walk the per-vertex mask stages share (csrc/mask_rows.h): segment voting, mask NMS, mask components and mask
holes read, and the last three write, rows of V mask bytes in 16-byte chunks laid over the row's ADDRESS.  Rows set in exactly one byte
(for the holes: unset in exactly one), the byte put at each of the 16 positions of a chunk, in the head chunk, in full chunks and in the
tail chunk of rows at every misalignment; and out= at a misaligned base inside a poisoned buffer.  Every comparison is for equal bits,
against the numpy restatements of the four stages."""
import numpy as np
import pytest
import torch

from tests import components_ref, holes_ref, mask_nms_ref, segments_ref

pytestmark = pytest.mark.gpu

R = 16                                                                # rows k * V apart: V = 67 puts them at all 16 misalignments
BYTES = np.array([0, 1, 2, 255], np.uint8)
STAGES = ("segments", "mask_nms", "components", "holes")
PLACES = ("head", "inner", "late", "tail", "stairs")
POISON = 0xAB
NO_FACES = np.zeros((0, 3), np.int32)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


def one_byte_rows(v, place):
    """-> the device tensor (R, V) with one set byte per row, its host copy, the set vertex of each row and the position of that byte in
    its 16-byte chunk.  With a0 the address of row k modulo 16, chunk q of the row is its vertices [16 q - a0, 16 q - a0 + 16):
    head   vertex 0, at position a0 of chunk 0 (a ragged chunk unless a0 = 0)
    inner  position k of chunk 2, a full chunk
    late   position 15 - k of the last full chunk of the row
    tail   vertex V - 1, in the row's last chunk (ragged unless the row ends on a 16-byte boundary)
    stairs vertex 32 + k, whatever the address: no two rows share a vertex"""
    masks = torch.zeros((R, v), dtype=torch.uint8, device="cuda")
    a0 = (masks.data_ptr() + np.arange(R) * v) % 16
    k = np.arange(R)
    at = {"head": 0 * k, "inner": 32 - a0 + k, "late": 16 * ((v + a0) // 16 - 1) - a0 + 15 - k, "tail": 0 * k + v - 1, "stairs": 32 + k}[place]
    assert (at >= 0).all() and (at < v).all()
    host = np.zeros((R, v), np.uint8)
    host[k, at] = BYTES[1 + k % 3]
    masks.copy_(torch.from_numpy(host))
    return masks, host, at, (a0 + at) % 16


def path_mesh(v):
    """-> the path 0 - 1 - ... - V-1 as degenerate faces (a, b, b), and the vertices on a line, xyz[i] = (i, 0, 0)"""
    i = np.arange(v - 1)
    xyz = np.zeros((v, 3), np.float32)
    xyz[:, 0] = np.arange(v)
    return np.stack((i, i + 1, i + 1), axis=1).astype(np.int32), xyz


def test_the_rows_of_67_vertices_start_at_every_misalignment_and_the_places_cover_every_position():
    """the premise of the cases below, on the addresses the allocator really gives"""
    for place in PLACES[:4]:
        masks, host, at, position = one_byte_rows(67, place)
        assert sorted((masks.data_ptr() + np.arange(R) * 67) % 16) == list(range(16))
        assert sorted(position) == list(range(16)), place
        assert (host != 0).sum(1).tolist() == [1] * R
    for v in (64, 4099, 8200):
        for place in ("inner", "late"):
            assert sorted(one_byte_rows(v, place)[3]) == list(range(16)), (v, place)


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("v", (64, 67, 4099, 8200))
@pytest.mark.parametrize("stage", STAGES)
def test_a_vector_set_in_exactly_one_byte_at_each_of_its_positions(stage, v, place):
    masks, host, at, _ = one_byte_rows(v, place)
    rows, normal = np.arange(R), (host != 0).astype(np.uint8)
    apart = np.unique(at).size == R                                   # no two rows share their vertex ("stairs"; "inner" and "late" where the rows are aligned)
    if stage == "segments":
        from gspn_amd.segments import segment_vote
        rng = np.random.default_rng(4)
        for s, seg in ((v, np.arange(v)), (5, rng.integers(0, 5, size=v))):
            for th in (0.5, 0.0):
                out, points = segment_vote(masks, dev(seg, np.int32), s, th)
                want = segments_ref.segment_vote_ref(host, seg, s, th)
                assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(points.cpu().numpy(), want[1]), (s, th)
        out, points = segment_vote(masks, dev(np.arange(v), np.int32), v)             # singleton segments: the normalised input
        assert points.tolist() == [1] * R and np.array_equal(out.cpu().numpy(), normal)
    elif stage == "mask_nms":
        from gspn_amd.mask_nms import mask_nms, mask_overlaps
        sizes, inter = mask_overlaps(masks)
        want = mask_nms_ref.mask_overlaps_ref(host)
        assert sizes.tolist() == [1] * R and np.array_equal(sizes.cpu().numpy(), want[0]) and np.array_equal(inter.cpu().numpy(), want[1])
        if apart:
            assert np.array_equal(inter.cpu().numpy(), np.eye(R, dtype=np.int32))
        got = [t.cpu().numpy() for t in mask_nms(masks, iou_th=0.0)]
        want = mask_nms_ref.mask_nms_ref(host, iou_th=0.0)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        if apart:
            assert got[1].tolist() == [1] * R and np.array_equal(got[0], normal)
        host[:, v - 1] = 7                                            # now they all share the last vertex: at 0 one shared vertex suppresses
        got = [t.cpu().numpy() for t in mask_nms(dev(host), iou_th=0.0)]
        want = mask_nms_ref.mask_nms_ref(host, iou_th=0.0)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert got[1].tolist() == [1] + [0] * (R - 1) and got[2].tolist() == [2 if at[0] != v - 1 else 1] + [0] * (R - 1)
    elif stage == "holes":
        from gspn_amd.holes import hole_fill
        faces, xyz = path_mesh(v)
        mirror = BYTES[1 + (rows[:, None] + np.arange(v)[None, :]) % 3]              # the mirror case: every byte set but the one at the place
        mirror[rows, at] = 0
        masks.copy_(torch.from_numpy(mirror))                        # in place: the rows stay at the addresses the places were computed for
        got = [t.cpu().numpy() for t in hole_fill(masks, dev(faces), dev(xyz), max_vertices=1, label=True)]
        want = holes_ref.hole_fill_ref(mirror, faces, xyz, 1)
        assert len(got) == len(want) == 5 and all(np.array_equal(g, w) for g, w in zip(got, want))
        inner = ((at != 0) & (at != v - 1)).astype(np.int32)          # an unset end of the path lies outside the box of the set vertices: not filled
        assert np.array_equal(got[0][rows, at], inner) and np.array_equal(got[1], v - 1 + inner)
        assert np.array_equal(got[2], inner) and np.array_equal(got[3], inner)
        out, points, nholes, nfilled = hole_fill(masks, dev(faces), dev(xyz), max_vertices=0)           # the normalised input
        assert np.array_equal(out.cpu().numpy(), (mirror != 0).astype(np.uint8)) and points.tolist() == [v - 1] * R
        assert nholes.tolist() == nfilled.tolist() == [0] * R
    else:
        from gspn_amd.components import component_filter, mask_components
        comp, ncomp, largest = mask_components(masks, dev(NO_FACES))   # without faces a set vertex is its own component
        want = np.full((R, v), -1, np.int32)
        want[rows, at] = at
        assert np.array_equal(comp.cpu().numpy(), want) and ncomp.tolist() == [1] * R and largest.tolist() == [1] * R
        assert np.array_equal(want, components_ref.mask_components_ref(host, NO_FACES)[0])
        out, points, ncomp, nkept = component_filter(masks, dev(NO_FACES), min_vertices=1, min_share=0.0)      # the identity
        assert np.array_equal(out.cpu().numpy(), normal) and points.tolist() == [1] * R and ncomp.tolist() == nkept.tolist() == [1] * R


@pytest.mark.parametrize("offset", (1, 7, 15))
@pytest.mark.parametrize("v", (67, 4099))
@pytest.mark.parametrize("stage", STAGES)
def test_out_at_a_misaligned_base_is_written_in_full_and_nothing_around_it(stage, v, offset):
    """out is a view that starts `offset` bytes into a poisoned buffer; ws stays aligned (the ops allocate it).  Dense rows, so that every
    position of every chunk carries a bit."""
    rng = np.random.default_rng(100 * v + offset)
    host = (BYTES[rng.integers(1, 4, size=(R, v))] * (rng.random((R, v)) < 0.5)).astype(np.uint8)
    host[3], host[5] = 0, 255
    masks = dev(host)
    buf = torch.full((offset + R * v + 64,), POISON, dtype=torch.uint8, device="cuda")
    out = buf[offset:offset + R * v].view(R, v)
    assert out.data_ptr() % 16 == (buf.data_ptr() + offset) % 16 and out.is_contiguous()
    if stage == "segments":
        from gspn_amd.segments import segment_vote
        seg = rng.integers(0, 9, size=v)
        got = segment_vote(masks, dev(seg, np.int32), 9, out=out)
        want = segments_ref.segment_vote_ref(host, seg, 9)
    elif stage == "mask_nms":
        from gspn_amd.mask_nms import mask_nms
        got = mask_nms(masks, iou_th=0.3, out=out)
        want = mask_nms_ref.mask_nms_ref(host, iou_th=0.3)
        assert 0 < int(want[1].sum()) < R                             # suppressed rows, written as zeros, and kept ones
    elif stage == "holes":
        from gspn_amd.holes import hole_fill
        faces, xyz = path_mesh(v)
        got = hole_fill(masks, dev(faces), dev(xyz), max_vertices=3, out=out)
        want = holes_ref.hole_fill_ref(host, faces, xyz, 3)[:4]
        assert int(want[3].sum()) > 0 and int(want[0].sum()) < R * v  # filled vertices, and unset ones left
    else:
        from gspn_amd.components import component_filter
        faces = np.stack((np.arange(v - 2), np.arange(1, v - 1), np.arange(2, v)), axis=1).astype(np.int32)
        got = component_filter(masks, dev(faces), min_vertices=3, min_share=0.0, out=out)
        want = components_ref.component_filter_ref(host, faces, 3, 0.0)
        assert 0 < int(want[0].sum()) < int((host != 0).sum())        # dropped vertices and kept ones
    assert got[0].data_ptr() == out.data_ptr()
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    whole = buf.cpu().numpy()
    assert (whole[:offset] == POISON).all() and (whole[offset + R * v:] == POISON).all()
    assert np.array_equal(whole[offset:offset + R * v].reshape(R, v), want[0])
