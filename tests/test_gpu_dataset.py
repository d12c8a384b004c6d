"""GPU tests of gspn_amd/dataset.py on csrc/sampling_segments.hip: the segmented FPS equal to the CPU oracle run on every host-compacted
instance, in every size class of the kernels and on a lattice where ties are everywhere; the padded rows equal to the documented draws;
the same picks as the per-instance loop over farthest_point_sample; the error codes of the C entry point; a segment that is the whole scene equal to
the dense kernel, which runs the same round loop (csrc/fps_rounds.h), in every instantiation; the captured call; resample_scene
and augment_and_box against the numpy restatement (tests/dataset_ref.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import dataset_ref as DR

pytestmark = pytest.mark.gpu

N, G, M = 32768, 8, 64


def dev_seed(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


@functools.lru_cache(maxsize=None)
def scenes(lattice):
    """(pc (2, N, 3), label (2, N)) of the two scenes of DR.SIZES -- shared, never written"""
    both = [DR.labelled_scene(N, DR.SIZES[s], G, 40 + s, lattice) for s in range(2)]
    pc, label = np.stack([p for p, _ in both]), np.stack([l for _, l in both])
    pc.setflags(write=False)
    label.setflags(write=False)
    return pc, label


@functools.lru_cache(maxsize=None)
def expected(lattice, m, seed, nscene=2):
    pc, label = scenes(lattice)
    return DR.instance_sets(pc[:nscene], label[:nscene], G, m, seed)


def run(lattice, m, seed, nscene=2):
    from gspn_amd import dataset
    pc, label = scenes(lattice)
    pc, label = torch.from_numpy(pc[:nscene].copy()).cuda(), torch.from_numpy(label[:nscene].copy()).cuda()
    idx, pts, count = dataset.fps_segments(pc, label, G, m, seed)
    assert idx.dtype == torch.int32 and count.dtype == torch.int32 and pts.dtype == torch.float32
    assert idx.shape == (nscene, G, m) and pts.shape == (nscene, G, m, 3) and count.shape == (nscene, G)
    return pc, idx.cpu().numpy(), pts.cpu().numpy(), count.cpu().numpy()


def check_rows(pc, idx, pts, count, want):
    want_idx, want_pts, want_count = want
    assert np.array_equal(count, want_count)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(pts.view(np.int32), want_pts.view(np.int32))
    pc = pc.cpu().numpy()
    for s in range(idx.shape[0]):
        for j in range(G):
            if j == 0 or count[s, j] == 0:                      # the background and empty groups: -1 / zeros
                assert (idx[s, j] == -1).all() and not pts[s, j].view(np.int32).any()
            else:                                               # pts is pc[idx], bit for bit
                assert idx[s, j].min() >= 0
                assert np.array_equal(pts[s, j].view(np.int32), pc[s][idx[s, j]].view(np.int32))


# ---- 1. exact against the oracle, every size class ---------------------------------------------------------------------------------

@pytest.mark.parametrize("lattice", [False, True], ids=["cloud_d", "lattice"])
def test_fps_segments_equals_the_oracle_in_every_size_class(lattice):
    sizes = sorted(c for s in range(2) for j, c in enumerate(DR.SIZES[s]) if j > 0)
    for lo, hi in ((M, 512), (512, 1024), (1024, 1536), (1536, 2048), (2048, 4096), (4096, 8192), (8192, 16384), (16384, 32768)):
        assert any(lo < c <= hi for c in sizes), "no instance in size class (%d, %d]" % (lo, hi)
    assert M in sizes and 0 in sizes and any(0 < c < M for c in sizes)
    pc, idx, pts, count = run(lattice, M, 7)
    check_rows(pc, idx, pts, count, expected(lattice, M, 7))


# ---- 2. the reference's npoint_ins -------------------------------------------------------------------------------------------------

def test_fps_segments_at_the_default_npoint_ins():
    pc, idx, pts, count = run(False, 512, 7, nscene=1)
    check_rows(pc, idx, pts, count, expected(False, 512, 7, 1))


# ---- 3. padding --------------------------------------------------------------------------------------------------------------------

def test_padded_rows_follow_the_documented_draws():
    _, label = scenes(False)
    pc, idx, pts, count = run(False, M, 7)
    _, idx_again, pts_again, _ = run(False, M, 7)
    _, idx_other, _, _ = run(False, M, 8)
    assert np.array_equal(idx, idx_again) and np.array_equal(pts.view(np.int32), pts_again.view(np.int32))
    padded = 0
    for s in range(2):
        for j in range(1, G):
            c = int(count[s, j])
            if c == 0 or c >= M:
                assert np.array_equal(idx[s, j], idx_other[s, j])                  # another seed changes the padded tails only
                continue
            padded += 1
            members = np.nonzero(label[s] == j)[0]
            assert np.array_equal(idx[s, j, :c], members)
            assert np.array_equal(idx_other[s, j, :c], members)
            for seed, got in ((7, idx), (8, idx_other)):
                assert np.array_equal(got[s, j, c:], members[DR.padding_draws(seed, s, j, M - c, c)])
            assert not np.array_equal(idx[s, j, c:], idx_other[s, j, c:])
    assert padded >= 1


# ---- 4. against the loop the library offered before --------------------------------------------------------------------------------

def test_instance_point_sets_equals_the_per_instance_loop():
    from gspn_amd import dataset
    from gspn_amd.tf_sampling import farthest_point_sample
    pc_np, label_np = scenes(False)
    pc, label = torch.from_numpy(pc_np.copy()).cuda(), torch.from_numpy(label_np.copy()).cuda()
    pc_ins = dataset.instance_point_sets(pc, label, G, M, 7)
    assert pc_ins.shape == (2, G, M, 3)
    compared = 0
    for s in range(2):
        for j in range(1, G):
            pts = pc[s][label[s] == j]
            if pts.shape[0] < M:
                continue
            pick = farthest_point_sample(M, pts[None])[0].long()
            if pts.shape[0] == M:
                # the reference copies such an instance in its own order (:114-115) and so does instance_point_sets; the loop's FPS of all
                # M points visits the same coordinates in another order
                assert torch.equal(pc_ins[s, j], pts) and torch.equal(torch.unique(pts[pick], dim=0), torch.unique(pts, dim=0))
            else:
                assert torch.equal(pc_ins[s, j], pts[pick])
            compared += 1
    assert compared == 11


# ---- 5. the C entry point alone ----------------------------------------------------------------------------------------------------

def test_abi_error_codes_and_the_empty_batch():
    from gspn_amd import _lib as L
    lib = L.lib()
    assert lib.gspn_fps_segments_ws_bytes(2, 32769, 8) == -2 and lib.gspn_fps_segments_ws_bytes(2, 0, 8) == -1
    null = ctypes.c_void_p(0)
    # null pointers throughout: a launch would fault, an error code proves there was none
    assert lib.gspn_fps_segments(2, 32769, 8, 64, null, null, null, null, null, null, null, null, L.stream()) == -2
    assert lib.gspn_fps_segments(2, 4096, 8, 0, null, null, null, null, null, null, null, null, L.stream()) == -1
    assert lib.gspn_fps_segments(0, 4096, 8, 64, null, null, null, null, null, null, null, null, L.stream()) == 0
    b, n, g, m = 1, 700, 3, 16
    rng = np.random.default_rng(3)
    pc = torch.from_numpy(rng.random((b, n, 3), dtype=np.float32)).cuda()
    label = torch.from_numpy(rng.integers(0, g, (b, n)).astype(np.int32)).cuda()
    from gspn_amd import invlists
    order, offsets = invlists.inverse_lists(label, g)
    ws_bytes = int(lib.gspn_fps_segments_ws_bytes(b, n, g))
    assert ws_bytes >= 0
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    idx = torch.empty((b, g, m), dtype=torch.int32, device="cuda")
    pts = torch.empty((b, g, m, 3), dtype=torch.float32, device="cuda")
    count = torch.empty((b, g), dtype=torch.int32, device="cuda")
    rc = lib.gspn_fps_segments(b, n, g, m, L.ptr(dev_seed(0)), L.ptr(pc), L.ptr(order), L.ptr(offsets), L.ptr(ws), L.ptr(idx), L.ptr(pts),
                               L.ptr(count), L.stream())
    assert rc == 0
    want = DR.instance_sets(pc.cpu().numpy(), label.cpu().numpy(), g, m, 0)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[2])
    assert np.array_equal(pts.cpu().numpy().view(np.int32), want[1].view(np.int32))


# ---- 5b. one round loop, two callers: a segment that is the whole scene against the dense kernel ------------------------------------

def tie_cloud(n):
    """n points on the 1/8 lattice of [0, 2)^3 (distances exact in float32), a quarter of them exact duplicates of other points"""
    rng = np.random.default_rng(n)
    pc = (rng.integers(0, 16, (n, 3)) * 0.125).astype(np.float32)
    dst = rng.permutation(n)[:n // 4]
    pc[dst] = pc[rng.integers(0, n, n // 4)]
    return pc


def rounds_with_a_tied_maximum(pc, picks):
    """replays the oracle's picks on exact coordinates: the rounds whose largest min-distance is held by more than one point"""
    p = pc.astype(np.float64)
    td = np.full(len(p), np.inf)
    tied = 0
    for j in range(1, len(picks)):
        td = np.minimum(td, ((p - p[picks[j - 1]]) ** 2).sum(1))
        assert td[picks[j]] == td.max() > 0
        tied += int((td == td.max()).sum() > 1)
    return tied


# 300 ... 2048: fps_small C = 1, 2, 3, 4; 2049, 4097, 8193: fps_resident P = 4, 8, 16; 16385: P = 32 with the z plane in LDS
@pytest.mark.parametrize("n,ties", [(300, False), (1024, False), (1536, False), (2048, False), (2049, False), (4097, False), (8193, False),
                                    (16385, False), (1536, True), (4097, True)])
def test_a_whole_scene_segment_equals_the_dense_kernel(n, ties):
    from gspn_amd import _lib as L
    from gspn_amd import synth
    from oracle import oracle as O
    lib = L.lib()
    g, m = 2, 64
    pc_np = tie_cloud(n) if ties else synth.cloud_d(n, n)
    if ties:
        want = O.farthest_point_sample(m, pc_np[None])[0]
        assert rounds_with_a_tied_maximum(pc_np, want) >= 1
    pc = torch.from_numpy(pc_np).cuda()[None].contiguous()
    order = torch.arange(n, dtype=torch.int32, device="cuda")[None].contiguous()      # every label is 1: group 1 is the scene, in order
    offsets = torch.tensor([[0, 0, n]], dtype=torch.int32, device="cuda")
    idx = torch.full((1, g, m), -7, dtype=torch.int32, device="cuda")
    pts = torch.full((1, g, m, 3), -7.0, dtype=torch.float32, device="cuda")
    count = torch.full((1, g), -7, dtype=torch.int32, device="cuda")
    dense = torch.full((1, m), -7, dtype=torch.int32, device="cuda")
    assert lib.gspn_fps_segments(1, n, g, m, L.ptr(dev_seed(0)), L.ptr(pc), L.ptr(order), L.ptr(offsets), L.ptr(None), L.ptr(idx), L.ptr(pts),
                                 L.ptr(count), L.stream()) == 0
    assert lib.gspn_farthestpointsampling(1, n, m, L.ptr(pc), L.ptr(None), L.ptr(dense), L.stream()) == 0       # no workspace: small / resident
    assert count.cpu().tolist() == [[0, n]]
    assert torch.equal(idx[0, 1], dense[0])
    assert torch.equal(pts[0, 1], pc[0][dense[0].long()])
    if ties:
        assert np.array_equal(dense[0].cpu().numpy(), want)


# ---- 6. captured -------------------------------------------------------------------------------------------------------------------

def test_instance_point_sets_captured_draws_afresh_on_replay():
    from gspn_amd import dataset, graph
    pc_np, label_np = scenes(False)
    pc, label = torch.from_numpy(pc_np.copy()).cuda(), torch.from_numpy(label_np.copy()).cuda()
    seed = dev_seed(7)
    step = graph.CapturedStep(lambda: dataset.instance_point_sets(pc, label, G, M, seed))
    first = step.replay().clone()
    seed += 1
    second = step.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(first, dataset.instance_point_sets(pc, label, G, M, 7))
    assert torch.equal(second, dataset.instance_point_sets(pc, label, G, M, 8))
    _, want7, count = expected(False, M, 7)
    assert np.array_equal(first.cpu().numpy().view(np.int32), want7.view(np.int32))
    for s in range(2):
        for j in range(1, G):
            if 0 < count[s, j] < M:
                assert not torch.equal(first[s, j], second[s, j])                  # padded tails are new ...
                assert torch.equal(first[s, j, :count[s, j]], second[s, j, :count[s, j]])
            else:
                assert torch.equal(first[s, j], second[s, j])                      # ... FPS rows are not


# ---- 7. resample_scene -------------------------------------------------------------------------------------------------------------

def scan(b, n, seed):
    from gspn_amd import synth
    rng = np.random.default_rng(seed)
    pc = synth.batch("D", b, n, seed)
    return pc, rng.random((b, n, 3), dtype=np.float32), rng.integers(0, 9, (b, n)), rng.integers(0, 19, (b, n))


@pytest.mark.parametrize("n,npoint", [(4096, 1024), (1024, 1024), (1000, 1024)])
def test_resample_scene(n, npoint):
    from gspn_amd import dataset
    b, seed = 2, 11
    arrays = scan(b, n, 5)
    got = dataset.resample_scene(*(torch.from_numpy(a).cuda() for a in arrays), npoint, seed)
    for s in range(b):
        choice = DR.resample_choice(arrays[0][s], npoint, seed, s)
        assert len(choice) == npoint and choice.min() >= 0 and choice.max() < n
        if n <= npoint:
            assert np.array_equal(choice[:n], np.arange(n))                        # order kept, duplicates behind
        for a, t in zip(arrays, got):
            assert t.shape[1] == npoint and np.array_equal(t[s].cpu().numpy(), a[s][choice])


# ---- 8. augment_and_box ------------------------------------------------------------------------------------------------------------

def within_one_ulp(got, want):
    """got == want, or its float32 neighbour on either side; returns the number of elements that are not bit-equal"""
    ok = (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    assert ok.all()
    return int((got != want).sum())


def test_augment_and_box_against_the_float64_restatement():
    from gspn_amd import dataset
    b, n, g, m = 2, 2048, 6, 32
    rng = np.random.default_rng(21)
    pc = (rng.random((b, n, 3), dtype=np.float32) * np.float32(8.0))
    pc_ins = (rng.random((b, g, m, 3), dtype=np.float32) * np.float32(8.0))
    pc_ins[:, 0] = 0
    pc_ins[1, 4:] = 0
    valid = np.array([6, 4])
    angle = rng.uniform(size=b) * 2 * np.pi
    rot = np.stack([np.array([[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1]]) for a in angle])
    trans = rng.normal(0, 1, (b, 3))
    got_pc, got_ins, got_ind, got_box = dataset.augment_and_box(torch.from_numpy(pc).cuda(), torch.from_numpy(pc_ins).cuda(),
                                                                torch.from_numpy(valid).cuda(), torch.from_numpy(rot), torch.from_numpy(trans))
    got_pc, got_ins, got_box = got_pc.cpu().numpy(), got_ins.cpu().numpy(), got_box.cpu().numpy()
    want_pc = np.stack([DR.rigid(pc[s], rot[s], trans[s]) for s in range(b)])
    want_ins = np.stack([DR.rigid(pc_ins[s], rot[s], trans[s]) for s in range(b)])
    print("augment_and_box: %d of %d pc and %d of %d pc_ins values one float32 step from numpy's"
          % (within_one_ulp(got_pc, want_pc), want_pc.size, within_one_ulp(got_ins, want_ins), want_ins.size))
    assert np.array_equal(got_box, DR.boxes(got_ins))                                     # the restatement on OUR pc_ins
    assert got_ind.dtype == torch.int32 and np.array_equal(got_ind.cpu().numpy(), DR.group_indicator(valid, g))
    # drawn on the host from the seed: the same seed repeats, the indicator takes an int too
    a = dataset.augment_and_box(torch.from_numpy(pc).cuda(), torch.from_numpy(pc_ins).cuda(), 4, seed=5)
    a2 = dataset.augment_and_box(torch.from_numpy(pc).cuda(), torch.from_numpy(pc_ins).cuda(), 4, seed=dev_seed(5))
    assert all(torch.equal(x, y) for x, y in zip(a, a2))
    assert a[2].cpu().tolist() == [[1, 1, 1, 1, 0, 0]] * 2
    assert np.array_equal(a[3].cpu().numpy(), DR.boxes(a[1].cpu().numpy()))
