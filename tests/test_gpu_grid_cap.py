"""Every kernel launched through a capped grid, at a size just past the cap: some threads take a second trip through the grid-stride loop,
their neighbours leave after the first, and the last workgroup is ragged.

grid_for() (csrc/common.h) caps a launch at G workgroups; below G * B items every thread runs its loop body once, and the stride update,
the partially filled second trip and the loop-carried locals are code the rest of the suite never executes.  Each case here asks the
library itself (gspn_grid_blocks) for the grid of its launch and asserts G * B < T < 2 * G * B and T % B != 0 before anything runs, T being
the launcher's own item count (vectors for a 4-wide kernel): a later change of the cap fails the assertion, by name, instead of quietly
turning the case back into a one-trip test.  SHAPES holds every case's (T, B); tests/test_cpu_grid_cap.py asserts the same condition without
a GPU and holds COVERED against the launch sites of csrc/*.hip.

Every pure output starts as a sentinel (NaN, 0x7FC0DEAD), workspaces start as garbage, in-place updates run exactly as often as their
reference, and a mismatch is reported separately for what the first trip [0, G * B) and the second trip [G * B, T) wrote.  References and
tolerances are those of each op's existing test: the C oracle, the *_ref.py restatements, float64 torch; where a restatement is a Python
loop over the items it is replaced by a vectorised numpy form of the same definition, and the case says so.

COVERED: kernel -> the case of this file that takes it past the cap, or the existing test that already does with its shape and T."""
import ctypes
import math
import os
import re
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gspn_amd", "csrc")

COVERED = {
    # csrc/optim.hip, csrc/train.hip
    "adam_flat_kernel": "test_flat_optimisers[adam_flat]",
    "adam_flat_dev_kernel": "test_flat_optimisers[adam_flat_dev]",
    "adam_tf_flat_kernel": "test_flat_optimisers[adam_tf_flat]",
    "momentum_flat_kernel": "test_flat_optimisers[momentum_flat]",
    # csrc/grouping.hip
    "group_point_kernel": "test_group_point_and_grad[1] (<1>), [4] (<4>)",
    "group_point_grad_kernel": "test_group_point_and_grad[1] (<1>), [4] (<4>)",
    "group_maxpool_kernel": "test_group_maxpool_and_grad",
    "group_maxpool_grad_kernel": "test_group_maxpool_and_grad",
    "sa_group_concat_kernel": "test_sa_group_concat",
    "sa_group_concat_grad_kernel": "test_sa_group_concat_grad",
    "sa_group_concat_grad_csr_narrow_kernel": "test_sa_group_concat_grad_csr_narrow",
    "pad_rows_kernel": "test_pad_rows",
    "csr_count_kernel": "test_inverse_lists_global_build",
    "csr_fill_kernel": "test_inverse_lists_global_build",
    "multi_copy_kernel": "test_multi_copy_more_pieces_than_workgroups",
    # csrc/interpolate.hip
    "three_interpolate_kernel": "test_three_interpolate_and_grad",
    "three_interpolate_grad_kernel": "test_three_interpolate_and_grad",
    "three_nn_weights_kernel": "test_three_nn_weights",
    "fp_concat_kernel": "test_fp_concat[scalar]",
    "fp_concat4_kernel": "test_fp_concat[vec4]",
    "fp_concat_grad_kernel": "test_fp_concat_grad",
    # csrc/mlp.hip, csrc/batchnorm.hip
    "sa_rel_kernel": "test_sa_rel",
    "bn_apply_kernel": "test_bn_apply",
    "bn_backward_apply_kernel": "test_bn_backward_apply",
    "bnrelu_apply_kernel": "test_bnrelu_apply[scalar]",
    "bnrelu_apply4_kernel": "test_bnrelu_apply[vec4]",
    "bnrelu_maxpool_kernel": "test_bnrelu_maxpool[scalar]",
    "bnrelu_maxpool4_kernel": "test_bnrelu_maxpool[vec4]",
    "pool_select_kernel": "test_pool32_select",
    "pool_select_groups_kernel": "test_pool32_select_groups",
    # csrc/nndistance.hip
    "nm_distance_grad_kernel": "test_nm_distance_grad_atomics_and_csr",
    "nm_distance_grad_csr_kernel": "test_nm_distance_grad_atomics_and_csr",
    # csrc/predict.hip, csrc/data_prep.hip, csrc/segments.hip
    "sem_iou_counts_kernel": "test_sem_iou_counts",
    "segment_table_init_kernel": "test_segment_labels",
    "segment_pairs_kernel": "test_segment_labels",
    "segment_gather_kernel": "test_segment_labels",
    "segment_conflicts_kernel": "test_segment_labels",
    "sv_init_kernel": "test_segment_label_vote (s * c counters); in gspn_segment_vote by test_gpu_segments.py::test_row_offsets_are_64_bit, "
                      "(r + 1) * s = 1025 * 32768 = 33,587,200 counters",
    "sl_count_kernel": "test_segment_label_vote",
    "sl_winner_kernel": "test_segment_label_vote[one_class]",
    "sl_gather_kernel": "test_segment_label_vote",
    "sv_size_kernel": "test_gpu_segments.py::test_row_offsets_are_64_bit, v = 2^21 + 3: T = 2,097,155 (the third trip's first three items included)",
    # csrc/deconv.hip
    "dc_sum_parts_kernel": "test_deconv_kernel_gradient_part_sum",
    # csrc/mask_nms.hip, csrc/components.hip, csrc/nearest.hip: their largest tests stay under the cap -- mask_overlaps' b * r * r = 1024 * 1024 is
    # exactly G * B (one trip), the components test at v = 2^24 has about 10,000 faces, nearest_point's b * cells is 65,536 at most
    "mn_init_kernel": "test_mask_overlaps_two_scenes",
    "mc_hook_kernel": "test_mask_components_a_million_faces",
    "nearest_init_kernel": "test_nearest_point_many_scenes",
    # csrc/sampling.hip: a fixed grid of 2048 workgroups walks the rows
    "prefix_rows_kernel": "test_prob_sample_more_rows_than_workgroups",
}

SENT_I = 0x7FC0DEAD
N_OPT = 1_049_579

# (T, B) of every case: the launcher's own item count and block size.  Dimensions first, so that the cases and this table cannot drift apart.
GP = {1: (1, 2048, 67, 1023, 16), 4: (2, 2048, 64, 1065, 31)}                 # b, n, c, m, ns
GMP = (1, 2048, 128, 8201, 4)                                                  # b, n, c, m, ns
TI = (1, 16401, 64, 512)                                                       # b, n, c, m
FPC = {"scalar": (1, 16700, 512, 33, 30, 63), "vec4": (1, 61700, 512, 32, 32, 68)}      # b, n, m, c2, c1, ld
FPG = (1, 16700, 512, 33, 30, 64)
SGC = (1, 2048, 5, 3650, 32, 9)                                                # b, n, c, m, ns, ld
SGG = (1, 2048, 5, 6561, 32, 9)
PAD = (262_200, 3, 4)                                                          # rows, c, ld
REL = (2, 2048, 16401, 32)                                                     # b, n, m, ns
NARROW = (8, 131_201, 3, 64, 8, 5)                                             # b, n, c, m, ns, ld
BN_ROWS = 16401                                                                # x 64 columns (scalar), x 256 / 4 vectors (4-wide)
INV = (9, 116_623, 40_000)                                                     # b, L, n: n > CSR_LDS_MAX_N = 32768, or the LDS build runs and no capped grid
NM = (2, 524_801, 32_800)                                                      # b, n, m
SEM = (N_OPT, 20)
SEGL = (4_194_304 + 1203, N_OPT, N_OPT)                                        # n, p, s
SLV = {"one_class": (N_OPT, N_OPT, 1), "three_classes": (N_OPT, 349_860, 3)}   # v, s, c
DC = (128, 2, 2, 257, 511, 3, 3, 1, 1)                                         # n, hi, wi, cin, cout, kh, kw, sh, sw
MN = (2, 725, 67)                                                              # b, r, v
MC = (2, 1_050_000, 1000)                                                      # r, v, strip length
NP = (1025, 6, 4100)                                                           # b, n, m: cells = m / 4 = 1025


def _prod(*a):
    return int(np.prod([int(x) for x in a], dtype=np.int64))


SHAPES = {
    "adam_flat": (N_OPT, 256), "adam_flat_dev": (N_OPT, 256), "adam_tf_flat": (N_OPT, 256), "momentum_flat": (N_OPT, 256),
    "group_point<1>": (_prod(GP[1][0], GP[1][3], GP[1][4], GP[1][2]), 256),
    "group_point<4>": (_prod(GP[4][0], GP[4][3], GP[4][4], GP[4][2] // 4), 256),
    "group_maxpool": (_prod(GMP[0], GMP[3], GMP[2]), 256),
    "three_interpolate": (_prod(TI[0], TI[1], TI[2]), 256),
    "three_nn_weights": (N_OPT, 256),
    "fp_concat[scalar]": (_prod(FPC["scalar"][0], FPC["scalar"][1], FPC["scalar"][5]), 256),
    "fp_concat[vec4]": (_prod(FPC["vec4"][0], FPC["vec4"][1], FPC["vec4"][5]) // 4, 256),
    "fp_concat_grad": (_prod(FPG[0], FPG[1], FPG[3] + FPG[4]), 256),
    "sa_group_concat": (_prod(SGC[0], SGC[3], SGC[4], SGC[5]), 256),
    "sa_group_concat_grad": (_prod(SGG[0], SGG[3], SGG[4], SGG[2]), 256),
    "sa_group_concat_grad_csr_narrow": (_prod(NARROW[0], NARROW[1]), 256),
    "pad_rows": (_prod(PAD[0], PAD[2]), 256),
    "sa_rel": (_prod(REL[0], REL[2], REL[3]), 256),
    "bn_scalar": (BN_ROWS * 64, 256), "bn_vec4": (BN_ROWS * 256 // 4, 256),
    "inverse_lists": (_prod(INV[0], INV[1]), 256),
    "nm_distance_grad": (_prod(NM[0], NM[1]), 256),
    "nm_distance_grad_csr": (_prod(NM[0], NM[1] + NM[2]), 256),
    "sem_iou_counts": (SEM[0], 256),
    "segment_labels.table": (SEGL[2], 256), "segment_labels.pairs": (SEGL[1], 256), "segment_labels.gather": ((SEGL[0] + 3) // 4, 256),
    "segment_label_vote[one_class].v": (SLV["one_class"][0], 256), "segment_label_vote[one_class].s": (SLV["one_class"][1], 256),
    "segment_label_vote[three_classes].v": (SLV["three_classes"][0], 256),
    "segment_label_vote[three_classes].sc": (SLV["three_classes"][1] * SLV["three_classes"][2], 256),
    "dc_sum_parts": (_prod(DC[5], DC[6], DC[4], DC[3]), 256),
    "mn_init": (_prod(MN[0], MN[1], MN[1]), 256),
    "mc_hook": (MC[1] - MC[1] // MC[2], 256),
    "nearest_init": (_prod(NP[0], NP[2] // 4), 256),
}

TRIPS = {}          # case -> (G, B, T), as asserted


def _lib():
    from gspn_amd import _lib as L
    return L, L.lib()


def trip(case):
    """the assertion every case starts with -> G * B, the first item of the second trip"""
    T, B = SHAPES[case]
    G = int(_lib()[1].gspn_grid_blocks(T, B))
    assert G >= 1 and G * B < T < 2 * G * B and T % B != 0, \
        "%s: T = %d items in blocks of %d on a grid of %d no longer runs one full and one ragged trip; resize the case" % (case, T, B, G)
    TRIPS[case] = (G, B, T)
    print("grid-cap %s: G = %d, B = %d, T = %d" % (case, G, B, T))
    return G * B


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                   # a fault is sticky: nothing more of this file runs on the device
        pytest.exit("GPU error after %s: %s" % (request.node.name, e), returncode=3)
    print("grid-cap wall time %s: %.2f s" % (request.node.name, time.perf_counter() - t0))


def P(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nanf(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def senti(*shape):
    return torch.full(shape, SENT_I, dtype=torch.int32, device="cuda")


def garbage_ws(nbytes):
    """a workspace the call must not rely on: random bytes, 16-byte aligned"""
    assert nbytes >= 0
    return torch.randint(0, 255, (max(int(nbytes), 16),), dtype=torch.uint8, device="cuda")


def _t(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.detach().cuda()


def verdict(what, got, ref, bound, second):
    """|got - ref| <= bound elementwise (0: equal), a sentinel left behind counts as wrong.  second: the output elements a second-trip item
    writes or adds into -- a bool mask, or the first such element of an output laid out like the items.  The message splits by trip."""
    got, ref = _t(got).reshape(-1), _t(ref).reshape(-1)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = (got.double() - ref.double()).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    left = torch.isnan(got) if got.dtype.is_floating_point else got == SENT_I
    if torch.is_tensor(bound) or isinstance(bound, np.ndarray):
        bound = _t(bound).reshape(-1).double()
    bad = (err > bound) | left
    if not bool(bad.any()):
        return
    if isinstance(second, int):
        second = torch.arange(got.numel(), device=got.device) >= second
    else:
        second = _t(second).reshape(-1).bool()
    parts = []
    for name, m in (("first trip [0, G*B)", ~second), ("second trip [G*B, T)", second)):
        e = err[m]
        parts.append("%s: %d of %d elements wrong, worst error %.3g, %d still the sentinel"
                     % (name, int(bad[m].sum()), int(m.sum()), float(e.max()) if e.numel() else 0.0, int(left[m].sum())))
    raise AssertionError("%s -- %s" % (what, "; ".join(parts)))


def sum_bound(scale, tol=1e-5):
    """tests/test_gpu_dropin_grads.py::close: tol x the sum of |terms| that went into each element (atomic adds have no order)"""
    return tol * np.maximum(np.asarray(scale, np.float64), 1e-30) + 1e-12


# ---- the flat optimisers -------------------------------------------------------------------------------------------------------------------

def _adam_tf_step(p, g, t, m, v, lr, b1=0.9, b2=0.999, eps=1e-8):
    """tests/test_gpu_train.py::adam_tf_ref on one float64 tensor (on the device: a million elements)"""
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    m.mul_(b1).add_(g, alpha=1.0 - b1)
    v.mul_(b2).add_(g * g, alpha=1.0 - b2)
    p.sub_(lr_t * m / (v.sqrt() + eps))


@pytest.mark.parametrize("kind", ["adam_flat", "adam_flat_dev", "adam_tf_flat", "momentum_flat"])
def test_flat_optimisers(kind):
    """one parameter of 1,049,579 elements in a FlatGradBucket, three updates behind a bucket summed over 4 ranks (grad_scale = 0.25), against
    torch.optim.Adam / torch.optim.SGD / the TensorFlow rule in float64 at the optimiser tests' 2e-6 of the largest parameter.  gspn_adam_flat
    runs with weight_decay != 0; gspn_adam_flat_dev must leave state == [3, 0]: its ticket counter is drawn by the whole capped grid.
    The gradients have either sign and a magnitude in [0.5, 1.5) x 0.1, 1, 10: Adam's m / (sqrt(v) + eps) is ill-conditioned in fp32 where a
    gradient is comparable to eps or cancels against weight_decay * p, which a few elements in a million normal draws do (2 of 1,049,579 were off
    by 2.7e-5 with them, both in the first trip) and the few thousand elements of the optimiser tests never meet."""
    from gspn_amd.parallel import FlatAdam, FlatGradBucket
    from gspn_amd.train import FlatAdamTF, FlatMomentum
    gb = trip(kind)
    g = torch.Generator().manual_seed(31)
    init = torch.randn(N_OPT, generator=g)
    q = torch.nn.Parameter(init.clone().cuda())
    bucket = FlatGradBucket([q])
    ref = torch.nn.Parameter(init.double().cuda())
    rule = None
    if kind in ("adam_flat", "adam_flat_dev"):
        opt = FlatAdam(bucket, lr=1e-2, weight_decay=1e-3, device_step=kind == "adam_flat_dev")
        rule = torch.optim.Adam([ref], lr=1e-2, weight_decay=1e-3)
    elif kind == "adam_tf_flat":
        opt = FlatAdamTF(bucket, lr=1e-2)
        m64, v64 = torch.zeros_like(ref.data), torch.zeros_like(ref.data)
    else:
        opt = FlatMomentum(bucket, lr=1e-2, momentum=0.9)
        rule = torch.optim.SGD([ref], lr=1e-2, momentum=0.9)
    for step in range(3):
        sign = torch.randint(0, 2, (N_OPT,), generator=g).float() * 2.0 - 1.0
        grad = (sign * (0.5 + torch.rand(N_OPT, generator=g)) * (10.0 ** (step - 1))).cuda()
        bucket.flat.copy_(grad * 4.0)                           # as if summed over 4 ranks: step() scales it back, exactly
        opt.step(grad_scale=0.25)
        if rule is not None:
            ref.grad = grad.double()
            rule.step()
        else:
            _adam_tf_step(ref.data, grad.double(), step + 1, m64, v64, 1e-2)
    torch.cuda.synchronize()
    assert opt.t == 3
    if kind == "adam_flat_dev":
        assert opt._dev_state.tolist() == [3, 0]
    assert opt.flat.data_ptr() <= q.data_ptr() < opt.flat.data_ptr() + 4 * N_OPT
    verdict(kind, q.detach(), ref.detach(), 2e-6 * float(ref.detach().abs().max()), gb)


# ---- group_point, group_maxpool --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vec", [1, 4])
def test_group_point_and_grad(vec):
    """gspn_grouppoint / gspn_grouppoint_grad, the scalar (c = 67) and the four-wide (c = 64) instantiation, indices as in
    tests/test_gpu_geometry.py::test_group_point_and_grad with the repeated-index columns: the gather bit-equal to the C oracle, the atomic
    scatter within 1e-5 of the sum of |terms| (tests/test_gpu_dropin_grads.py) and equal where a point collects one term or none"""
    from oracle import oracle as O
    L, lib = _lib()
    b, n, c, m, ns = GP[vec]
    gb = trip("group_point<%d>" % vec)
    rng = np.random.default_rng(5 + vec)
    pts = rng.standard_normal((b, n, c)).astype(np.float32)
    idx = rng.integers(0, n, size=(b, m, ns)).astype(np.int32)
    idx[:, :, ns // 2:] = idx[:, :, :1]                       # padded rows repeat one index (atomic contention)
    tp, ti = dev(pts), dev(idx)
    out = nanf(b, m, ns, c)
    assert (tp.data_ptr() | out.data_ptr()) % 16 == 0
    assert lib.gspn_grouppoint(b, n, c, m, ns, P(tp), P(ti), P(out), ST()) == 0
    verdict("group_point<%d>" % vec, out, O.group_point(pts, idx), 0.0, gb * vec)
    go = rng.standard_normal((b, m, ns, c)).astype(np.float32)
    g = nanf(b, n, c)
    assert lib.gspn_grouppoint_grad(b, n, c, m, ns, P(dev(go)), P(ti), P(g), ST()) == 0
    torch.cuda.synchronize()
    zero = np.zeros((b, n, c), np.float32)
    ref = O.group_point_grad(zero, idx, go)
    scale = O.group_point_grad(zero, idx, np.abs(go)).astype(np.float64)
    rows = np.arange(b * m * ns)
    late = rows >= (gb * vec) // c                             # the grouped rows (all or part of) whose items a second trip handles
    second = np.zeros((b, n), bool)
    second[rows[late] // (m * ns), idx.reshape(-1)[late]] = True
    second = np.repeat(second[:, :, None], c, axis=2)
    verdict("group_point_grad<%d>" % vec, g, ref, sum_bound(scale), second)
    cnt = np.zeros((b, n), np.int64)
    for i in range(b):
        np.add.at(cnt[i], idx[i].reshape(-1), 1)
    np.testing.assert_array_equal(g.cpu().numpy()[cnt <= 1], ref[cnt <= 1])


def test_group_maxpool_and_grad():
    """gspn_groupmaxpool / gspn_groupmaxpool_grad at b, m, c = 1, 8201, 128, nsample = 4, tied maxima: values and arg-max bit-equal to the C oracle,
    the atomic scatter within 1e-5 of the sum of |terms|"""
    from oracle import oracle as O
    L, lib = _lib()
    b, n, c, m, ns = GMP
    gb = trip("group_maxpool")
    rng = np.random.default_rng(50)
    pts = (np.round(rng.standard_normal((b, n, c)) * 2) / 2).astype(np.float32)         # tied maxima
    idx = rng.integers(0, n, size=(b, m, ns)).astype(np.int32)
    want, wmi = O.group_maxpool(pts, idx)
    out, mi = nanf(b, m, c), senti(b, m, c)
    assert lib.gspn_groupmaxpool(b, n, c, m, ns, P(dev(pts)), P(dev(idx)), P(out), P(mi), ST()) == 0
    verdict("group_maxpool out", out, want, 0.0, gb)
    verdict("group_maxpool max_idx", mi, wmi, 0.0, gb)
    go = rng.standard_normal((b, m, c)).astype(np.float32)
    g = nanf(b, n, c)
    assert lib.gspn_groupmaxpool_grad(b, n, c, m, P(dev(go)), P(dev(wmi)), P(g), ST()) == 0
    torch.cuda.synchronize()
    ref = O.group_maxpool_grad(pts, wmi, go)
    scale = O.group_maxpool_grad(pts, wmi, np.abs(go)).astype(np.float64)
    item = np.arange(b * m * c)
    late = item >= gb
    second = np.zeros((b, n, c), bool)
    second[item[late] // (m * c), wmi.reshape(-1)[late], item[late] % c] = True
    verdict("group_maxpool_grad", g, ref, sum_bound(scale), second)


# ---- three_interpolate, three_nn_weights, fp_concat --------------------------------------------------------------------------------------------

def _interp_inputs(rng, b, n, m):
    idx = rng.integers(0, m, size=(b, n, 3)).astype(np.int32)
    idx[:, ::7, :] = idx[:, :1, :1]                            # a hot sparse point; also i1 == i2 == i3 rows
    w = rng.random((b, n, 3)).astype(np.float32)
    w /= w.sum(2, keepdims=True)
    return idx, w


def _sparse_touched(b, m, idx, first_row):
    """(b, m) bool: the sparse points a dense row >= first_row adds into"""
    n = idx.shape[1]
    second = np.zeros((b, m), bool)
    rows = np.arange(b * n)
    late = rows >= first_row
    for t in range(3):
        second[rows[late] // n, idx.reshape(-1, 3)[late, t]] = True
    return second


def test_three_interpolate_and_grad():
    """gspn_threeinterpolate bit-equal to the C oracle (same products, same order); gspn_threeinterpolate_grad (hardware atomics) within 1e-5 of
    the sum of |terms|, as tests/test_gpu_dropin_grads.py holds it"""
    from oracle import oracle as O
    L, lib = _lib()
    b, n, c, m = TI
    gb = trip("three_interpolate")
    rng = np.random.default_rng(7)
    pts = rng.standard_normal((b, m, c)).astype(np.float32)
    idx, w = _interp_inputs(rng, b, n, m)
    ti, tw = dev(idx), dev(w)
    out = nanf(b, n, c)
    assert lib.gspn_threeinterpolate(b, m, c, n, P(dev(pts)), P(ti), P(tw), P(out), ST()) == 0
    verdict("three_interpolate", out, O.three_interpolate(pts, idx, w), 0.0, gb)
    go = rng.standard_normal((b, n, c)).astype(np.float32)
    g = nanf(b, m, c)
    assert lib.gspn_threeinterpolate_grad(b, n, c, m, P(dev(go)), P(ti), P(tw), P(g), ST()) == 0
    torch.cuda.synchronize()
    zero = np.zeros((b, m, c), np.float32)
    ref = O.three_interpolate_grad(zero, idx, w, go)
    scale = O.three_interpolate_grad(zero, idx, w, np.abs(go)).astype(np.float64)
    second = np.repeat(_sparse_touched(b, m, idx, gb // c)[:, :, None], c, axis=2)
    verdict("three_interpolate_grad", g, ref, sum_bound(scale), second)


def test_three_nn_weights():
    """gspn_three_nn_weights over 1,049,579 rows (the launcher counts rows, three distances each) against the float64 formula at the existing
    test's 1e-6 of the largest weight, coincident points included"""
    L, lib = _lib()
    gb = trip("three_nn_weights")
    g = torch.Generator().manual_seed(1)
    dist = (torch.rand(N_OPT, 3, generator=g) ** 4).cuda()
    dist[::7, 0] = 0.0                                         # coincident points: clamped at 1e-10
    w = nanf(N_OPT, 3)
    assert lib.gspn_three_nn_weights(N_OPT, P(dist), P(w), ST()) == 0
    d = torch.clamp(dist.double(), min=float(np.float32(1e-10)))
    ref = (1.0 / d) / (1.0 / d).sum(dim=1, keepdim=True)
    verdict("three_nn_weights", w, ref, 1e-6 * float(ref.abs().max()), gb * 3)
    assert torch.allclose(w.sum(dim=1), torch.ones(N_OPT, device="cuda"), atol=1e-6)


@pytest.mark.parametrize("width", ["scalar", "vec4"])
def test_fp_concat(width):
    """gspn_fp_concat with c2 + c1 odd (fp_concat_kernel, ld = 63) and a multiple of 4 (fp_concat4_kernel, ld = 68: one zeroed pad vector per row):
    bit-equal to the oracle's three_interpolate next to points1 next to zeros, as tests/test_gpu_modules.py holds it"""
    from oracle import oracle as O
    L, lib = _lib()
    b, n, m, c2, c1, ld = FPC[width]
    gb = trip("fp_concat[%s]" % width)
    rng = np.random.default_rng(70 + ld)
    p2 = rng.standard_normal((b, m, c2)).astype(np.float32)
    p1 = rng.standard_normal((b, n, c1)).astype(np.float32)
    idx, w = _interp_inputs(rng, b, n, m)
    out = nanf(b, n, ld)
    tp2 = dev(p2)
    assert (ld % 4 == 0 and c2 % 4 == 0 and (out.data_ptr() | tp2.data_ptr()) % 16 == 0) == (width == "vec4")
    assert lib.gspn_fp_concat(b, n, m, c2, c1, P(tp2), P(dev(idx)), P(dev(w)), P(dev(p1)), ld, P(out), ST()) == 0
    want = np.zeros((b, n, ld), np.float32)
    want[:, :, :c2] = O.three_interpolate(p2, idx, w)
    want[:, :, c2:c2 + c1] = p1
    verdict("fp_concat[%s]" % width, out, want, 0.0, gb * (4 if width == "vec4" else 1))


def test_fp_concat_grad():
    """gspn_fp_concat_grad over b * n * (c2 + c1) items of a gradient with row pitch 64: the points1 columns a bit-equal slice, the points2 columns the
    atomic three_interpolate_grad within 1e-5 of the sum of |terms|"""
    from oracle import oracle as O
    L, lib = _lib()
    b, n, m, c2, c1, ld = FPG
    gb = trip("fp_concat_grad")
    rng = np.random.default_rng(71)
    idx, w = _interp_inputs(rng, b, n, m)
    go = rng.standard_normal((b, n, ld)).astype(np.float32)
    g2, g1 = nanf(b, m, c2), nanf(b, n, c1)
    assert lib.gspn_fp_concat_grad(b, n, m, c2, c1, ld, P(dev(go)), P(dev(idx)), P(dev(w)), P(g2), P(g1), ST()) == 0
    torch.cuda.synchronize()
    cc = c2 + c1
    item = np.arange(b * n * cc).reshape(b, n, cc)
    verdict("fp_concat_grad points1", g1, go[:, :, c2:cc], 0.0, item[:, :, c2:] >= gb)
    zero = np.zeros((b, m, c2), np.float32)
    part = np.ascontiguousarray(go[:, :, :c2])
    ref = O.three_interpolate_grad(zero, idx, w, part)
    scale = O.three_interpolate_grad(zero, idx, w, np.abs(part)).astype(np.float64)
    second = np.repeat(_sparse_touched(b, m, idx, gb // cc)[:, :, None], c2, axis=2)
    verdict("fp_concat_grad points2", g2, ref, sum_bound(scale), second)


# ---- the set-abstraction front end ------------------------------------------------------------------------------------------------------------

def _group_inputs(rng, b, n, m, ns):
    idx = rng.integers(0, n, size=(b, m, ns))
    idx[:, :, ns // 2:] = idx[:, :, :1]
    return torch.from_numpy(idx.astype(np.int32)).cuda()


@pytest.mark.parametrize("xyz_first", [1, 0])
def test_sa_group_concat(xyz_first):
    """gspn_sa_group_concat over rows * ld_out items, one pad column: [xyz[idx] - new_xyz | points[idx] | 0] or [points[idx] | xyz[idx] - new_xyz | 0],
    bit-equal to the same fp32 gather and subtraction in torch"""
    L, lib = _lib()
    b, n, c, m, ns, ld = SGC
    gb = trip("sa_group_concat")
    gen = torch.Generator(device="cuda").manual_seed(3)
    xyz = torch.randn(b, n, 3, generator=gen, device="cuda")
    new_xyz = torch.randn(b, m, 3, generator=gen, device="cuda")
    pts = torch.randn(b, n, c, generator=gen, device="cuda")
    idx = _group_inputs(np.random.default_rng(3), b, n, m, ns)
    out = nanf(b, m, ns, ld)
    assert lib.gspn_sa_group_concat(b, n, c, m, ns, P(xyz), P(new_xyz), P(pts), P(idx), xyz_first, ld, P(out), ST()) == 0
    flat = (idx.long() + torch.arange(b, device="cuda").view(b, 1, 1) * n).reshape(-1)
    rel = xyz.reshape(-1, 3)[flat].view(b, m, ns, 3) - new_xyz.view(b, m, 1, 3)
    feat = pts.reshape(-1, c)[flat].view(b, m, ns, c)
    want = torch.zeros(b, m, ns, ld, device="cuda")
    want[..., :3 + c] = torch.cat((rel, feat) if xyz_first else (feat, rel), dim=-1)
    verdict("sa_group_concat xyz_first=%d" % xyz_first, out, want, 0.0, gb)


def test_sa_group_concat_grad():
    """gspn_sa_group_concat_grad (atomics) over rows * c items of a gradient with pitch 9 behind the three xyz columns, against a float64 index_add_
    of the same terms (the vectorised form of the oracle's loop), within 1e-5 of the sum of |terms|"""
    L, lib = _lib()
    b, n, c, m, ns, ld = SGG
    gb = trip("sa_group_concat_grad")
    gen = torch.Generator(device="cuda").manual_seed(4)
    go = torch.randn(b, m, ns, ld, generator=gen, device="cuda")
    idx = _group_inputs(np.random.default_rng(4), b, n, m, ns)
    g = nanf(b, n, c)
    assert lib.gspn_sa_group_concat_grad(b, n, c, m, ns, P(idx), 1, ld, P(go), P(g), ST()) == 0
    flat = (idx.long() + torch.arange(b, device="cuda").view(b, 1, 1) * n).reshape(-1)
    terms = go[..., 3:3 + c].reshape(-1, c).double()
    ref = torch.zeros(b * n, c, dtype=torch.float64, device="cuda").index_add_(0, flat, terms)
    scale = torch.zeros(b * n, c, dtype=torch.float64, device="cuda").index_add_(0, flat, terms.abs())
    second = torch.zeros(b * n, dtype=torch.bool, device="cuda")
    second[flat[gb // c:]] = True
    verdict("sa_group_concat_grad", g, ref, 1e-5 * scale.clamp(min=1e-30) + 1e-12, second.view(-1, 1).expand(-1, c))


def test_sa_group_concat_grad_csr_narrow():
    """the narrow path (c <= 8) of gspn_sa_group_concat_grad_csr counts b * n data points: 8 x 131,201 of them, 512 grouped rows per scene.  The
    inverse lists are a stable sort here, not the library's; the sums are in ascending grouped position, so the result is bit-equal to the same fp32
    additions in that order (numpy, one list entry per step: the vectorised form of the sequential loop)"""
    L, lib = _lib()
    b, n, c, m, ns, ld = NARROW
    gb = trip("sa_group_concat_grad_csr_narrow")
    ln = m * ns
    rng = np.random.default_rng(8)
    idx = rng.integers(0, n, size=(b, ln))
    idx[:, : ln // 4] = rng.integers(n - 40, n, size=(b, ln // 4))            # crowded points of the second trip's end
    idx[:, ln // 4: ln // 4 + 40] = 7                                          # and one long list in the first
    go = rng.standard_normal((b, ln, ld)).astype(np.float32)
    order = np.argsort(idx, axis=1, kind="stable")
    cnt = np.stack([np.bincount(idx[i], minlength=n) for i in range(b)])
    offsets = np.concatenate((np.zeros((b, 1), np.int64), np.cumsum(cnt, axis=1)), axis=1)
    want = np.zeros((b, n, c), np.float32)
    for i in range(b):
        for k in range(int(cnt[i].max())):
            sel = np.flatnonzero(cnt[i] > k)
            want[i, sel] += go[i, order[i, offsets[i, sel] + k], :c]
    g = nanf(b, n, c)
    assert lib.gspn_sa_group_concat_grad_csr(b, n, c, m, ns, P(dev(order.astype(np.int32))), P(dev(offsets.astype(np.int32))), 0, ld, P(dev(go)), P(g),
                                             ST()) == 0
    assert int(cnt.max()) >= 40 and int((cnt.reshape(-1)[gb:] > 1).sum()) > 0
    verdict("sa_group_concat_grad_csr narrow", g, want, 0.0, gb * c)


def test_pad_rows():
    L, lib = _lib()
    rows, c, ld = PAD
    gb = trip("pad_rows")
    src = torch.randn(rows, c, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")
    dst = nanf(rows, ld)
    assert lib.gspn_pad_rows(rows, c, ld, P(src), P(dst), ST()) == 0
    want = torch.zeros(rows, ld, device="cuda")
    want[:, :c] = src
    verdict("pad_rows", dst, want, 0.0, gb)


@pytest.mark.parametrize("shifted", [False, True])
def test_sa_rel(shifted):
    """gspn_sa_rel / gspn_sa_rel_shift over b * m * ns grouped rows: centred coordinates (a second fp32 subtraction with a shift) in 16-byte rows and
    the source row, bit-equal to the same arithmetic in torch"""
    L, lib = _lib()
    b, n, m, ns = REL
    gb = trip("sa_rel")
    gen = torch.Generator(device="cuda").manual_seed(6)
    xyz = torch.randn(b, n, 3, generator=gen, device="cuda")
    new_xyz = torch.randn(b, m, 3, generator=gen, device="cuda")
    shift = torch.randn(b, m, 3, generator=gen, device="cuda")
    idx = _group_inputs(np.random.default_rng(6), b, n, m, ns)
    rel, gidx = nanf(b * m * ns, 4), senti(b * m * ns)
    if shifted:
        assert lib.gspn_sa_rel_shift(b, n, m, ns, P(xyz), P(new_xyz), P(shift), P(idx), P(rel), P(gidx), ST()) == 0
    else:
        assert lib.gspn_sa_rel(b, n, m, ns, P(xyz), P(new_xyz), P(idx), P(rel), P(gidx), ST()) == 0
    flat = (idx.long() + torch.arange(b, device="cuda").view(b, 1, 1) * n).reshape(-1)
    d = xyz.reshape(-1, 3)[flat].view(b, m, ns, 3) - new_xyz.view(b, m, 1, 3)
    if shifted:
        d = d - shift.view(b, m, 1, 3)
    want = torch.zeros(b * m * ns, 4, device="cuda")
    want[:, :3] = d.reshape(-1, 3)
    verdict("sa_rel rel", rel, want, 0.0, gb * 4)
    verdict("sa_rel gidx", gidx, flat.int(), 0.0, gb)


# ---- batch-norm applications and pools ----------------------------------------------------------------------------------------------------------
# z = fl(fl(y * scale) + shift): two roundings of at most 2^-24 relative each, so |z - exact| <= 2^-23 (|y * scale| + |shift|) -- and a fused
# multiply-add, one rounding, lies inside the same bound.  The arg-max is compared with the first maximum of the same fp32 arithmetic in torch
# (separate multiply and add: the library is built without contraction).

EPS2 = 2.0 ** -23


def _bn_inputs(rows, c, ld, seed, negative=()):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    Y = torch.randn(rows, ld, generator=gen, device="cuda")
    scale = torch.rand(c, generator=gen, device="cuda") + 0.5
    shift = torch.randn(c, generator=gen, device="cuda") * 0.5
    for k in negative:
        scale[k] = -scale[k]
    return Y, scale, shift


def _first_max(z, dim):
    """(values, first index) of the maximum along dim"""
    vmax = z.max(dim=dim, keepdim=True).values
    pos = torch.arange(z.shape[dim], device=z.device).view([-1 if k == dim else 1 for k in range(z.dim())])
    arg = torch.where(z == vmax, pos, torch.full_like(pos, z.shape[dim])).min(dim=dim).values
    return vmax.squeeze(dim), arg.int()


@pytest.mark.parametrize("relu", [0, 1])
def test_bn_apply(relu):
    L, lib = _lib()
    rows, c, ldx, ldo = BN_ROWS, 64, 67, 65
    gb = trip("bn_scalar")
    X, scale, shift = _bn_inputs(rows, c, ldx, 11, negative=(5,))
    out = nanf(rows, ldo)
    assert lib.gspn_bn_apply(rows, c, P(X), ldx, P(scale), P(shift), relu, P(out), ldo, ST()) == 0
    x = X[:, :c].double()
    ref = x * scale.double() + shift.double()
    bound = EPS2 * ((x * scale.double()).abs() + shift.double().abs())
    if relu:
        ref = ref.clamp(min=0.0)
    verdict("bn_apply relu=%d" % relu, out[:, :c], ref, bound, gb)
    assert bool(torch.isnan(out[:, c:]).all())                  # the pitch columns are not the kernel's


def test_bn_backward_apply():
    """dx = fma(cA, dz, fma(cB, x, cC)): two roundings, |error| <= 2^-23 (|cA dz| + |cB x| + |cC|)"""
    L, lib = _lib()
    rows, c, ldz, ldx, lddx = BN_ROWS, 64, 64, 66, 65
    gb = trip("bn_scalar")
    dZ, cA, cC = _bn_inputs(rows, c, ldz, 12)
    X, cB, _ = _bn_inputs(rows, c, ldx, 13, negative=(1, 9))
    dX = nanf(rows, lddx)
    assert lib.gspn_bn_backward_apply(rows, c, P(dZ), ldz, P(X), ldx, P(cA), P(cB), P(cC), P(dX), lddx, ST()) == 0
    a, bq = cA.double() * dZ[:, :c].double(), cB.double() * X[:, :c].double()
    verdict("bn_backward_apply", dX[:, :c], a + bq + cC.double(), EPS2 * (a.abs() + bq.abs() + cC.double().abs()), gb)


@pytest.mark.parametrize("width", ["scalar", "vec4"])
def test_bnrelu_apply(width):
    """gspn_bnrelu_apply: c = 64 on rows of an odd pitch (bnrelu_apply_kernel), c = 256 on 16-byte rows (bnrelu_apply4_kernel)"""
    L, lib = _lib()
    rows = BN_ROWS
    c, ldy, ldo = (64, 65, 67) if width == "scalar" else (256, 260, 256)
    gb = trip("bn_" + width)
    Y, scale, shift = _bn_inputs(rows, c, ldy, 14, negative=(3,))
    out = nanf(rows, ldo)
    assert lib.gspn_bnrelu_apply(rows, c, P(Y), ldy, P(scale), P(shift), P(out), ldo, ST()) == 0
    y = Y[:, :c].double()
    ref = (y * scale.double() + shift.double()).clamp(min=0.0)
    bound = EPS2 * ((y * scale.double()).abs() + shift.double().abs())
    verdict("bnrelu_apply[%s]" % width, out[:, :c], ref, bound, gb * (4 if width == "vec4" else 1))


@pytest.mark.parametrize("width", ["scalar", "vec4"])
def test_bnrelu_maxpool(width):
    """gspn_bnrelu_maxpool over groups * c items: c = 64 on an odd pitch with 3 rows per group (bnrelu_maxpool_kernel), c = 256 with 9 rows per group, one
    more than the 4-wide kernel keeps in flight (bnrelu_maxpool4_kernel)"""
    L, lib = _lib()
    groups = BN_ROWS
    c, ldy, ns = (64, 65, 3) if width == "scalar" else (256, 256, 9)
    gb = trip("bn_" + width)
    Y, scale, shift = _bn_inputs(groups * ns, c, ldy, 15, negative=(2,))
    out, arg = nanf(groups, c), senti(groups, c)
    assert lib.gspn_bnrelu_maxpool(groups, ns, c, P(Y), ldy, P(scale), P(shift), P(out), P(arg), ST()) == 0
    per = 4 if width == "vec4" else 1
    z32 = (Y[:, :c] * scale + shift).clamp(min=0.0).view(groups, ns, c)
    _, first = _first_max(z32, 1)
    verdict("bnrelu_maxpool[%s] arg" % width, arg, first, 0.0, gb * per)
    y = Y[:, :c].double().view(groups, ns, c)
    z = (y * scale.double() + shift.double()).clamp(min=0.0)
    at = first.long().unsqueeze(1)
    ref = z.gather(1, at).squeeze(1)
    bound = EPS2 * ((y * scale.double()).abs().gather(1, at).squeeze(1) + shift.double().abs())
    verdict("bnrelu_maxpool[%s] out" % width, out, ref, bound, gb * per)


def _pool_select_check(what, gb, per, groups, rows_per_group, c, Y, scale, shift, out, arg, yarg):
    """out = relu(scale * y* + shift) with y* the group's maximum, its minimum for a negative scale; arg its first row; yarg = y*"""
    y = Y.view(groups, rows_per_group, c)
    vmax, amax = _first_max(y, 1)
    vmin, amin = _first_max(-y, 1)
    neg = (scale < 0).view(1, c)
    ystar = torch.where(neg, -vmin, vmax)
    verdict(what + " arg", arg, torch.where(neg, amin, amax), 0.0, gb * per)
    verdict(what + " y at the arg row", yarg, ystar, 0.0, gb * per)
    prod = ystar.double() * scale.double()
    verdict(what + " out", out, (prod + shift.double()).clamp(min=0.0), EPS2 * (prod.abs() + shift.double().abs()), gb * per)


def test_pool32_select():
    """gspn_pool32_select over groups * c items with the tile maxima the forward epilogue would have left (first maximum of each 32-row group), two
    channels with a negative scale that re-read their 32 values of Y; vmax leaves as y at the arg row"""
    L, lib = _lib()
    groups, c = BN_ROWS, 64
    gb = trip("bn_scalar")
    Y, scale, shift = _bn_inputs(groups * 32, c, c, 16, negative=(0, 37))
    vmax, amax = _first_max(Y.view(groups, 32, c), 1)
    vmax, amax = vmax.contiguous(), amax.contiguous()
    out, arg = nanf(groups, c), senti(groups, c)
    assert lib.gspn_pool32_select(groups, c, P(vmax), P(amax), P(Y), c, P(scale), P(shift), P(out), P(arg), ST()) == 0
    _pool_select_check("pool32_select", gb, 1, groups, 32, c, Y, scale, shift, out, arg, vmax)


def test_pool32_select_groups():
    """gspn_pool32_select_groups over groups * c / 4 vectors, two 32-row tiles per group: the first largest tile maximum, row offset 32 * tile + its own"""
    L, lib = _lib()
    groups, c, sub = BN_ROWS, 256, 2
    gb = trip("bn_vec4")
    Y, scale, shift = _bn_inputs(groups * sub * 32, c, c, 17, negative=(4, 255))
    vmax, amax = _first_max(Y.view(groups * sub, 32, c), 1)
    vmax, amax = vmax.contiguous(), amax.contiguous()
    out, arg, yarg = nanf(groups, c), senti(groups, c), nanf(groups, c)
    assert lib.gspn_pool32_select_groups(groups, sub, c, P(vmax), P(amax), P(Y), c, P(scale), P(shift), P(out), P(arg), P(yarg), ST()) == 0
    _pool_select_check("pool32_select_groups", gb, 4, groups, 32 * sub, c, Y, scale, shift, out, arg, yarg)


# ---- inverse lists, nn_distance gradient --------------------------------------------------------------------------------------------------------

def test_inverse_lists_global_build():
    """gspn_inverse_lists with n = 40,000 values: above CSR_LDS_MAX_N = 32,768 the count and fill passes are grid-stride kernels over b * L positions
    (below it one workgroup per scene builds the lists in LDS and no capped grid is launched) == stable sort + searchsorted, crowded values and
    positions outside [0, n) (dropped) included"""
    from gspn_amd.geometry import inverse_lists
    b, ln, n = INV
    trip("inverse_lists")
    g = torch.Generator().manual_seed(ln + n)
    idx = torch.randint(0, n, (b, ln), generator=g, dtype=torch.int32)
    idx[:, : ln // 3] = idx[:, : ln // 3] % 3                 # a few crowded values: long groups
    idx[:, -500:] = idx[:, -500:] % 5 + n - 5                  # ... also among the last positions
    bad = torch.rand(b, ln, generator=g) < 0.03
    idx[bad] = torch.where(torch.rand(int(bad.sum()), generator=g) < 0.5, torch.tensor(-1, dtype=torch.int32), torch.tensor(n + 5, dtype=torch.int32))
    order, offsets = inverse_lists(idx.cuda(), n)
    order, offsets = order.cpu().long(), offsets.cpu().long()
    for s_ in range(b):
        valid = (idx[s_] >= 0) & (idx[s_] < n)
        pos = torch.nonzero(valid).squeeze(1)
        keys, perm = torch.sort(idx[s_][valid].long(), stable=True)
        nv = int(valid.sum())
        assert int(offsets[s_, n]) == nv, s_
        assert torch.equal(offsets[s_], torch.searchsorted(keys.contiguous(), torch.arange(n + 1))), s_
        assert torch.equal(order[s_, :nv], pos[perm]), s_


def test_nm_distance_grad_atomics_and_csr():
    """gspn_nmdistance_grad beyond the LDS kernel (n + m > 4096: global atomics, one launch over b * n points, one over b * m) and
    gspn_nmdistance_grad_csr (one launch over b * (n + m)) at b, n, m = 2, 524,801, 32,800.  The indices are drawn, not searched -- the gradient takes
    any index --, about 16 terms per point of the smaller cloud and one point with 1000, no more than the existing tests' hot points.  Against the C
    oracle's loop: the atomics within 1e-5 of the sum of |terms| (tests/test_gpu_dropin_grads.py::test_nmdistance_grad_symbol), the gather at that
    test's rtol = 1e-5, atol = 1e-5 of the largest element"""
    from gspn_amd.geometry import inverse_lists
    from oracle import oracle as O
    L, lib = _lib()
    b, n, m = NM
    gb = trip("nm_distance_grad")
    gb_csr = trip("nm_distance_grad_csr")
    rng = np.random.default_rng(m)
    a = rng.standard_normal((b, n, 3)).astype(np.float32)
    c = rng.standard_normal((b, m, 3)).astype(np.float32)
    i1 = rng.integers(0, m, size=(b, n)).astype(np.int32)
    i1[:, -1000:] = m - 3                                      # a hot point fed by the last items
    i2 = rng.integers(0, n, size=(b, m)).astype(np.int32)
    g1 = rng.standard_normal((b, n)).astype(np.float32)
    g2 = rng.standard_normal((b, m)).astype(np.float32)
    ta, tc, tg1, tg2, ti1, ti2 = dev(a), dev(c), dev(g1), dev(g2), dev(i1), dev(i2)
    ga, gc = nanf(b, n, 3), nanf(b, m, 3)
    assert lib.gspn_nmdistance_grad(b, n, P(ta), m, P(tc), P(tg1), P(ti1), P(tg2), P(ti2), P(ga), P(gc), ST()) == 0
    o1, f1 = inverse_lists(ti1, m)
    o2, f2 = inverse_lists(ti2, n)
    ha, hc = nanf(b, n, 3), nanf(b, m, 3)
    assert lib.gspn_nmdistance_grad_csr(b, n, P(ta), m, P(tc), P(tg1), P(ti1), P(tg2), P(ti2), P(o1), P(f1), P(o2), P(f2), P(ha), P(hc), ST()) == 0
    torch.cuda.synchronize()
    r1, r2 = O.nn_distance_grad(a, c, g1, i1, g2, i2)
    s1, s2 = np.zeros((b, n, 3)), np.zeros((b, m, 3))
    for i in range(b):
        t = 2 * np.abs(g1[i])[:, None].astype(np.float64) * np.abs(a[i] - c[i][i1[i]])
        s1[i] += t
        np.add.at(s2[i], i1[i], t)
        t = 2 * np.abs(g2[i])[:, None].astype(np.float64) * np.abs(c[i] - a[i][i2[i]])
        s2[i] += t
        np.add.at(s1[i], i2[i], t)
    item = np.arange(b * n)
    second2 = np.zeros((b, m), bool)
    second2[item[gb:] // n, i1.reshape(-1)[gb:]] = True
    verdict("nm_distance_grad grad_xyz1", ga, r1, sum_bound(s1), gb * 3)
    verdict("nm_distance_grad grad_xyz2", gc, r2, sum_bound(s2), np.repeat(second2[:, :, None], 3, axis=2))
    verdict("nm_distance_grad_csr grad_xyz1", ha, r1, 1e-5 * np.abs(r1) + 1e-5 * float(np.abs(r1).max()), gb_csr * 3)
    verdict("nm_distance_grad_csr grad_xyz2", hc, r2, 1e-5 * np.abs(r2) + 1e-5 * float(np.abs(r2).max()), max(gb_csr - b * n, 0) * 3)


# ---- integer stages --------------------------------------------------------------------------------------------------------------------------------

def test_sem_iou_counts():
    """gspn_sem_iou_counts over 1,049,579 rows of 20 one-decimal logits (equal maxima happen; the first wins), added into accumulators that are not
    zero, against tests/predict_ref.py::iou_counts"""
    from gspn_amd.predict import semantic_iou_counts
    from tests import predict_ref as PR
    rows, c = SEM
    gb = trip("sem_iou_counts")
    rng = np.random.default_rng(rows + c)
    logits = np.round(1.5 * rng.standard_normal((rows, c)), 1).astype(np.float32)
    logits[::5, 0] = 9.0
    logits[::5, c - 1] = 9.0
    logits[1::5, c - 1] = 9.0
    logits[2::5, 1] = 9.0
    logits[2::5, 2] = 9.0
    labels = rng.integers(0, c, rows).astype(np.int32)
    labels[::3] = 0
    start = (np.arange(c - 1, dtype=np.int64) * 1000 + 7, np.arange(c - 1, dtype=np.int64) * 3000 + 11)
    inter, union = dev(start[0].copy()), dev(start[1].copy())
    got = semantic_iou_counts(dev(logits), dev(labels), inter, union)
    assert got[0] is inter and got[1] is union
    want = PR.iou_counts(logits, labels, c, start[0].copy(), start[1].copy())
    if not (np.array_equal(inter.cpu().numpy(), want[0]) and np.array_equal(union.cpu().numpy(), want[1])):
        first = PR.iou_counts(logits[:gb], labels[:gb], c, start[0].copy(), start[1].copy())
        raise AssertionError("sem_iou_counts: got %s / %s, want %s / %s; the rows of the first trip [0, G*B) alone give %s / %s"
                             % (inter.tolist(), union.tolist(), want[0].tolist(), want[1].tolist(), first[0].tolist(), first[1].tolist()))


@pytest.mark.parametrize("offset", [0, 1])
def test_segment_labels(offset):
    """gspn_segment_labels with n = 2^22 + 1203 vertices (the gather counts 16-byte vectors), p = s = 1,049,579 pairs and segments, segment ids outside
    [0, s) on both sides; offset 1: seg_indices and out_label are [1:] views, 4-byte aligned only.  The reference's loop over the pairs (last pair of
    a segment wins) as numpy array operations: an assignment through a repeated index keeps the last value, bincount counts the pairs"""
    L, lib = _lib()
    n, p, s = SEGL
    for part in ("table", "pairs", "gather"):
        gb = trip("segment_labels." + part)
    rng = np.random.default_rng(9 + offset)
    seg = rng.integers(0, s, size=n).astype(np.int32)
    seg[::1001] = -1
    seg[5::1001] = s + 4
    seg[-40:] = s - 1                                           # the last segment, read by the last vector and the tail
    pair_segment = rng.integers(0, s, size=p).astype(np.int32)
    pair_segment[::997] = s + 1
    pair_segment[3::997] = -2
    pair_segment[-1] = s - 1
    pair_object = rng.integers(0, 5000, size=p).astype(np.int32)
    inside = (pair_segment >= 0) & (pair_segment < s)
    winner = np.full(s, -1, np.int64)
    winner[pair_segment[inside]] = np.flatnonzero(inside)       # ascending pair index: the last one stays
    named = np.bincount(pair_segment[inside], minlength=s)
    ok = (seg >= 0) & (seg < s)
    w = np.where(ok, winner[np.clip(seg, 0, s - 1)], -1)
    want = np.where(w >= 0, pair_object[np.maximum(w, 0)], -1).astype(np.int32)
    seen = np.zeros(s, bool)
    seen[seg[w >= 0]] = True
    conflicts = int((named[seen] - 1).sum())
    assert conflicts > 0 and (want == -1).any() and winner[s - 1] == p - 1
    tseg = torch.empty(n + offset, dtype=torch.int32, device="cuda")[offset:]
    tseg.copy_(torch.from_numpy(seg))
    label = senti(n + offset)[offset:]
    assert tseg.data_ptr() % 16 == 4 * offset and label.data_ptr() % 16 == 4 * offset
    out_conflicts = senti(1)
    ws = garbage_ws(int(lib.gspn_segment_labels_ws_bytes(s)))
    assert lib.gspn_segment_labels(n, p, s, P(tseg), P(dev(pair_segment)), P(dev(pair_object)), P(ws), P(label), P(out_conflicts), ST()) == 0
    head = (4 - offset) % 4                                     # the entries in front of the first 16-byte boundary
    verdict("segment_labels label (offset %d)" % offset, label, want, 0.0, head + 4 * gb)
    assert int(out_conflicts.item()) == conflicts


@pytest.mark.parametrize("kind", ["one_class", "three_classes"])
def test_segment_label_vote(kind):
    """gspn_segment_label_vote with v and s just past the cap and one class (the counters, the winners and both passes over the vertices take two
    trips), and with three classes and s * c just past it (a real vote): with two classes or more, s past the cap puts s * c past 2 * G * B, where
    the trip assertion does not hold, so no one shape does both.  tests/segments_ref.py::segment_label_vote_ref loops over the vertices in
    Python; here the same definition as numpy array operations: bincount, the first maximum by argmax"""
    from gspn_amd.segments import segment_label_vote
    L, lib = _lib()
    v, s, c = SLV[kind]
    gb = trip("segment_label_vote[%s].v" % kind)
    trip("segment_label_vote[%s].%s" % (kind, "s" if kind == "one_class" else "sc"))
    rng = np.random.default_rng(v % 1000 + c)
    seg = rng.integers(0, s, size=v).astype(np.int32)
    seg[: v // 2] = seg[: v // 2] % 5000                       # segments with many voters, and many with one or none
    seg[::777] = -1
    seg[1::777] = s
    seg[-3:] = s - 1
    labels = rng.integers(-1, c + 1, size=v).astype(np.int32)  # -1 and c do not vote
    inside = (seg >= 0) & (seg < s)
    votes = inside & (labels >= 0) & (labels < c)
    cnt = np.bincount(seg[votes].astype(np.int64) * c + labels[votes], minlength=s * c)[:s * c].reshape(s, c)
    win = np.where(cnt.max(1) > 0, cnt.argmax(1), -1)
    w = np.where(inside, win[np.clip(seg, 0, s - 1)], -1)
    want = np.where(w >= 0, w, labels).astype(np.int32)
    assert (want != labels).any()
    ws = garbage_ws(int(lib.gspn_segment_label_vote_ws_bytes(v, s, c)))
    out = segment_label_vote(dev(labels), dev(seg), s, c, ws=ws)
    verdict("segment_label_vote[%s]" % kind, out, want, 0.0, gb)


# ---- the sum of the kernel gradient's partial tiles -----------------------------------------------------------------------------------------------

def test_deconv_kernel_gradient_part_sum():
    """gspn_deconv_bwd_kernel at 128 decodes of a 2 x 2 map, 3 x 3 taps, 257 -> 511 channels: the 512 reduction rows are split in two, and
    dc_sum_parts_kernel adds the two partial kernels over 3 * 3 * 511 * 257 = 1,181,943 elements.  Against float64 autograd of tests/deconv_ref.py
    at tests/test_gpu_deconv.py's 1e-5 of the largest element; 512 terms per element, a quarter of that test's (512, 2, 2, 512, 256, 3, 3, 1, 1)"""
    from tests import deconv_ref as DR
    L, lib = _lib()
    n, hi, wi, cin, cout, kh, kw, sh, sw = DC
    gb = trip("dc_sum_parts")
    T = SHAPES["dc_sum_parts"][0]
    gen = torch.Generator(device="cuda").manual_seed(sum(DC))
    x = torch.randn(n, hi, wi, cin, generator=gen, device="cuda")
    k64 = torch.zeros(kh, kw, cout, cin, dtype=torch.float64, device="cuda", requires_grad=True)
    b64 = torch.zeros(cout, dtype=torch.float64, device="cuda", requires_grad=True)
    y64 = DR.deconv(x.double(), k64, b64, (sh, sw))
    dy = torch.randn(y64.shape, generator=gen, device="cuda")
    rk, rb = torch.autograd.grad(y64, (k64, b64), dy.double())
    work = int(lib.gspn_deconv_bwd_kernel_work_bytes(*DC))
    assert work >= 4 * (2 * T + cout), "the reduction is no longer split: dc_sum_parts_kernel does not run over the kernel"
    ws = nanf((work + 3) // 4)
    dk, db = nanf(kh, kw, cout, cin), nanf(cout)
    assert lib.gspn_deconv_bwd_kernel(*DC, P(dy), P(x), P(dk), P(db), P(ws), ST()) == 0
    verdict("deconv dK", dk, rk, 1e-5 * float(rk.abs().max()), gb)
    verdict("deconv dbias", db, rb, 1e-5 * float(rb.abs().max()), cout)


# ---- the three init / hook kernels whose own tests stay under the cap -----------------------------------------------------------------------------

def test_mask_overlaps_two_scenes():
    """gspn_mask_overlaps at b, r = 2, 725: mn_init_kernel clears b * r * r = 1,051,250 counters the Gram kernel then adds into (one scene of 1024 rows,
    the largest elsewhere, is exactly G * B).  Outputs start as the sentinel, so a counter the init pass skipped shows."""
    from tests import mask_nms_ref as ref
    L, lib = _lib()
    b, r, v = MN
    gb = trip("mn_init")
    rng = np.random.default_rng(12)
    masks = (rng.random((b, r, v)) < 0.4).astype(np.uint8) * rng.choice(np.array([1, 2, 255], np.uint8), size=(b, r, v))
    sizes, inter = senti(b, r), senti(b, r, r)
    ws = garbage_ws(int(lib.gspn_mask_overlaps_ws_bytes(b, r, v)))
    assert ws.data_ptr() % 16 == 0
    assert lib.gspn_mask_overlaps(b, r, v, P(dev(masks)), P(ws), P(sizes), P(inter), ST()) == 0
    want = [ref.mask_overlaps_ref(masks[k]) for k in range(b)]
    verdict("mask_overlaps sizes", sizes, np.stack([w_[0] for w_ in want]), 0.0, b * r)
    verdict("mask_overlaps inter", inter, np.stack([w_[1] for w_ in want]), 0.0, gb)


def test_mask_components_a_million_faces():
    """gspn_mask_components with f = 1,048,950 faces: one degenerate face (a, a + 1, a + 1) per edge of 1050 paths of 1000 consecutive vertices, in
    shuffled order, so every face is the only one that joins its two vertices and a face the hook pass skipped splits a component.  tests/components_ref.py
    runs a union-find in Python; the definition on this mesh is a running maximum: a component starts at a set vertex whose predecessor is unset or
    in another path, and its smallest vertex is where it starts.  Row 1 has holes that cut paths."""
    from gspn_amd.components import mask_components
    L, lib = _lib()
    r, v, strip = MC
    trip("mc_hook")
    rng = np.random.default_rng(13)
    a = np.arange(v - 1)
    a = a[(a + 1) % strip != 0]
    assert a.shape[0] == SHAPES["mc_hook"][0]
    a = a[rng.permutation(a.shape[0])]
    faces = np.stack((a, a + 1, a + 1), axis=1).astype(np.int32)
    masks = np.full((r, v), 255, np.uint8)
    masks[1, rng.integers(0, v, size=3000)] = 0
    masks[1, strip * 7: strip * 9] = 0
    at = np.arange(v)
    want = np.empty((r, v), np.int32)
    for k in range(r):
        on = masks[k] != 0
        start = on & ((at % strip == 0) | ~np.concatenate(([False], on[:-1])))
        want[k] = np.where(on, np.maximum.accumulate(np.where(start, at, 0)), -1)
    f = faces.shape[0]
    ws = garbage_ws(int(lib.gspn_mask_components_ws_bytes(r, v, f)))
    comp, ncomp, largest = mask_components(dev(masks), dev(faces), ws=ws)
    got = comp.cpu().numpy()
    wrong = np.flatnonzero((got != want).reshape(-1))
    assert wrong.size == 0, "%d vertices in the wrong component, the first at (row, vertex) %s: %s instead of %s" % (
        wrong.size, divmod(int(wrong[0]), v), got.reshape(-1)[wrong[:5]].tolist(), want.reshape(-1)[wrong[:5]].tolist())
    assert ncomp.tolist() == [int(np.unique(w_[w_ >= 0]).size) for w_ in want]
    assert largest.tolist() == [int(np.bincount(w_[w_ >= 0]).max()) for w_ in want]


def test_nearest_point_many_scenes():
    """gspn_nearest_point with 1025 scenes of 4100 known points: nearest_init_kernel clears b * cells = 1025 * 1025 counters of a workspace that starts as
    garbage, and resets the first b headers.  Against the definition in torch: the unfused fp32 (dx*dx + dy*dy) + dz*dz, the lowest index among equal
    distances"""
    from gspn_amd.nearest import nearest_point
    L, lib = _lib()
    b, n, m = NP
    trip("nearest_init")
    gen = torch.Generator(device="cuda").manual_seed(14)
    known = torch.rand(b, m, 3, generator=gen, device="cuda")
    known[:, 1::2] = known[:, ::2]                              # every point twice: the lower index wins
    q = torch.rand(b, n, 3, generator=gen, device="cuda")
    ws = garbage_ws(int(lib.gspn_nearest_point_ws_bytes(b, m)))
    dist, idx = nearest_point(q, known, ws=ws)
    d = q.view(b, n, 1, 3) - known.view(b, 1, m, 3)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    want_d, want_i = _first_max(-d2, 2)
    assert torch.equal(dist, -want_d) and torch.equal(idx, want_i)
    assert bool((idx % 2 == 0).all())


# ---- the two launchers with a grid of their own ---------------------------------------------------------------------------------------------------

def _own_grid(source, pattern):
    """the cap a launcher writes into its own grid expression, read from the source"""
    with open(os.path.join(CSRC, source)) as fh:
        found = re.search(pattern, fh.read())
    assert found, "%s: the launcher's grid is no longer `x < CAP ? x : CAP`; bring this case up to date" % source
    return int(found.group(1))


def test_multi_copy_more_pieces_than_workgroups():
    """gspn_multi_copy splits its segments into 64 KB pieces and walks them with at most 2048 workgroups: one segment of 2101 pieces (and 5 bytes), an
    unaligned one of three pieces, small ones -- the first 78 workgroups take a second piece, the others do not"""
    from gspn_amd.graph import copy_into
    G = _own_grid("grouping.hip", r"multi_copy_kernel, dim3\(\(unsigned\)\(np < (\d+) \? np : \1\)\)")
    sizes = [2100 * 16384 + 5, 3, 17, 4096, 300001]
    pieces = sum((4 * s_ + 65535) // 65536 for s_ in sizes) + 3
    assert G < pieces < 2 * G, "multi_copy: %d pieces on a grid of %d" % (pieces, G)
    print("grid-cap multi_copy: G = %d workgroups, T = %d pieces" % (G, pieces))
    gen = torch.Generator(device="cuda").manual_seed(0)
    src = [torch.randn(s_, generator=gen, device="cuda") for s_ in sizes]
    src.append(torch.randn(40000, generator=gen, device="cuda")[1:39998])          # 4-byte aligned only: three pieces, bytewise
    dst = [nanf(s_) for s_ in sizes] + [nanf(39999)[2:39999]]
    copy_into({"a": dst}, {"a": src})
    torch.cuda.synchronize()
    for k, (d, s_) in enumerate(zip(dst, src)):
        wrong = torch.nonzero(d.view(torch.int32) != s_.view(torch.int32)).reshape(-1)
        assert wrong.numel() == 0, "segment %d: %d floats differ, the first in its piece %d" % (k, wrong.numel(), int(wrong[0]) * 4 // 65536)


def test_prob_sample_more_rows_than_workgroups():
    """gspn_probsample walks its rows with at most 2048 workgroups: 3001 rows, so 953 workgroups sum a second row.  Prefix sums and picks bit-equal to
    the C oracle, as tests/test_gpu_geometry.py holds them"""
    from oracle import oracle as O
    L, lib = _lib()
    G = _own_grid("sampling.hip", r"prefix_rows_kernel, dim3\(b < (\d+) \? b : \1\)")
    b, n, m = 3001, 70, 7
    assert G < b < 2 * G, "prob_sample: %d rows on a grid of %d" % (b, G)
    print("grid-cap prob_sample: G = %d workgroups, T = %d rows" % (G, b))
    rng = np.random.default_rng(n)
    w = (rng.random((b, n)) ** 3).astype(np.float32)
    r = rng.random((b, m)).astype(np.float32)
    temp, out = nanf(b, n), senti(b, m)
    assert lib.gspn_probsample(b, n, m, P(dev(w)), P(dev(r)), P(temp), P(out), ST()) == 0
    verdict("prob_sample prefix sums", temp, O.cumsum(w), 0.0, G * n)
    assert np.array_equal(temp.cpu().numpy().view(np.uint32), O.cumsum(w).view(np.uint32))
    verdict("prob_sample picks", out, O.prob_sample(w, r), 0.0, G * m)
