"""The shared MLP, the stand-alone batch norm, the transposed convolution and the head layers on poisoned, guard-banded allocations
(tests/arena.py; the table's rules are those of tests/test_gpu_arena_geometry.py).

Every stack is rebuilt from the same seed in each of the four runs, so the moving statistics it updates in place start equal; a case
returns the output, x.grad, every parameter gradient and every moving statistic.  No row is masked and none takes a tolerance: the
header and DESIGN.md document every path here as repeating its bits.  That includes the two four_byte_aligned_* stacks, which do run
fp32 atomics: mlp_bwd_wgrad_kernel (mlp.hip:1707), the kernel wgrad_choose takes for an operand that is only 4-byte aligned, always
adds its partial tiles into zero-filled slots -- but with nslots == nch (below the plan's 12 MiB cap) every address receives exactly
one add onto zero, so the bits repeat.  The streaming kernel's atomics (mlp.hip:2088) start beyond 64 MiB of partial tiles.

The backward workspaces are exactly gspn_mlp_bwd_work_bytes long (mlp.py allocated four floats more until these cases showed that no
kernel touches them)."""
import pytest
import torch

from tests.arena import Case, sweep
from tests.test_gpu_mlp import make_params, place_grad, place_x, to_layers

pytestmark = pytest.mark.gpu

CASES = []
T, F = True, False


def case(fn):
    CASES.append(fn)
    return fn


def leaf(t):
    return t.detach().requires_grad_(True)


def rand(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


# ---- mlp_stack -----------------------------------------------------------------------------------------------------------------------
def stack_case(name, rows, ld, cin, chans, ns, training=True, bn=True, place=None, backward=True):
    """rows x (ld >= cin) input, pad columns zero as the callers leave them; a random grad_output.  place='all': every operand 4-byte
    aligned only, as tests/test_gpu_mlp.py places them (its misaligned() allocates through torch.empty, so under the arena too)."""
    from gspn_amd.mlp import mlp_stack
    x0 = rand(rows, ld, seed=rows + cin)
    if ld > cin:
        x0[:, cin:] = 0.0
    orows = rows // ns if ns else rows
    go0 = rand(orows, chans[-1], seed=7)

    def run():
        layers = to_layers(make_params(chans, cin, 3, bn=bn), place)
        x = place_x(x0.clone(), place) if backward else x0
        out = mlp_stack(x, cin, layers, training, 0.7, pool_ns=ns)
        res = {"out": out.detach()}
        if backward:
            out.backward(place_grad(go0.clone(), place))
            assert x.grad is not None and all(t.grad is not None for lp in layers for t in lp.tensors())
            res["dx"] = x.grad
            res["grads"] = [[t.grad for t in lp.tensors()] for lp in layers]
        res["moving"] = [[lp.moving_mean, lp.moving_variance] for lp in layers if lp.bn]
        return res
    return Case(name, run)


STACKS = [
    # name, rows, ld, cin, chans, pool_ns, training, bn, place          (shapes: tests/test_gpu_mlp.py, test_gpu_mlp_instances.py, test_gpu_mlp_mixed_bn.py)
    ("generic_ragged_rows", 3000, 20, 20, [24, 40, 16], None, T, T, None),               # rows no multiple of any tile, streaming + generic kernels
    ("pooled_top_layer_ns32", 4096, 32, 32, [32, 64, 48], 32, T, T, None),               # the pooled top layer, early coefficients
    ("k_tail_cin67", 2048 + 32, 68, 67, [64, 128], None, T, T, None),                    # cin % 4 != 0 behind a 16-byte pitch
    ("wide_pooled_cin131", 1024, 132, 131, [128, 256], 32, T, T, None),
    ("first_layer_cin6_pool", 4096, 8, 6, [36, 20], 32, T, T, None),                     # mlp_fwd_stream_kernel<64, 4, false, true>
    ("short_kernels", 8192, 64, 64, [320, 64], None, T, T, None),                        # fwd_short_kernel<KW, 1, 2> then <KW, 1, 1>
    ("short_two_row_tiles", 8192, 64, 64, [288], None, T, T, None),                      # fwd_short_kernel<KW, 2, 1>: workgroups without a tile
    ("lean_64_columns", 32768, 64, 64, [32, 32], None, T, T, None),                      # bwd_lean_kernel<2, 0, false, true>
    ("long_fused_backward", 65536, 20, 20, [64, 64, 64], None, T, T, None),              # gspn_mlp_bwd_fused twice, the dense top layer's pre-pass
    ("long_fused_backward_pooled", 65536, 8, 6, [64, 128], 32, T, T, None),              # the pooled (ns = 32) top layer through the fused launch
    ("mixed_bn_TFT", 4096, 8, 6, [32, 32, 64], 32, T, [T, F, T], None),
    ("mixed_bn_FTF", 1000, 68, 67, [64, 64, 64], None, T, [F, T, F], None),
    ("no_bn", 1000, 68, 67, [64, 64], None, T, F, None),
    ("four_byte_aligned_operands", 3000, 20, 20, [24, 40, 16], None, T, T, "all"),
    ("four_byte_aligned_pooled", 4096, 32, 32, [32, 64, 48], 32, T, T, "all"),
    ("inference_forward", 3000, 20, 20, [24, 40, 16], None, F, T, None),
    ("inference_forward_pooled", 4096, 32, 32, [32, 64, 48], 32, F, T, None),
    ("inference_backward", 4096, 4, 3, [32, 32], 256, F, T, None),                       # bwd_lean_kernel<1, 2, false, true>: pool groups >= 128 rows
]


def _stack(row):
    name, rows, ld, cin, chans, ns, training, bn, place = row

    def build():
        return stack_case("mlp_stack %s rows=%d cin=%d %s pool=%s training=%s bn=%s place=%s" % (name, rows, cin, chans, ns, training, bn, place),
                          rows, ld, cin, chans, ns, training, bn, place, backward=name not in ("inference_forward", "inference_forward_pooled"))
    build.__name__ = "mlp_stack_" + name
    return build


for _row in STACKS:
    case(_stack(_row))


@case
def mlp_linear():
    from gspn_amd.mlp import LayerParams, mlp_linear
    x0, go = rand(1000, 68, seed=1), rand(1000, 36, seed=2)
    x0[:, 67:] = 0.0
    w0, b0 = rand(67, 36, seed=3, scale=0.1), rand(36, seed=4)

    def run():
        x, w, b = leaf(x0), leaf(w0), leaf(b0)
        y = mlp_linear(x, 67, LayerParams(w, b, False))
        y.backward(go)
        return y.detach(), x.grad, w.grad, b.grad
    return Case("mlp_linear rows=1000 cin=67 (ld 68) cout=36 + backward", run)


def _sa_module(name, c, training):
    """pointnet_sa_module: c = 3 features take the gathered first layer, c = 64 the pre-aggregated one (training mode, mlp.PREAGG_MIN_C)"""
    from gspn_amd.pointnet_util import pointnet_sa_module
    from tests import data as D
    from tests.test_gpu_modules import fresh_store
    b, n, npoint, ns = 2, 1024, 128, 32
    xyz = torch.from_numpy(D.batch("U", b, n, 9)).cuda()
    pts0 = rand(b, n, c, seed=c)
    go = rand(b, npoint, 64, seed=5)

    def run():
        store = fresh_store(31)
        pts = leaf(pts0)
        new_xyz, out, idx = pointnet_sa_module(xyz, pts, npoint, 0.2, ns, [32, 32, 64], None, False, training, 0.5, 'sa')
        out.backward(go)
        names = sorted(store.vars)
        return {"new_xyz": new_xyz, "out": out.detach(), "idx": idx, "dpoints": pts.grad,
                "grads": [store.vars[k].grad for k in names if store.vars[k].grad is not None],
                "moving": [store.vars[k] for k in names if "moving" in k]}
    return Case("pointnet_sa_module %s c=%d training=%s" % (name, c, training), run)


@case
def sa_module_gathered_first_layer():
    return _sa_module("gathered first layer", 3, True)


@case
def sa_module_preaggregated_first_layer():
    return _sa_module("pre-aggregated first layer", 64, True)


@case
def sa_module_gathered_first_layer_eval():
    return _sa_module("gathered first layer", 64, False)


@case
def fp_module_preaggregated():
    from gspn_amd.pointnet_util import pointnet_fp_module
    from tests import data as D
    from tests.test_gpu_modules import fresh_store
    xyz1, xyz2 = torch.from_numpy(D.batch("D", 2, 900, 4)).cuda(), torch.from_numpy(D.batch("D", 2, 200, 5)).cuda()
    p1_0, p2_0, go = rand(2, 900, 3, seed=1), rand(2, 200, 32, seed=2), rand(2, 900, 16, seed=3)

    def run():
        store = fresh_store(21)
        p1, p2 = leaf(p1_0), leaf(p2_0)
        out = pointnet_fp_module(xyz1, xyz2, p1, p2, [32, 16], True, 0.5, 'fa')
        out.backward(go)
        names = sorted(store.vars)
        return {"out": out.detach(), "d1": p1.grad, "d2": p2.grad, "grads": [store.vars[k].grad for k in names if store.vars[k].grad is not None],
                "moving": [store.vars[k] for k in names if "moving" in k]}
    return Case("pointnet_fp_module 900 <- 200, c2=32 c1=3 (pre-aggregated first layer, CSR-split transpose)", run)


# ---- the stand-alone batch norm ------------------------------------------------------------------------------------------------------
def _batch_norm(rows, c, training):
    from gspn_amd.tf_util import _BatchNormRows
    x0, go = rand(rows, c, seed=rows) + 3.0, rand(rows, c, seed=c)
    g0, b0 = torch.rand(c, generator=torch.Generator().manual_seed(1)).cuda() + 0.5, rand(c, seed=2)
    mm0, mv0 = rand(c, seed=3, scale=0.1), torch.rand(c, generator=torch.Generator().manual_seed(4)).cuda() + 0.5

    def run():
        x, g, b, mm, mv = leaf(x0), leaf(g0), leaf(b0), mm0.clone(), mv0.clone()
        y = _BatchNormRows.apply(x, g, b, mm, mv, training, 0.7)
        y.backward(go)
        return y.detach(), x.grad, g.grad, b.grad, mm, mv
    return Case("tf_util batch norm rows=%d c=%d training=%s, forward and backward" % (rows, c, training), run)


@case
def batch_norm_train():
    return _batch_norm(513, 37, True)


@case
def batch_norm_eval():
    return _batch_norm(513, 37, False)


@case
def batch_norm_train_wide():
    return _batch_norm(3 * 129, 1000, True)


# ---- conv2d_transpose ------------------------------------------------------------------------------------------------------------------
def _deconv(shape):
    from gspn_amd.deconv import conv2d_transpose_valid, deconv_out_size
    n, hi, wi, cin, cout, kh, kw, sh, sw = shape
    x0, k0, b0 = rand(n, hi, wi, cin, seed=1), rand(kh, kw, cout, cin, seed=2, scale=0.1), rand(cout, seed=3)
    dy = rand(n, deconv_out_size(hi, sh, kh), deconv_out_size(wi, sw, kw), cout, seed=4)

    def run():
        x, k, b = leaf(x0), leaf(k0), leaf(b0)
        y = conv2d_transpose_valid(x, k, b, (sh, sw))
        y.backward(dy)
        return y.detach(), x.grad, k.grad, b.grad
    return Case("conv2d_transpose %s forward, input and kernel gradients" % (shape,), run)


@case
def deconv_odd():
    return _deconv((3, 5, 5, 3, 5, 2, 2, 3, 3))


@case
def deconv_decoder():
    return _deconv((64, 3, 3, 512, 256, 3, 3, 2, 2))          # decoding_net's second up-convolution, at 64 decodes instead of 512


@case
def deconv_decoder_last():
    return _deconv((64, 16, 16, 128, 3, 1, 1, 1, 1))


# ---- the head layers -----------------------------------------------------------------------------------------------------------------
def _crop_linear(shape, normalize=True):
    from tests import heads_ref as HR
    from tests.test_gpu_heads import run_crop_linear
    b, n, c, r, p, cout = shape
    case_ = HR.crop_linear_case(*shape, seed=2)
    dy = torch.randn(b, r, p, cout, generator=torch.Generator().manual_seed(7))

    def run():
        y, grads = run_crop_linear(case_, normalize, dy)
        return y.detach(), grads
    return Case("crop_linear %s normalize=%s forward and the four gradients" % (shape, normalize), run)


@case
def crop_linear_smallest():
    return _crop_linear((1, 7, 8, 2, 5, 4))


@case
def crop_linear_dead_lanes_cout12():
    return _crop_linear((2, 50, 8, 3, 33, 12), False)


@case
def crop_linear_second_tile():
    return _crop_linear((2, 64, 4, 130, 257, 12))             # more tiles than CL_MAX_PARTS workgroups, a last tile of 4 rows


@case
def tile_add_tile_sum():
    from gspn_amd.heads import _TileAdd

    def one(groups, p, c):
        a0, g0, dy = rand(groups * p, c, seed=p), rand(groups, c, seed=c), rand(groups * p, c, seed=groups)

        def run():
            a, g = leaf(a0), leaf(g0)
            y = _TileAdd.apply(a, g, p)
            y.backward(dy)
            return y.detach(), a.grad, g.grad
        return run
    runs = [one(*s) for s in [(1, 1, 4), (7, 3, 20), (3, 256, 256), (2, 130, 260)]]      # tests/test_gpu_tile_linear.py: with and without the join kernel
    return Case("tile_add and tile_sum (its gradient) at (1,1,4) (7,3,20) (3,256,256) (2,130,260)", lambda: [r() for r in runs])


@case
def tile_linear():
    from tests.test_gpu_tile_linear import run_tile_linear, tile_linear_case
    cases = [(tile_linear_case(*s, seed=5), s[1]) for s in [(3, 5, 8, 4, 8), (2, 16, 12, 20, 36)]]
    return Case("tile_linear (3,5,8,4,8) and (2,16,12,20,36) + gradients", lambda: [run_tile_linear(c, p) for c, p in cases])


def _seg_head(training):
    from tests import test_gpu_heads as TH
    from tests.test_gpu_modules import fresh_store
    from tests.test_gpu_tile_linear import run_seg
    b, r, p, c = 2, 3, 16, 20
    crop = TH.crop_inputs(b, 200, c, r, p, seed=7)
    dmask = rand(b, r, p, TH.NCAT, seed=8)

    def run():
        store = fresh_store(31)
        masks = run_seg(None, None, training, crop=crop, split_post=True)
        grads = torch.autograd.grad((masks * dmask).sum(), store.parameters())
        return masks.detach(), list(grads), [store.vars[k] for k in sorted(store.vars) if "moving" in k]
    return Case("segmentation_head through the crop with the tile-linear split post layer, training=%s" % training, run)


@case
def seg_head_split_post_train():
    return _seg_head(True)


@case
def seg_head_split_post_eval():
    return _seg_head(False)


@case
def crop_mean():
    from gspn_amd.inference import crop_mean
    from tests import heads_ref as HR
    _, fea, _, _, idx, _, _ = HR.crop_linear_case(2, 300, 19, 5, 33, 4, seed=3)
    table, idx = fea.cuda(), idx.cuda()
    wide = rand(2, 300, 64, seed=6)
    return Case("crop_mean c=19 and c=64 over (2, 5, 33) indices", lambda: (crop_mean(table, idx), crop_mean(wide, idx)))


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
MASKED = set()          # names of the rows that carry a mask or a canonical form: none here


@pytest.mark.parametrize("build", CASES, ids=lambda f: f.__name__)
def test_arena(build):
    c = build()
    assert c.masked == (build.__name__ in MASKED)
    sweep(c)


def test_zz_masked_cases():
    print("\ntests/test_gpu_arena_layers.py: %d cases, %d masked" % (len(CASES), len(MASKED)))
    assert not MASKED
