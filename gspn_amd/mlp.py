"""Shared-MLP stack on the MFMA kernels (C ABI gspn_mlp_* / gspn_bn_*).

One `conv2d(1x1) + bias + batch_norm + relu` layer of utils/tf_util.py:120-185 over a
(batch, npoint, nsample, C) tensor is a row-major GEMM over rows = batch*npoint*nsample.
`mlp_stack` runs a whole `for num_out_channel in mlp:` loop of pointnet_util.py:109-113 (and the
reduce_max of :123-124 when `pool_ns` is given) as one autograd node: pre-BN activations are written
once, the BN+ReLU of layer l is applied inside the operand load of layer l+1, and backward rebuilds
dY on the fly inside the two backward GEMMs.
"""
import collections
import ctypes
import os
import types

import torch

from . import _lib as L
from ._args import _typed

BN_EPS = 1e-3      # tf.contrib.layers.batch_norm default epsilon (tf_util.py:529-534 passes none)

# The last kernel of a layer's weight-gradient pass (the double-precision sum over partial tiles) has no consumer before the
# optimiser and cannot fill the chip (latency-bound); DEFER_DW = True puts it on a side stream where it overlaps the next layer's
# kernels.  Off by default: inside a captured step the fork becomes a multi-branch hipGraph, and ROCm 7.2 replays those far slower
# than a linear graph (measured on MI355X: 3.9 -> 6.6 ms per step), which costs more than the ~0.2 ms of overlap gains.
DEFER_DW = os.environ.get("GSPN_DEFER_DW", "0") == "1"
# max-pool over nsample = 32 rows taken from the last layer's accumulators (gspn_mlp_fwd_pool32 + gspn_pool32_select) instead of a pass
# over the (rows, c) output
FUSE_POOL32 = os.environ.get("GSPN_FUSE_POOL32", "1") != "0"
# the same for pools over a multiple of 32 rows (the proposal head's 256 / 512): tile maxima from the forward launch + gspn_pool32_select_groups
FUSE_POOLN = os.environ.get("GSPN_FUSE_POOLN", "1") != "0"
# early coefficients (mlp.hip, "Early coefficients"): the BN reductions of a layer are taken before its pass A -- by the epilogue of the
# next layer's pass B, or from the pool arg-max for the top layer of a pooled stack -- so that pass A is one GEMM instead of two
EARLY_R = os.environ.get("GSPN_EARLY_R", "1") != "0"
# pre-aggregated first layer (mlp.hip, "Pre-aggregated first layer"): the feature part of an SA / FP module's first layer is multiplied on the
# source points, the grouped / interpolated rows are formed from the product.  Training-mode BN stacks with early coefficients only.
PREAGG = os.environ.get("GSPN_PREAGG", "1") != "0"
PREAGG_MIN_C = int(os.environ.get("GSPN_PREAGG_MIN_C", "16"))      # below this many feature columns the grouped GEMM is as cheap
# pass B of a pooled top layer as a streaming GEMM on the layer's INPUT (gspn_mlp_bwd_data_pooltop): its (rows, cout) output is not read
POOLTOP_STREAM = os.environ.get("GSPN_POOLTOP_STREAM", "1") != "0"
# one launch for pass B + the dW reduction of the same layer (gspn_mlp_bwd_data with a gspn_dw_args) instead of two
FUSE_DW = os.environ.get("GSPN_FUSE_DW", "1") != "0"
# pass A and pass B of a layer in one launch where the library has the kernel for the shape (gspn_mlp_bwd_fused: both products from one staged
# dY tile)
FUSED_BWD = os.environ.get("GSPN_FUSED_BWD", "1") != "0"
POOLTOP_FUSED = os.environ.get("GSPN_POOLTOP_FUSED", "1") != "0"
FUSED_COEF = os.environ.get("GSPN_FUSED_COEF", "1") != "0"          # r04: the coefficient kernel after a fused launch carries that launch's dW reduction       # the pooled (nsample = 32) top layer through the fused launch as well
# the top layer of a stack with a dense upstream gradient takes its BN reductions in a streaming pre-pass (gspn_dense_rsum) from this many rows on
DENSE_TOP_RSUM = os.environ.get("GSPN_DENSE_TOP_RSUM", "1") != "0"
DENSE_TOP_MIN_ROWS = int(os.environ.get("GSPN_DENSE_TOP_MIN_ROWS", "65536"))
_side_streams = {}

# Optional SyncBN: batch statistics over the global batch of all ranks instead of per replica -- what the single-GPU reference
# computes.  Off by default (standard data parallelism); when on, and torch.distributed has more than one rank, training-mode
# batch-normalised stacks run layer by layer: the GEMM kernel of the linear layer, then parallel.sync_bn_relu (two small all-reduces per
# layer).  Slower than the fused kernels; results equal a single-process run on the concatenated batch (tests/test_cpu_dist.py).
SYNC_BN = False
# r04: SyncBN ON the fused kernels.  Every batch-norm reduction of the stack already leaves the kernels as per-workgroup partial rows that a
# small kernel sums (gspn_bn_finalize*, gspn_mlp_bwd_coef): with equal shards the ranks' partial buffers have the same shape, so ONE
# all-reduce(SUM) of that buffer between the producing kernel and the summing kernel turns every local sum into the global one; the
# summing kernel then runs with rows x world.  Same kernels, same hipGraph, two small collectives per layer.  Needs: equal rows on every
# rank (weak scaling), training-mode BN on every layer, coefficients that come from partial rows everywhere (EARLY_R; the dense top
# layer's reductions always through gspn_dense_rsum).  SYNC_BN_FUSED = False restores round 2's layer-by-layer torch form.
SYNC_BN_FUSED = os.environ.get("GSPN_SYNC_BN_FUSED", "1") != "0"


def _sync_world(stack_ok=True):
    """world size over which the fused kernels' BN reductions are all-reduced (1: no SyncBN, or a single rank)"""
    if not (SYNC_BN and SYNC_BN_FUSED and stack_ok):
        return 1
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def _allreduce_sum(t):
    import torch.distributed as dist
    dist.all_reduce(t, op=dist.ReduceOp.SUM)

# bench.py sets this to a list to collect (kind, rows, cin, cout, start_event, end_event) around every GEMM-kernel launch of the stack
# ("fwd", "wgrad" = pass A incl. its finalize kernels, "bwd" = pass B (+ the dW reduction riding in it)); None = no events
PROFILE = None


def _tic():
    if PROFILE is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _toc(e0, kind, rows, cin, cout, executed=None):
    """executed: multiply-add flops the launches between the two events really issue when that differs from the algorithmic
    2*rows*cin*cout of the layer (pre-aggregated first layers run their feature part on the source rows; the two-product pass A
    runs two GEMMs; pass B of a first layer may cover only the columns that carry a gradient)"""
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        PROFILE.append((kind, rows, cin, cout, e0, e1, 2.0 * rows * cin * cout if executed is None else float(executed)))


def _side_stream(dev):
    key = (dev.type, dev.index)
    s = _side_streams.get(key)
    if s is None:
        s = _side_streams[key] = torch.cuda.Stream(device=dev)
    return s


class LayerParams:
    """Variables of one conv2d scope (tf_util.py:159-183): weights (cin,cout) [= the (1,1,cin,cout) kernel],
    biases, and under bn: beta, gamma, moving_mean, moving_variance."""

    def __init__(self, weights, biases, bn=True, beta=None, gamma=None, moving_mean=None, moving_variance=None):
        self.weights, self.biases, self.bn = weights, biases, bn
        self.beta, self.gamma, self.moving_mean, self.moving_variance = beta, gamma, moving_mean, moving_variance

    def tensors(self):
        t = [self.weights, self.biases]
        if self.bn:
            t += [self.beta, self.gamma]
        return t


def _label(what, i):
    return what if i is None else "%s: layer %d" % (what, i)


def _vector_typed(t, cout, updated, what, i, name):
    """one per-channel tensor of a layer: float32, 1-D, cout long; a moving statistic (`updated`) contiguous besides.  (The label is put
    together only when a rule fails: this runs for every layer tensor on every call.)"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1:
        _typed(t, torch.float32, 1, "%s: %s" % (_label(what, i), name))
    if t.shape[0] != cout:
        raise ValueError("%s: %s must have cout = %d elements, got %d" % (_label(what, i), name, cout, t.shape[0]))
    if updated and not t.is_contiguous():
        # updated in place through its data pointer: a copy would take the update, a strided write would land somewhere else
        raise ValueError("%s: %s is updated in place and must be contiguous, got strides %s" % (_label(what, i), name, tuple(t.stride())))


def _on_device(t, dev, what, i, name):
    if t.device != dev:
        raise L.GspnHipError("%s: %s is on %s, the input on %s" % (_label(what, i), name, t.device, dev))


def layer_typed(lp, cin, what, i=None):
    """dtype, rank and shape rules of one LayerParams (ValueError wherever the tensors live, like _args._typed) -> cout"""
    w = lp.weights
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 2:
        _typed(w, torch.float32, 2, "%s: weights" % _label(what, i))
    if cin is not None and w.shape[0] != cin:
        raise ValueError("%s: weights must be (cin, cout) = (%d, cout), got %s" % (_label(what, i), cin, tuple(w.shape)))
    cout = w.shape[1]
    _vector_typed(lp.biases, cout, False, what, i, "biases")
    if lp.bn:
        _vector_typed(lp.beta, cout, False, what, i, "beta")
        _vector_typed(lp.gamma, cout, False, what, i, "gamma")
        _vector_typed(lp.moving_mean, cout, True, what, i, "moving_mean")
        _vector_typed(lp.moving_variance, cout, True, what, i, "moving_variance")
    return cout


def layer_on_device(lp, dev, what, i=None):
    """the device rule, after the shape rules: every tensor of the layer on `dev` (GspnHipError, like L.need) -> a LayerParams whose tensors the
    kernels can read through a bare pointer.  A non-contiguous weight / bias / beta / gamma (a .t() view, a slice of a wider buffer) is
    copied here, under autograd: the gradient the stack computes for the copy reaches the caller's tensor with that tensor's shape and
    strides.  The copy is a new allocation, so it never matches a gradient sink: such a gradient goes through autograd."""
    _on_device(lp.weights, dev, what, i, "weights")
    _on_device(lp.biases, dev, what, i, "biases")
    contiguous = lp.weights.is_contiguous() and lp.biases.is_contiguous()
    if lp.bn:
        for name in ("beta", "gamma", "moving_mean", "moving_variance"):
            _on_device(getattr(lp, name), dev, what, i, name)
        contiguous = contiguous and lp.beta.is_contiguous() and lp.gamma.is_contiguous()
    if contiguous:
        return lp
    return LayerParams(lp.weights.contiguous(), lp.biases.contiguous(), lp.bn, lp.beta.contiguous() if lp.bn else None,
                       lp.gamma.contiguous() if lp.bn else None, lp.moving_mean, lp.moving_variance)


def checked_layers(x, ndim, layers, cin, what):
    """The argument rules of everything that hands LayerParams to the library (mlp_stack, mlp_linear, tf_util's wide-input layer): dtype,
    rank and shape of x and of every layer tensor first (ValueError), then the device rule (GspnHipError) -> (x contiguous, layers with
    contiguous tensors).  cin: the first layer's input width (None: not checked); each later layer takes the width the one before it gives."""
    _typed(x, torch.float32, ndim, "x")
    for i, lp in enumerate(layers):
        cin = layer_typed(lp, cin, what, i)
    x = L.need(x, torch.float32, ndim, "x")
    return x, [layer_on_device(lp, x.device, what, i) for i, lp in enumerate(layers)]


def checked_bn(x, gamma, beta, moving_mean, moving_variance, what):
    """the same rules for a stand-alone batch norm over the rows of x (rows, c) -> (x, gamma, beta) contiguous; the moving statistics, which
    the kernels update in place, must be contiguous as they are"""
    _typed(x, torch.float32, 2, "x")
    named = (("gamma", gamma, False), ("beta", beta, False), ("moving_mean", moving_mean, True), ("moving_variance", moving_variance, True))
    for name, t, updated in named:
        _vector_typed(t, x.shape[1], updated, what, None, name)
    x = L.need(x, torch.float32, 2, "x")
    for name, t, _ in named:
        _on_device(t, x.device, what, None, name)
    return x, gamma.contiguous(), beta.contiguous()


# ---- gradient sinks (r06) ---------------------------------------------------------------------------------------------------------
# A caller that keeps all parameter gradients in ONE flat buffer (parallel.FlatGradBucket: the operand of the gradient all-reduce and of the
# one-launch Adam) can register, per parameter, the slice of that buffer its gradient belongs in (FlatGradBucket.attach_sinks()).  The backward
# pass of a stack then lets its reduction kernels write dW / dbias / dbeta / dgamma STRAIGHT into those slices and returns None to autograd for
# them: no per-step `cat` of ~60 gradient tensors into the bucket (the last library kernel inside the captured step but autograd's two gradient
# accumulations).  Keyed by the parameter's data pointer (LayerParams.weights is a fresh VIEW of the stored kernel on every forward); an entry
# holds a weak reference to the stored parameter and dies with it.  A parameter used by two stacks in one backward pass is written once; its
# .grad is the slice from then on, so the second gradient, which goes through autograd, is added to the slice by autograd's own accumulation.
# The rules of a claim -- frozen parameters, abandoned steps, torch.autograd.grad -- are FlatGradBucket's docstring and DESIGN.md 4.5.
GRAD_SINKS = {}


class _Sink:
    __slots__ = ("bucket", "index", "view", "ref")

    def __init__(self, bucket, index, view, ref):
        self.bucket, self.index, self.view, self.ref = bucket, index, view, ref


def _delivers_grad(base):
    """does the backward pass that is running accumulate into base.grad?  torch.autograd.grad() and backward(inputs=...) without `base`
    do not: a gradient written into the bucket would be lost to the caller, so such a pass gets its gradients through autograd.
    Asks the engine (torch._C._will_engine_execute_node on the parameter's AccumulateGrad node: a private call, probed once by
    FlatGradBucket.attach_sinks()).  Under torch.autograd.grad the engine refuses the question for a leaf with a RuntimeError that names
    autograd.grad: only that error means "no"; any other is raised."""
    with torch.enable_grad():
        acc = base.view_as(base).grad_fn.next_functions[0][0]
    try:
        return bool(torch._C._will_engine_execute_node(acc))
    except RuntimeError as e:
        if "autograd.grad" in str(e):
            return False
        raise


def probe_engine_query():
    """attach_sinks() calls this once: a plain backward() must answer True for a leaf, or sinks would switch themselves off silently (or
    claim under torch.autograd.grad) after a torch update.  CPU tensors, no launch."""
    seen = []
    w = torch.ones(1, requires_grad=True)

    def product():
        y = w * 2.0
        y.register_hook(lambda g: seen.append(_delivers_grad(w)))       # (runs inside the backward pass, like a node's backward)
        return y.sum()

    product().backward()
    torch.autograd.grad(product(), [w])
    if seen != [True, False]:
        raise L.GspnHipError("gradient sinks: torch's engine no longer tells backward() from autograd.grad() (got %s): sinks cannot be attached" % seen)


def _grad_buffer(param, sunk):
    """where the gradient of `param` is to be written: its registered bucket slice (first gradient since the parameter's .grad was last
    reset) or a fresh tensor.  A claim shows on the parameter: its .grad becomes the slice.  Whatever autograd delivers afterwards -- a second
    use of the layer, a second backward pass -- is then added to the slice by autograd itself; a .grad that was reset since (None, or another
    tensor) marks the claim as one of an abandoned step, and the slice is claimed again and overwritten.  A parameter that does not require a
    gradient gets a scratch tensor and no claim: its slice stays zero."""
    e = GRAD_SINKS.get(param.data_ptr())
    if e is not None:
        base = e.ref()
        if base is None or base.data_ptr() != param.data_ptr() or base.numel() != param.numel():
            GRAD_SINKS.pop(param.data_ptr(), None)                 # the parameter is gone (or moved): never write through a stale entry
        elif param.requires_grad and base.requires_grad and param.dtype == torch.float32 and param.is_contiguous():
            g = base.grad
            mine = g is not None and g.data_ptr() == e.view.data_ptr() and g.numel() == e.view.numel()
            if (g is None or mine) and not (mine and e.index in e.bucket._written) and _delivers_grad(base):
                e.bucket._written.add(e.index)
                base.grad = e.view.view(base.shape)
                v = e.view.view(param.shape)
                sunk.add(v.data_ptr())
                return v
    return torch.empty_like(param)


def _grad_release(param, buf, sunk):
    """undo _grad_buffer(param, sunk) for a launch that declined before it wrote `buf`: the slice is claimable again, so whichever launch does
    produce the gradient writes it there (a slot left claimed but unwritten would get that gradient ADDED by autograd, onto whatever the
    slice held -- the previous step's gradient)"""
    if buf.data_ptr() in sunk:
        e = GRAD_SINKS.get(param.data_ptr())
        if e is not None:
            e.bucket._written.discard(e.index)
            base = e.ref()
            if base is not None and base.grad is not None and base.grad.data_ptr() == e.view.data_ptr():
                base.grad = None
        sunk.discard(buf.data_ptr())


# what the forward pass keeps of one layer for backward: its input x (rows, ldx) (None when the rows are virtual) with the scale / shift
# applied while loading it, its pre-BN output y, the statistics it normalised with and its own forward scale / shift
_Saved = collections.namedtuple("_Saved", "x ldx cin in_scale in_shift y mean var scale shift")


def _zeros(n, dev, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype, device=dev)


class _MlpStack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cin0, spec, *params):
        """x: (rows, ld) float32 contiguous; spec: dict(layers=[LayerParams], is_training, decay, pool_ns);
        params: flat list of the differentiable tensors (w, b[, beta, gamma]) per layer, for autograd."""
        lib = L.lib()
        dev = x.device
        gather = spec.get("gather")              # fused SA front end: x is the (b*n, ldf) feature matrix, the GEMM rows are virtual
        if gather is not None:
            rows, ld = gather["rows"], 0
            ga = L.GatherArgs(x.data_ptr(), x.shape[1], gather["c"], gather["gidx"].data_ptr(), gather["rel"].data_ptr(), int(gather["xyz_first"]))
            ctx.gargs = ga
            ctx.gather_x = x                     # the backward pass gathers from it again: keep the storage alive
        else:
            rows, ld = x.shape
        pre = spec.get("preagg")                 # pre-aggregated first layer: x is the (source rows, ldf) feature matrix
        if pre is not None:
            rows, ld = pre["rows"], 0
            ctx.pre_x = x
        layers = spec["layers"]
        is_training = bool(spec["is_training"])
        decay = float(spec["decay"])
        pool_ns = spec["pool_ns"]
        sw = _sync_world(is_training) if spec.get("sync_bn") else 1          # > 1: BN statistics over the global batch (fused SyncBN)
        saved = []
        cur, cur_ld, cin = x, ld, cin0
        in_scale = in_shift = None
        pool = None                              # (vmax, amax) of the last layer when the pool rides in its forward epilogue
        with torch.cuda.device(dev):
            st = L.stream()                      # the current stream of x's device (not of whatever device was current outside)
            for li, lp in enumerate(layers):
                cout = lp.weights.shape[1]
                y = torch.empty((rows, cout), dtype=torch.float32, device=dev)
                use_stats = lp.bn and is_training
                pre0 = pre if li == 0 else None
                if pre0 is not None:
                    nparts0 = int(lib.gspn_preagg_fwd_parts(rows, cout))
                    stats = torch.empty(nparts0 * 2 * cout, dtype=torch.float32, device=dev) if use_stats else None
                else:
                    stats = torch.empty(int(lib.gspn_mlp_fwd_stats_bytes(rows, cout)) // 4, dtype=torch.float32, device=dev) if use_stats else None
                ev = _tic()
                if (FUSE_POOL32 and pool_ns and (pool_ns == 32 or (FUSE_POOLN and pool_ns % 32 == 0 and lp.weights.shape[1] % 4 == 0)) and li == len(layers) - 1 and rows % 32 == 0
                        and not (li == 0 and (pre is not None or gather is not None))):      # (a one-layer stack with a gathered / pre-aggregated input has no plain forward)
                    g32 = rows // 32
                    pool = (torch.empty((g32, cout), dtype=torch.float32, device=dev), torch.empty((g32, cout), dtype=torch.int32, device=dev))
                    try:
                        L.check(lib.gspn_mlp_fwd_pool32(rows, cin, cout, L.ptr(cur), cur_ld, L.ptr(in_scale), L.ptr(in_shift), L.ptr(lp.weights),
                                                        L.ptr(lp.biases), L.ptr(y), cout, L.ptr(stats), L.ptr(pool[0]), L.ptr(pool[1]), st),
                                "mlp_fwd_pool32")
                    except NotImplementedError:          # a shape / alignment without a pool epilogue: plain forward, the stand-alone pool below
                        pool = None
                        L.check(lib.gspn_mlp_fwd(rows, cin, cout, L.ptr(cur), cur_ld, L.ptr(in_scale), L.ptr(in_shift),
                                                 L.ptr(lp.weights), L.ptr(lp.biases), L.ptr(y), cout, L.ptr(stats), st), "mlp_fwd")
                elif li == 0 and pre is not None:
                    # F = feat . W_feat on the source rows, then the output rows from F (+ side . W_side + bias) and their column sums
                    wf = lp.weights[pre["wf0"]:pre["wf0"] + pre["c"]]
                    ws = lp.weights[pre["ws0"]:pre["ws0"] + pre["side_n"]]
                    fsrc = torch.empty((x.shape[0], cout), dtype=torch.float32, device=dev)
                    L.check(lib.gspn_mlp_fwd(x.shape[0], pre["c"], cout, L.ptr(x), x.shape[1], None, None, L.ptr(wf), None, L.ptr(fsrc), cout, None, st),
                            "mlp_fwd(pre-aggregation)")
                    L.check(lib.gspn_preagg_fwd(rows, cout, pre["T"], L.ptr(fsrc), L.ptr(pre["idx"]), L.ptr(pre["w"]), pre["per_scene_rows"],
                                                pre["per_scene_src"], L.ptr(pre["side"]), pre["side_ld"], pre["side_n"], L.ptr(ws), L.ptr(lp.biases),
                                                L.ptr(y), L.ptr(stats), st), "preagg_fwd")
                elif li == 0 and gather is not None:
                    L.check(lib.gspn_mlp_fwd_gather(rows, ctypes.byref(ga), cout, L.ptr(lp.weights), L.ptr(lp.biases), L.ptr(y), cout, L.ptr(stats), st),
                            "mlp_fwd_gather")
                else:
                    L.check(lib.gspn_mlp_fwd(rows, cin, cout, L.ptr(cur), cur_ld, L.ptr(in_scale), L.ptr(in_shift),
                                             L.ptr(lp.weights), L.ptr(lp.biases), L.ptr(y), cout, L.ptr(stats), st), "mlp_fwd")
                _toc(ev, "fwd", rows, cin, cout,
                     2.0 * cout * (x.shape[0] * pre["c"] + rows * pre["side_n"]) if (li == 0 and pre is not None) else None)
                mean = torch.empty(cout, dtype=torch.float32, device=dev)
                var = torch.empty(cout, dtype=torch.float32, device=dev)
                scale = torch.empty(cout, dtype=torch.float32, device=dev)
                shift = torch.empty(cout, dtype=torch.float32, device=dev)
                if sw > 1 and use_stats:
                    _allreduce_sum(stats)                # every partial row becomes the sum of the ranks' rows: global column sums
                rows_bn = rows * sw
                if lp.bn and pre0 is not None:
                    L.check(lib.gspn_bn_finalize_parts(rows_bn, cout, L.ptr(stats), nparts0, L.ptr(lp.gamma), L.ptr(lp.beta), BN_EPS, decay,
                                                       int(is_training), L.ptr(lp.moving_mean), L.ptr(lp.moving_variance),
                                                       L.ptr(mean), L.ptr(var), L.ptr(scale), L.ptr(shift), st), "bn_finalize")
                elif lp.bn and sw > 1:
                    # (gspn_bn_finalize derives the number of partial rows from `rows`: the local count; the statistics divide by the global one)
                    L.check(lib.gspn_bn_finalize_parts(rows_bn, cout, L.ptr(stats), int(lib.gspn_mlp_fwd_stats_bytes(rows, cout)) // (8 * cout), L.ptr(lp.gamma),
                                                       L.ptr(lp.beta), BN_EPS, decay, int(is_training), L.ptr(lp.moving_mean), L.ptr(lp.moving_variance),
                                                       L.ptr(mean), L.ptr(var), L.ptr(scale), L.ptr(shift), st), "bn_finalize(sync)")
                elif lp.bn:
                    L.check(lib.gspn_bn_finalize(rows, cout, L.ptr(stats), L.ptr(lp.gamma), L.ptr(lp.beta), BN_EPS, decay,
                                                 int(is_training), L.ptr(lp.moving_mean), L.ptr(lp.moving_variance),
                                                 L.ptr(mean), L.ptr(var), L.ptr(scale), L.ptr(shift), st), "bn_finalize")
                else:
                    scale.fill_(1.0)
                    shift.zero_()
                    mean.zero_()
                    var.fill_(1.0)
                saved.append(_Saved(None if (li == 0 and (gather is not None or pre is not None)) else cur, cur_ld, cin, in_scale, in_shift, y, mean, var, scale, shift))
                cur, cur_ld, cin, in_scale, in_shift = y, cout, cout, scale, shift
            cl = cin
            arg = None
            if pool_ns:
                groups = rows // pool_ns
                out = torch.empty((groups, cl), dtype=torch.float32, device=dev)
                arg = torch.empty((groups, cl), dtype=torch.int32, device=dev)
                done = False
                if pool is not None and pool_ns == 32:             # the group extrema came out of the last forward launch: finish on (groups, c) elements
                    try:
                        L.check(lib.gspn_pool32_select(groups, cl, L.ptr(pool[0]), L.ptr(pool[1]), L.ptr(cur), cur_ld,
                                                       L.ptr(in_scale), L.ptr(in_shift), L.ptr(out), L.ptr(arg), st), "pool32_select")
                        done = True
                    except NotImplementedError:
                        pool = None
                elif pool is not None:           # groups of 32 * sub rows: the first largest of the tile maxima
                    yarg = torch.empty((groups, cl), dtype=torch.float32, device=dev)
                    try:
                        L.check(lib.gspn_pool32_select_groups(groups, pool_ns // 32, cl, L.ptr(pool[0]), L.ptr(pool[1]), L.ptr(cur), cur_ld,
                                                              L.ptr(in_scale), L.ptr(in_shift), L.ptr(out), L.ptr(arg), L.ptr(yarg), st), "pool32_select_groups")
                        pool = (yarg, None)
                        done = True
                    except NotImplementedError:  # (the library declined the shape -- the header's contract is "the caller then runs gspn_bnrelu_maxpool")
                        pool = None
                if not done:
                    L.check(lib.gspn_bnrelu_maxpool(groups, pool_ns, cl, L.ptr(cur), cur_ld, L.ptr(in_scale), L.ptr(in_shift),
                                                    L.ptr(out), L.ptr(arg), st), "bnrelu_maxpool")
            else:
                out = torch.empty((rows, cl), dtype=torch.float32, device=dev)
                L.check(lib.gspn_bnrelu_apply(rows, cl, L.ptr(cur), cur_ld, L.ptr(in_scale), L.ptr(in_shift), L.ptr(out), cl, st), "bnrelu_apply")
        ctx.gather = gather
        ctx.pre = pre
        ctx.saved = saved
        # backward re-reads the weights and gamma, the top layer's biases of a pooled stack, the input x -- the feature matrix of the gathered and the
        # pre-aggregated form -- and those forms' index / weight / side tensors: an in-place update between forward and backward would
        # silently change the result (autograd's own check only covers save_for_backward tensors; these are kept as attributes so the
        # layer list stays one object)
        reread = [("x", x)]
        for li, lp in enumerate(layers):
            reread += [("layer %d weights" % li, lp.weights)] + ([("layer %d gamma" % li, lp.gamma)] if lp.bn else [])
        if pool_ns:
            reread.append(("layer %d biases" % (len(layers) - 1), layers[-1].biases))          # (gspn_mlp_bwd_data_pooltop rebuilds y from them)
        if gather is not None:
            reread += [("gather[%r]" % k, gather.get(k)) for k in ("gidx", "rel", "idx", "order", "offsets")]
        if pre is not None:
            reread += [("preagg[%r]" % k, pre.get(k)) for k in ("idx", "w", "side")]
            reread += [("preagg['scatter_reads'][%d]" % k, t) for k, t in enumerate(pre.get("scatter_reads", ()))]
        ctx.versions = [(name, t, t._version) for name, t in reread if t is not None]
        ctx.arg = arg
        ctx.pool_yarg = pool[0] if pool is not None else None
        if pool_ns:
            ctx.save_for_backward(out)           # the pooled output: where it is 0 no gradient passes the ReLU (POOLTOP_STREAM)
        ctx.spec = spec
        ctx.sw = sw
        ctx.rows = rows
        ctx.x_needs_grad = x.requires_grad
        return out

    @staticmethod
    def backward(ctx, d_out):
        spec = ctx.spec
        layers = spec["layers"]
        for name, t, version in ctx.versions:
            if t._version != version:
                raise RuntimeError("mlp_stack: %s, which backward reads again, was modified in place between forward and backward "
                                   "(it is at version %d, the forward pass saw version %d)" % (name, t._version, version))
        d_out = d_out.contiguous()
        dev = d_out.device
        is_training = bool(spec["is_training"])
        # what the steps of this backward pass share.  coef: layer index -> (cA, cB, cC, dgamma, dbeta, dbias) taken BEFORE that layer's pass A;
        # sunk: data pointers of gradient buffers that ARE bucket slices (returned to autograd as None)
        b = types.SimpleNamespace(lib=L.lib(), ctx=ctx, spec=spec, layers=layers, rows=ctx.rows, sw=ctx.sw, dev=dev, d_out=d_out, pool_ns=spec["pool_ns"],
                                  is_training=is_training, tr_all=is_training and EARLY_R and not DEFER_DW, coef={}, sunk=set(), side=None, main=None, keep=[])
        grads = []
        dz, ldz = (None if b.pool_ns else d_out), d_out.shape[1]        # dz: dense upstream gradient of the current layer
        with torch.cuda.device(dev):
            b.st = L.stream()
            for li in range(len(layers) - 1, -1, -1):
                lp, s = layers[li], ctx.saved[li]
                cin, cout = s.cin, lp.weights.shape[1]
                a = L.DyArgs()
                a.Y, a.ldy = s.y.data_ptr(), cout
                if dz is None:
                    a.dZ, a.ldz, a.dPool, a.pool_arg, a.ns = None, 0, d_out.data_ptr(), ctx.arg.data_ptr(), b.pool_ns
                else:
                    a.dZ, a.ldz, a.dPool, a.pool_arg, a.ns = dz.data_ptr(), ldz, None, None, 0
                a.scale, a.shift = s.scale.data_ptr(), s.shift.data_ptr()
                gather0 = ctx.gather if li == 0 else None
                if li == len(layers) - 1:
                    _early_top_coef(b, li, dz, ldz)
                known = b.coef.get(li)
                if b.sw > 1 and lp.bn and known is None:
                    raise RuntimeError("mlp_stack (fused SyncBN): layer %d has no early BN coefficients -- its reductions would be per replica" % li)
                cf = known
                if known is None:
                    cf = [torch.empty(cout, dtype=torch.float32, device=dev) for _ in range(3)]
                    cf += [_grad_buffer(lp.gamma, b.sunk) if lp.bn else None, _grad_buffer(lp.beta, b.sunk) if lp.bn else None, _grad_buffer(lp.biases, b.sunk)]
                cA, cB, cC, dgamma, dbeta, dbias = cf
                a.cA, a.cB, a.cC = cA.data_ptr(), cB.data_ptr(), cC.data_ptr()
                if li == 0 and ctx.pre is not None:
                    if known is None:
                        raise RuntimeError("mlp_stack(preagg=): the first layer's BN coefficients must be known before its backward (EARLY_R)")
                    ev = _tic()
                    dW, dx = _preagg_backward(b.lib, ctx.pre, ctx.pre_x, lp, a, b.rows, cout, ctx.x_needs_grad, dev, b.st, b.sunk)
                    # (the whole backward of the layer, both "passes": dW_feat and d(feat) on the source rows, dW_side on the output rows)
                    _toc(ev, "bwd", b.rows, cin, cout, 2.0 * cout * (ctx.pre_x.shape[0] * ctx.pre["c"] * (2 if ctx.x_needs_grad else 1) + b.rows * ctx.pre["side_n"]))
                    grads = [dW, dbias] + ([dbeta, dgamma] if lp.bn else []) + grads
                    del a
                    continue
                dW = _grad_buffer(lp.weights, b.sunk)
                grads = [dW, dbias] + ([dbeta, dgamma] if lp.bn else []) + grads
                wcin = int(b.lib.gspn_mlp_gather_cin(ctypes.byref(ctx.gargs))) if gather0 is not None else cin
                work = torch.empty(int(b.lib.gspn_mlp_bwd_work_bytes(b.rows, wcin, cout)) // 4, dtype=torch.float32, device=dev)
                has_dx = li > 0 or ctx.x_needs_grad
                dx = _fused_attempt(b, li, a, known, dz, work, dW)
                if dx is None:
                    fuse_dw = FUSE_DW and has_dx and not DEFER_DW and gather0 is None     # the dW reduction rides in spare workgroups of this layer's pass B
                    later = fuse_dw or (DEFER_DW and gather0 is None)      # the sum over pass A's partial tiles is left to pass B / the side stream
                    ran_known = _pass_a(b, li, a, known, cf, work, None if later else dW)
                    if DEFER_DW and gather0 is None:
                        _deferred_dw(b, li, a, work, dW)
                    # known coefficients: the partial tiles are dW's own (plain sum)
                    ride = _dw_args(s, lp, 0 if ran_known else int(lp.bn), is_training, work, dW) if fuse_dw else None
                    if has_dx:
                        dx = _pass_b_gathered(b, a, gather0) if gather0 is not None else _pass_b(b, li, a, known, dz, ride)
                if li > 0:
                    dz, ldz = dx, dx.shape[1]
                # keep the buffers referenced by `a` alive until the kernels are enqueued (same stream: ordered)
                del a
            if b.side is not None:
                b.main.wait_event(b.side.record_event())            # join: the gradients (and the workspaces) are complete past here
        del b.keep
        # dx: layer 0's.  Gradients that were written straight into their bucket slices are not handed to autograd (it would re-assign / clone them)
        return (dx, None, None) + tuple(None if (g is not None and g.data_ptr() in b.sunk) else g for g in grads)


def _ref(struct):
    return None if struct is None else ctypes.byref(struct)


def _dw_args(s, lp, use_bn, is_training, work, dW):
    """gspn_dw_args of a layer from its saved record: the dW reduction its pass A, run with dW = NULL, left in `work`"""
    return L.DwArgs(L.ptr(s.x), s.ldx, L.ptr(s.var), L.ptr(lp.gamma if lp.bn else None), BN_EPS, use_bn, int(is_training), L.ptr(work), L.ptr(dW))


def _rsum_args(b, p, c):
    """(gspn_rsum_args, part, npart) from the saved record p of the PREVIOUS layer (c channels): its BN reductions out of this layer's pass B"""
    part = torch.empty(int(b.lib.gspn_rsum_part_floats(b.rows, c)), dtype=torch.float32, device=b.dev)
    npart = ctypes.c_int(0)
    return L.RsumArgs(L.ptr(p.y), c, L.ptr(p.scale), L.ptr(p.shift), L.ptr(p.mean), L.ptr(p.var), BN_EPS, L.ptr(part), ctypes.pointer(npart)), part, npart


def _early_top_coef(b, li, dz, ldz):
    """early coefficients of the stack's top layer, from its upstream gradient, into b.coef[li]"""
    lib, rows, ctx, lp, s = b.lib, b.rows, b.ctx, b.layers[li], b.ctx.saved[li]
    cout = lp.weights.shape[1]
    # a DENSE stack takes them in one streaming pass over (d_out, Y): worth its launch on the long layers only (the two-product pass A of a
    # short layer costs less than the extra dependent kernels)
    dense = dz is not None and (DENSE_TOP_RSUM or b.sw > 1) and (
        (li > 0 and rows >= DENSE_TOP_MIN_ROWS) or (b.sw > 1 and not (li == 0 and (ctx.gather is not None or ctx.pre is not None))))
    if not (b.tr_all and lp.bn and li not in b.coef and (dz is None or dense)):
        return
    part = torch.empty(int(lib.gspn_rsum_part_floats(rows, cout)), dtype=torch.float32, device=b.dev)
    npart = ctypes.c_int(0)
    if dz is None:
        # ---- a pooled stack: (groups x c) work on (dPool, arg, Y) ----
        yarg = ctx.pool_yarg           # y at the arg row, left by gspn_pool32_select (None: gather it from Y)
        L.check(lib.gspn_pool_rsum(rows // b.pool_ns, b.pool_ns, cout, L.ptr(b.d_out), L.ptr(ctx.arg), L.ptr(s.y if yarg is None else yarg),
                                   cout if yarg is None else 0, L.ptr(s.scale), L.ptr(s.shift),
                                   L.ptr(s.mean), L.ptr(s.var), BN_EPS, L.ptr(part), ctypes.byref(npart), b.st), "pool_rsum")
        b.coef[li] = _coef_from_parts(lib, rows, cout, npart.value, part, s.mean, s.var, lp, b.dev, b.st, b.sw, b.sunk)
    else:
        try:
            L.check(lib.gspn_dense_rsum(rows, cout, L.ptr(dz), ldz, L.ptr(s.y), cout, L.ptr(s.scale), L.ptr(s.shift), L.ptr(s.mean), L.ptr(s.var),
                                        BN_EPS, L.ptr(part), ctypes.byref(npart), b.st), "dense_rsum")
            b.coef[li] = _coef_from_parts(lib, rows, cout, npart.value, part, s.mean, s.var, lp, b.dev, b.st, b.sw, b.sunk)
        except NotImplementedError:
            pass


def _fused_attempt(b, li, a, known, dz, work, dW):
    """both passes of layer li in one launch (known coefficients, an inner layer of a shape the fused kernel takes): its dX, or None when
    the launch is not tried or the library declines it"""
    lib, rows, layers, lp, s = b.lib, b.rows, b.layers, b.layers[li], b.ctx.saved[li]
    cin, cout = s.cin, lp.weights.shape[1]
    if not (FUSED_BWD and known is not None and (dz is not None or (b.pool_ns == 32 and POOLTOP_FUSED)) and li > 0 and not DEFER_DW
            and int(lib.gspn_mlp_bwd_fused_work_bytes(rows, cin, cout)) > 0):
        return None
    prev, p = layers[li - 1], b.ctx.saved[li - 1]
    want_rsum = b.tr_all and prev.bn
    dx = torch.empty((rows, cin), dtype=torch.float32, device=b.dev)
    part = torch.empty(int(lib.gspn_rsum_part_floats(rows, cin)), dtype=torch.float32, device=b.dev) if want_rsum else None
    npart = ctypes.c_int(0)
    ev = _tic()
    merged = pg = None
    try:
        if want_rsum and b.sw == 1 and FUSED_COEF:
            # the previous layer's coefficient kernel and this layer's dW reduction depend on the fused launch only: one launch
            pc = [torch.empty(cin, dtype=torch.float32, device=b.dev) for _ in range(3)]
            pg = [_grad_buffer(prev.gamma, b.sunk), _grad_buffer(prev.beta, b.sunk), _grad_buffer(prev.biases, b.sunk)]
            L.check(lib.gspn_mlp_bwd_fused_coef(rows, cin, cout, ctypes.byref(a), L.ptr(lp.weights), L.ptr(s.x), s.ldx, L.ptr(s.in_scale),
                                                L.ptr(s.in_shift), L.ptr(dx), cin, L.ptr(work), L.ptr(dW), L.ptr(p.mean), L.ptr(p.var), BN_EPS,
                                                L.ptr(part), ctypes.byref(npart), L.ptr(prev.gamma), L.ptr(pc[0]), L.ptr(pc[1]), L.ptr(pc[2]),
                                                L.ptr(pg[0]), L.ptr(pg[1]), L.ptr(pg[2]), b.st), "mlp_bwd_fused_coef")
            merged = (pc[0], pc[1], pc[2], pg[0], pg[1], pg[2])
        else:
            L.check(lib.gspn_mlp_bwd_fused(rows, cin, cout, ctypes.byref(a), L.ptr(lp.weights), L.ptr(s.x), s.ldx, L.ptr(s.in_scale), L.ptr(s.in_shift),
                                           L.ptr(dx), cin, L.ptr(work), L.ptr(dW), L.ptr(p.mean), L.ptr(p.var), BN_EPS, L.ptr(part),
                                           ctypes.byref(npart), b.st), "mlp_bwd_fused")
    except NotImplementedError:
        if pg is not None:           # the declined launch filled none of the previous layer's sinks: hand them back
            for prm, buf in zip((prev.gamma, prev.beta, prev.biases), pg):
                _grad_release(prm, buf, b.sunk)
        return None
    _toc(ev, "fused", rows, cin, cout, 4.0 * rows * cin * cout)
    if merged is not None:
        b.coef[li - 1] = merged
    elif want_rsum:
        b.coef[li - 1] = _coef_from_parts(lib, rows, cin, npart.value, part, p.mean, p.var, prev, b.dev, b.st, b.sw, b.sunk)
    return dx


def _pass_a(b, li, a, known, cf, work, dW):
    """pass A of layer li: one GEMM where the coefficients are known and the kernels take the shape (returns True), else the two-product form,
    which writes cf = (cA, cB, cC, dgamma, dbeta, dbias) itself.  dW None: the sum over the partial tiles in `work` is left to a later launch"""
    lib, rows, ctx, lp, s = b.lib, b.rows, b.ctx, b.layers[li], b.ctx.saved[li]
    cin, cout = s.cin, lp.weights.shape[1]
    gargs = ctypes.byref(ctx.gargs) if (li == 0 and ctx.gather is not None) else None
    ev = _tic()
    ran_known = False
    if known is not None:
        try:
            L.check(lib.gspn_mlp_bwd_wgrad_known(rows, cin, cout, ctypes.byref(a), L.ptr(s.x), s.ldx, L.ptr(s.in_scale), L.ptr(s.in_shift), gargs, L.ptr(work),
                                                 L.ptr(dW), b.st), "mlp_bwd_wgrad_known")
            ran_known = True
        except NotImplementedError:
            pass                             # a shape the one-GEMM kernels do not take: the two-product pass recomputes the same coefficients
    if not ran_known:
        tail = (L.ptr(s.mean), L.ptr(s.var), L.ptr(lp.gamma if lp.bn else None), BN_EPS, int(lp.bn), int(b.is_training), L.ptr(work),
                L.ptr(cf[0]), L.ptr(cf[1]), L.ptr(cf[2]), L.ptr(cf[3]), L.ptr(cf[4]), L.ptr(cf[5]))
        if gargs is not None:
            L.check(lib.gspn_mlp_bwd_wgrad_gather(rows, gargs, cout, ctypes.byref(a), *tail, L.ptr(dW), b.st), "mlp_bwd_wgrad_gather")
        else:
            L.check(lib.gspn_mlp_bwd_wgrad(rows, cin, cout, ctypes.byref(a), L.ptr(s.x), s.ldx, L.ptr(s.in_scale), L.ptr(s.in_shift), *tail,
                                           L.ptr(dW), b.st), "mlp_bwd_wgrad")
    _toc(ev, "wgrad", rows, cin, cout, None if ran_known else 2 * 2.0 * rows * cin * cout)      # the two-product form: G1 and Gx
    return ran_known


def _deferred_dw(b, li, a, work, dW):
    """DEFER_DW: the dW reduction of layer li on the side stream, ordered after its pass A"""
    lp, s = b.layers[li], b.ctx.saved[li]
    if b.side is None:
        b.side = _side_stream(b.dev)
        b.main = torch.cuda.current_stream()
    b.side.wait_event(b.main.record_event())            # after this layer's wgrad + channel sums
    dw = _dw_args(s, lp, int(lp.bn), b.is_training, work, dW)
    L.check(b.lib.gspn_mlp_bwd_dw(b.rows, s.cin, lp.weights.shape[1], ctypes.byref(a), ctypes.byref(dw), ctypes.c_void_p(b.side.cuda_stream)), "mlp_bwd_dw")
    b.keep.append((work, a))                            # alive until the side stream has joined


def _pass_b_gathered(b, a, gather0):
    """pass B of a gathered first layer: dX of the feature columns in grouped-row layout, then the gather-form gradient of the grouping
    (inverse lists; atomics without them) straight into d(features)"""
    lib, rows, lp, s = b.lib, b.rows, b.layers[0], b.ctx.saved[0]
    cout = lp.weights.shape[1]
    gb, gn, gm, gns = gather0["dims"]
    gc, xf = gather0["c"], int(gather0["xyz_first"])
    ldp = (3 + gc + 3) // 4 * 4
    dxg = torch.empty((rows, ldp), dtype=torch.float32, device=b.dev)
    ev = _tic()
    L.check(lib.gspn_mlp_bwd_data(rows, s.cin, cout, ctypes.byref(a), L.ptr(lp.weights), 3 if xf else 0, gc, L.ptr(dxg), ldp, None, None, b.st), "mlp_bwd_data")
    _toc(ev, "bwd", rows, s.cin, cout, 2.0 * rows * gc * cout)
    gp = torch.empty((gb, gn, gc), dtype=torch.float32, device=b.dev)
    if gather0.get("order") is not None:
        L.check(lib.gspn_sa_group_concat_grad_csr(gb, gn, gc, gm, gns, L.ptr(gather0["order"]), L.ptr(gather0["offsets"]), xf, ldp,
                                                  L.ptr(dxg), L.ptr(gp), b.st), "sa_group_concat_grad_csr")
    else:
        L.check(lib.gspn_sa_group_concat_grad(gb, gn, gc, gm, gns, L.ptr(gather0["idx"]), xf, ldp, L.ptr(dxg), L.ptr(gp), b.st), "sa_group_concat_grad")
    ldf = b.ctx.gargs.ldf
    dx0 = gp.view(gb * gn, gc)
    return dx0 if ldf == gc else torch.nn.functional.pad(dx0, (0, ldf - gc))


def _pass_b(b, li, a, known, dz, ride):
    """pass B of layer li -> dX.  ride: the gspn_dw_args of the layer's dW reduction when it rides in this launch, else None.  This dX is
    the dz of layer li-1: its epilogue can take that layer's BN reductions (early coefficients for its pass A)"""
    lib, rows, layers, lp, s = b.lib, b.rows, b.layers, b.layers[li], b.ctx.saved[li]
    cin, cout = s.cin, lp.weights.shape[1]
    dx = torch.empty((rows, s.ldx if li == 0 else cin), dtype=torch.float32, device=b.dev)
    if li == 0 and s.ldx > cin and b.spec.get("grad_cols") is None:
        dx.zero_()
    # only grad_cols of the input feed a gradient upstream (e.g. not the xyz columns of an SA input)
    gc = (b.spec.get("grad_cols") if li == 0 else None) or (0, cin)
    prev = layers[li - 1] if li > 0 else None
    want_rsum = b.tr_all and prev is not None and prev.bn
    ev = _tic()
    p = b.ctx.saved[li - 1] if want_rsum else None
    rs, part, npart = _rsum_args(b, p, cin) if want_rsum else (None, None, None)
    top_done = False
    if (POOLTOP_STREAM and dz is None and b.pool_ns == 32 and want_rsum and ride is not None and known is not None and cin <= 64
            and cin % 4 == 0 and cout <= 128 and cout % 4 == 0 and tuple(gc) == (0, cin)):
        scr = torch.empty(int(lib.gspn_pooltop_scratch_floats(rows, cin, cout)), dtype=torch.float32, device=b.dev)
        try:
            L.check(lib.gspn_mlp_bwd_data_pooltop(rows, cin, cout, ctypes.byref(a), L.ptr(lp.weights), L.ptr(lp.biases), L.ptr(b.ctx.saved_tensors[0]),
                                                  L.ptr(scr), L.ptr(dx), dx.shape[1], ctypes.byref(ride), ctypes.byref(rs), b.st), "mlp_bwd_data_pooltop")
            top_done = True
        except NotImplementedError:
            pass
    if not top_done:
        L.check(lib.gspn_mlp_bwd_data(rows, cin, cout, ctypes.byref(a), L.ptr(lp.weights), int(gc[0]), int(gc[1]), L.ptr(dx), dx.shape[1],
                                      _ref(ride), _ref(rs), b.st), "mlp_bwd_data")
    if want_rsum:
        b.coef[li - 1] = _coef_from_parts(lib, rows, cin, npart.value, part, p.mean, p.var, prev, b.dev, b.st, b.sw, b.sunk)
    _toc(ev, "bwd", rows, cin, cout, 2.0 * rows * int(gc[1]) * cout)
    return dx


_consts = {}


def _const_vectors(dev, c):
    """(ones(c), zeros(c)) on dev, made once: read-only operands of the no-BN GEMM calls"""
    key = (dev.type, dev.index, c)
    v = _consts.get(key)
    if v is None:
        v = _consts[key] = (torch.ones(c, dtype=torch.float32, device=dev), torch.zeros(c, dtype=torch.float32, device=dev))
    return v


def _preagg_backward(lib, pre, x, lp, a, rows, cout, need_dx, dev, st, sunk=None):
    """backward of a pre-aggregated first layer: dY written once (+ dW_side), its transpose-gather G onto the source rows, then
    dW_feat = feat^T . G and d(feat) = G . W_feat^T as small GEMMs without BN (always-open mask: scale 0, shift 1, dY = dz)"""
    c, side_n = pre["c"], pre["side_n"]
    dW = _grad_buffer(lp.weights, sunk if sunk is not None else set())
    if pre["c"] + side_n < lp.weights.shape[0]:
        dW.zero_()
    dy = torch.empty((rows, cout), dtype=torch.float32, device=dev)
    part = torch.empty(int(lib.gspn_preagg_part_floats(cout, max(side_n, 1))), dtype=torch.float32, device=dev)
    dws = dW[pre["ws0"]:pre["ws0"] + side_n]
    ride = need_dx and FUSE_DW               # the reductions of dW_side's and dW_feat's partial tiles ride in the d(feat) launch ...
    dws_now = None if (ride and side_n) else dws         # ... and are then not run by the launches that leave the tiles
    nsl = ctypes.c_int(0)
    L.check(lib.gspn_preagg_bwd_dy(rows, cout, ctypes.byref(a), L.ptr(pre["side"]), pre["side_ld"], side_n, L.ptr(dy), L.ptr(part),
                                   L.ptr(dws_now), ctypes.byref(nsl), st), "preagg_bwd_dy")
    nsrc = x.shape[0]
    gsrc = pre["scatter"](dy, cout)                                 # (source rows, cout): sum over the output rows each source row fed
    one, zero = _const_vectors(dev, cout)
    a2 = L.DyArgs()
    a2.Y, a2.ldy = gsrc.data_ptr(), cout
    a2.dZ, a2.ldz, a2.dPool, a2.pool_arg, a2.ns = gsrc.data_ptr(), cout, None, None, 0
    a2.scale, a2.shift = zero.data_ptr(), one.data_ptr()           # always-open mask
    a2.cA, a2.cB, a2.cC = one.data_ptr(), zero.data_ptr(), zero.data_ptr()      # known coefficients: dY = dz
    dwf = dW[pre["wf0"]:pre["wf0"] + c]
    dwf_now = None if ride else dwf
    wf = lp.weights[pre["wf0"]:pre["wf0"] + c]
    work = torch.empty(int(lib.gspn_mlp_bwd_work_bytes(nsrc, c, cout)) // 4, dtype=torch.float32, device=dev)
    L.check(lib.gspn_mlp_bwd_wgrad_known(nsrc, c, cout, ctypes.byref(a2), L.ptr(x), x.shape[1], None, None, None, L.ptr(work),
                                         L.ptr(dwf_now), st), "mlp_bwd_wgrad_known(pre-aggregation)")
    dx = None
    if need_dx:
        dx = torch.empty((nsrc, x.shape[1]), dtype=torch.float32, device=dev)
        if x.shape[1] > c:
            dx.zero_()
        # riding: dW_feat's reduction, and dW_side's as the second job
        dw = L.DwArgs(L.ptr(x), x.shape[1], None, None, BN_EPS, 0, 0, L.ptr(work), L.ptr(dwf), L.ptr(part), side_n, nsl.value if side_n else 0,
                      L.ptr(dws)) if ride else None
        L.check(lib.gspn_mlp_bwd_data(nsrc, c, cout, ctypes.byref(a2), L.ptr(wf), 0, c, L.ptr(dx), x.shape[1], _ref(dw), None, st), "mlp_bwd_data(pre-aggregation)")
    return dW, dx


def _coef_from_parts(lib, rows, c, nparts, part, mean, var, lp, dev, st, sw=1, sunk=None):
    """gspn_mlp_bwd_coef: partial sums [nparts][2][c] of (dyh, dyh*xhat) -> the layer's final BN-backward coefficients and its
    dgamma / dbeta / dbias, before its pass A runs.  sw > 1 (fused SyncBN): the partial rows are all-reduced first, the coefficients are
    those of the global batch (rows x sw), and dgamma / dbeta / dbias -- global sums then -- are divided by sw so that the gradient
    bucket's SUM all-reduce restores them (an exact division for power-of-two worlds)."""
    cA = torch.empty(c, dtype=torch.float32, device=dev)
    cB = torch.empty(c, dtype=torch.float32, device=dev)
    cC = torch.empty(c, dtype=torch.float32, device=dev)
    if sunk is not None and sw == 1:
        dgamma, dbeta, dbias = _grad_buffer(lp.gamma, sunk), _grad_buffer(lp.beta, sunk), _grad_buffer(lp.biases, sunk)
        dgb = None
    else:
        dgb = torch.empty((3, c), dtype=torch.float32, device=dev)
        dgamma, dbeta, dbias = dgb[0], dgb[1], dgb[2]
    if sw > 1:
        _allreduce_sum(part[:int(nparts) * 2 * c])
    try:
        L.check(lib.gspn_mlp_bwd_coef(rows * sw, c, int(nparts), L.ptr(part), L.ptr(mean), L.ptr(var), L.ptr(lp.gamma), BN_EPS,
                                      L.ptr(cA), L.ptr(cB), L.ptr(cC), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dbias), st), "mlp_bwd_coef")
    except NotImplementedError:
        if dgb is None:                          # (the dense_rsum block catches this and runs the two-product pass A, which must find the sinks unclaimed; harmless where the caller lets it propagate)
            for prm, buf in zip((lp.gamma, lp.beta, lp.biases), (dgamma, dbeta, dbias)):
                _grad_release(prm, buf, sunk)
        raise
    if sw > 1:
        dgb.mul_(1.0 / sw)
    return cA, cB, cC, dgamma, dbeta, dbias


class _Linear(torch.autograd.Function):
    """y = x.W + b with no batch-norm and no activation (tf_util.conv1d(..., activation_fn=None), e.g. model_rpointnet.py:71-73,262-263)
    on the same kernels: the forward GEMM's raw output IS the result; backward runs the two passes with an always-open ReLU mask
    (scale 0, shift 1) and use_bn = 0, so dY = dz."""

    @staticmethod
    def forward(ctx, x, cin, w, b):
        lib = L.lib()
        rows, ld = x.shape
        cout = w.shape[1]
        y = torch.empty((rows, cout), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            L.check(lib.gspn_mlp_fwd(rows, cin, cout, L.ptr(x), ld, None, None, L.ptr(w), L.ptr(b), L.ptr(y), cout, None, L.stream()), "mlp_fwd")
        ctx.save_for_backward(x, w, y)
        ctx.cin = cin
        return y

    @staticmethod
    def backward(ctx, dz):
        lib = L.lib()
        x, w, y = ctx.saved_tensors
        cin = ctx.cin
        rows, ld = x.shape
        cout = w.shape[1]
        dz = dz.contiguous()
        dev = dz.device
        one = torch.ones(cout, dtype=torch.float32, device=dev)
        zero = torch.zeros(cout, dtype=torch.float32, device=dev)
        cA, cB, cC = torch.empty_like(one), torch.empty_like(one), torch.empty_like(one)
        a = L.DyArgs()
        a.Y, a.ldy = y.data_ptr(), cout
        a.dZ, a.ldz, a.dPool, a.pool_arg, a.ns = dz.data_ptr(), cout, None, None, 0
        a.scale, a.shift = zero.data_ptr(), one.data_ptr()          # 0*y + 1 > 0: every element passes
        a.cA, a.cB, a.cC = cA.data_ptr(), cB.data_ptr(), cC.data_ptr()
        dW = torch.empty_like(w)
        dbias = torch.empty(cout, dtype=torch.float32, device=dev)
        dx = None
        with torch.cuda.device(dev):
            work = torch.empty(int(lib.gspn_mlp_bwd_work_bytes(rows, cin, cout)) // 4, dtype=torch.float32, device=dev)
            L.check(lib.gspn_mlp_bwd_wgrad(rows, cin, cout, ctypes.byref(a), L.ptr(x), ld, None, None, None, None, None, BN_EPS, 0, 0,
                                           L.ptr(work), L.ptr(cA), L.ptr(cB), L.ptr(cC), None, None, L.ptr(dbias), L.ptr(dW), L.stream()), "mlp_bwd_wgrad")
            if ctx.needs_input_grad[0]:
                dx = torch.empty((rows, ld), dtype=torch.float32, device=dev)
                if ld > cin:
                    dx.zero_()
                L.check(lib.gspn_mlp_bwd_data(rows, cin, cout, ctypes.byref(a), L.ptr(w), 0, cin, L.ptr(dx), ld, None, None, L.stream()), "mlp_bwd_data")
        return dx, None, dW, dbias


def mlp_linear(x, cin, lp):
    """x (rows, ld >= cin) -> x[:, :cin].W + b for a LayerParams without batch-norm."""
    if lp.bn:
        raise ValueError("mlp_linear is the no-BN, no-activation layer")
    x, (lp,) = checked_layers(x, 2, [lp], cin, "mlp_linear")
    return _Linear.apply(x, cin, lp.weights, lp.biases)


def _mlp_stack_sync_bn(x, cin, layers, decay, pool_ns):
    """the SYNC_BN form of mlp_stack: per layer y = x.W + b on the MFMA kernel, then BN over the global batch + ReLU"""
    from .parallel import sync_bn_relu
    cur = x
    for lp in layers:
        y = _Linear.apply(cur, cin, lp.weights, lp.biases)
        cur = sync_bn_relu(y, lp.gamma, lp.beta, lp.moving_mean, lp.moving_variance, decay, BN_EPS) if lp.bn else torch.relu(y)
        cin = y.shape[1]
    if pool_ns:
        cur = cur.view(-1, pool_ns, cur.shape[1]).max(dim=1).values
    return cur


def _aligned16(t):
    # (a non-contiguous tensor never reaches a kernel: L.need copies the input x, layer_on_device a layer tensor, each to a fresh -- aligned --
    #  allocation, before use)
    return t is None or not t.is_contiguous() or t.data_ptr() % 16 == 0


def preagg_ok(layers, is_training, c, x=None):
    """can the stack's first layer be pre-aggregated?  (training-mode BN on the first two layers -- the second layer's pass B hands the
    first its BN coefficients --, a kernel-friendly width, enough feature columns for the saved GEMM work to matter, and operands the
    pre-aggregation kernels take: they read the first layer's weights and biases, and the source rows `x` in backward, 16 bytes at a time,
    and their launchers REJECT (not decline) a 4-byte-aligned one -- e.g. a parameter that lives in a flat optimiser buffer behind a
    tensor of odd length.  Such a stack takes the materialised input rows and the general kernels.)"""
    return (PREAGG and EARLY_R and not DEFER_DW and not (SYNC_BN and not SYNC_BN_FUSED) and is_training and len(layers) >= 2 and layers[0].bn and layers[1].bn
            and c >= PREAGG_MIN_C and bool(L.lib().gspn_preagg_ok(layers[0].weights.shape[1]))
            and _aligned16(layers[0].weights) and _aligned16(layers[0].biases) and _aligned16(x))


def mlp_stack(x, cin, layers, is_training, bn_decay, pool_ns=None, grad_cols=None, gather=None, preagg=None):
    """x: (rows, ld>=cin) float32 on a ROCm device.  Returns (rows/pool_ns, C_last) if pool_ns else (rows, C_last).
    grad_cols = (col0, ncols): the only columns of x whose gradient the caller will read (the rest of x.grad is left undefined).
    gather (fused SA front end): x is then the (b*n, ldf) FEATURE matrix and the stack's input rows are virtual --
    dict(rows, c, xyz_first, gidx, rel, dims=(b, n, m, ns), idx, order, offsets), see pointnet_util.pointnet_sa_module; cin = 3 + c.
    preagg (pre-aggregated first layer): x is the (source rows, ldf) feature matrix; dict(rows, c, T, idx, w, per_scene_rows,
    per_scene_src, side, side_ld, side_n, wf0, ws0 [first rows of W_feat / W_side inside the layer's weights], scatter [callable:
    (dY (rows, cout), cout) -> (source rows, cout), the transpose of the aggregation], scatter_reads [optional: the tensors that callable
    reads, so that an in-place change of one between forward and backward is refused like one of x]) -- see pointnet_util.
    Every layer tensor is validated (checked_layers); a non-contiguous weight / bias / beta / gamma is copied, a non-contiguous moving
    statistic is refused.  Backward raises RuntimeError when a tensor it reads again was modified in place since the forward pass.
    Raises NotImplementedError (before anything has run) when the first layer's shape is outside what the gathering kernels take."""
    if not layers:
        raise ValueError("mlp_stack needs at least one layer")
    x, layers = checked_layers(x, 2, layers, cin, "mlp_stack")
    if gather is not None:
        if x.shape[1] % 4 or x.data_ptr() % 16 or gather["c"] > x.shape[1] or cin != 3 + gather["c"] or len(layers) < 2 or layers[0].weights.shape[1] % 4:
            raise NotImplementedError("mlp_stack(gather=): needs 16-byte aligned feature rows, >= 2 layers and a first layer of 4k output channels")
        if SYNC_BN and not SYNC_BN_FUSED:
            raise NotImplementedError("mlp_stack(gather=) with the layer-by-layer SyncBN form")
    if preagg is not None:
        if gather is not None or not preagg_ok(layers, is_training, preagg["c"], x) or cin != preagg["c"] + preagg["side_n"]:
            raise NotImplementedError("mlp_stack(preagg=): training-mode BN stacks of >= 2 layers, cin = c + side_n, no gather")
    if pool_ns and (preagg["rows"] if preagg is not None else (gather["rows"] if gather is not None else x.shape[0])) % pool_ns:
        raise ValueError("rows must be a multiple of pool_ns")
    if grad_cols is not None and not (0 <= grad_cols[0] and grad_cols[1] > 0 and grad_cols[0] + grad_cols[1] <= cin):
        raise ValueError("grad_cols must be a column range inside [0, cin)")
    sync_fused = False
    if SYNC_BN and is_training and any(lp.bn for lp in layers):
        import torch.distributed as dist
        if dist.is_initialized() and dist.get_world_size() > 1:
            # the fused kernels when every layer is batch-normalised and the early coefficients are on (see SYNC_BN_FUSED); else layer by layer
            sync_fused = SYNC_BN_FUSED and EARLY_R and not DEFER_DW and all(lp.bn for lp in layers)
            if not sync_fused:
                if gather is not None or preagg is not None:
                    raise NotImplementedError("mlp_stack(gather= / preagg=) with the layer-by-layer SyncBN form")
                return _mlp_stack_sync_bn(x, cin, layers, 0.9 if bn_decay is None else float(bn_decay), pool_ns)
    spec = {"layers": layers, "is_training": is_training, "decay": 0.9 if bn_decay is None else float(bn_decay), "pool_ns": pool_ns,
            "grad_cols": grad_cols, "gather": gather, "preagg": preagg, "sync_bn": sync_fused}
    flat = []
    for lp in layers:
        flat += lp.tensors()
    return _MlpStack.apply(x, cin, spec, *flat)
