"""Every autograd node of gspn_amd/ (the rows of tests/autograd_cases.py) driven the ways autograd can drive it -- strided inputs, strided,
expanded and missing upstream gradients, one gradient tensor handed to two nodes, a retained graph, partial requires_grad, in-place changes
between the two passes, layer tensors that are views -- and the gradient-sink protocol of parallel.FlatGradBucket / mlp.GRAD_SINKS against the
run without sinks.

"Same" means bitwise (torch.equal): the library's backward passes add in a fixed order, and where one still adds with atomics the row feeds it
integer gradients, so that every order of the sum is exact.  Beside that, every run is held to the row's float64 restatement at the
tolerance of the node's own value test (the row names it)."""
import pytest
import torch

from tests import autograd_cases as AC

pytestmark = pytest.mark.gpu

CASES = AC.CASES
KINDS = ("permuted", "slice")


# ---- tensors ---------------------------------------------------------------------------------------------------------------------------

_MASTERS = {}


def masters(case):
    """the row's inputs, floats rounded to float32 (as float64) so that both sides start from the same numbers"""
    if case.name not in _MASTERS:
        _MASTERS[case.name] = {k: (v.float().double() if v.dtype.is_floating_point else v.clone()) for k, v in case.build().items()}
    return _MASTERS[case.name]


def as_view(t, kind):
    """the same values behind other strides.  permuted: a permuted-back view (for a matrix: the .t() of transposed storage).  slice: a
    column (1-D: every second element) slice of a larger poisoned buffer, 4 bytes past its 16-byte aligned start, pitch > width.
    expanded: the first element / row broadcast with stride 0 (other VALUES than t: the caller compares with its contiguous clone)."""
    if kind == "expanded":
        v = t[:1].expand(t.shape)
        assert 0 in v.stride() or t.shape[0] == 1
        return v
    poison = 777.0 if t.dtype.is_floating_point else 0          # (finite: a read of the wrong element shows as a difference, not as a NaN that spreads)
    if t.dim() == 1:
        buf = torch.full((2 * t.numel() + 1,), poison, dtype=t.dtype, device=t.device)
        v = buf[1::2] if kind == "slice" else buf[0::2][:t.numel()]
    elif kind == "permuted":
        buf = torch.full(tuple(reversed(t.shape)), poison, dtype=t.dtype, device=t.device)
        v = buf.permute(*reversed(range(t.dim())))
    else:
        buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 3,), poison, dtype=t.dtype, device=t.device)
        v = buf[..., 1:1 + t.shape[-1]]
    v.copy_(t)
    assert v.shape == t.shape and (not v.is_contiguous() or t.numel() == max(t.shape))
    if kind == "slice":
        assert v.data_ptr() % 16 != 0 and v.storage_offset() == 1
    return v


def on_device(case, values, views=None, requires="all"):
    """the row's tensors on the GPU.  views: {name: kind}; requires: 'all', or the names that are to require a gradient"""
    t = {}
    for k, v in values.items():
        d = (v.float() if v.dtype.is_floating_point else v).cuda()
        if views and k in views:
            d = as_view(d, views[k])
        if k in case.grads + case.params and (requires == "all" or k in requires):
            d.requires_grad_(True)
        t[k] = d
    return t


def upstream(case, outs, seed=5):
    """one upstream gradient per output, float64 on the CPU (rounded to float32): integers in [-8, 8] for a node that adds with atomics"""
    g = torch.Generator().manual_seed(seed)
    if case.int_grads:
        return [torch.randint(-8, 9, tuple(o.shape), generator=g).double() for o in outs]
    return [torch.randn(tuple(o.shape), generator=g).double().float().double() for o in outs]


def grads_of(case, t):
    return {k: (None if t[k].grad is None else t[k].grad.detach().clone()) for k in case.grads + case.params}


def run(case, t, gos=None, hold=None, outputs=None):
    """forward and (gos: list of device tensors, one per output, or per entry of `outputs`) backward -> (outs detached, {name: grad})"""
    outs = case.call(t, hold)
    if gos is not None:
        chosen = outs if outputs is None else [outs[i] for i in outputs]
        torch.autograd.backward(list(chosen), list(gos))
    return [o.detach() for o in outs], grads_of(case, t)


def reference(case, values, gos64, outputs=None):
    t = {k: (v.clone().requires_grad_(True) if k in case.grads + case.params else v.clone()) for k, v in values.items()}
    outs = case.ref(t)
    chosen = outs if outputs is None else [outs[i] for i in outputs]
    torch.autograd.backward(list(chosen), [g.to(o.dtype) for g, o in zip(gos64, chosen)])
    return [o.detach() for o in outs], {k: t[k].grad for k in case.grads + case.params}


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------

def within(got, ref, tol, floor=0.0):
    """-> (ok, figure) of got against the float64 ref under a row's tolerance (tests/autograd_cases.py)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if tol[0] == "exact":
        return torch.equal(got, ref), float((got - ref).abs().max())
    d = (got - ref).abs()
    if tol[0] == "rel":
        err = float(d.max() / (max(float(ref.abs().max()), floor) + 1e-30))
        return err < tol[1], err
    bound = tol[1] + tol[1] * ref.abs()
    return bool((d <= bound).all()), float((d / bound).max())


def assert_close(case, outs, grads, ref_outs, ref_grads, what, floors=None):
    """floors: {name: magnitude} for a run whose true gradients may be zero up to rounding; the error is then taken relative to at
    least that magnitude"""
    assert len(outs) == len(ref_outs)
    for i, (o, r) in enumerate(zip(outs, ref_outs)):
        ok, fig = within(o, r, case.tol_out)
        assert ok, "%s %s: output %d off its float64 value: %.3g (tolerance %s of %s)" % (case.name, what, i, fig, case.tol_out, case.tol_from)
    for k, g in grads.items():
        if ref_grads.get(k) is None:
            continue
        assert g is not None, "%s %s: no gradient for %s" % (case.name, what, k)
        floor = float(ref_grads[case.zero_scale[k]].abs().max()) if k in case.zero_scale else 0.0
        floor = max(floor, (floors or {}).get(k, 0.0))
        ok, fig = within(g, ref_grads[k], case.tol_grad, floor)
        assert ok, "%s %s: gradient of %s off its float64 value: %.3g (tolerance %s of %s)" % (case.name, what, k, fig, case.tol_grad, case.tol_from)


def assert_same(case, outs, grads, base_outs, base_grads, what, names=None):
    for i, (o, r) in enumerate(zip(outs, base_outs)):
        assert torch.equal(o, r), "%s %s: output %d differs from the contiguous run by %.3g" % (case.name, what, i, float((o - r).abs().max()))
    for k in (names if names is not None else base_grads):
        g, r = grads[k], base_grads[k]
        assert (g is None) == (r is None), "%s %s: gradient of %s %s" % (case.name, what, k, "missing" if g is None else "unexpected")
        if g is not None:
            assert g.shape == r.shape, "%s %s: gradient of %s has shape %s, the tensor %s" % (case.name, what, k, tuple(g.shape), tuple(r.shape))
            assert torch.equal(g, r), "%s %s: gradient of %s differs from the contiguous run by %.3g" % (case.name, what, k, float((g - r).abs().max()))


_BASE = {}


def baseline(case):
    """the contiguous, everything-requires-grad, one-backward run of the row -- the only way the rest of the suite drives a node -- held
    to float64 once; -> dict(outs, grads, gos (device), gos64, ref_outs, ref_grads)"""
    if case.name not in _BASE:
        m = masters(case)
        if case.decisions is not None:
            from tests.test_gpu_mlp import fragile_entries
            fragile, rows = fragile_entries(*case.decisions(m))
            assert not bool(fragile.any()) and not bool(rows.any()), "%s: a ReLU / pool decision within float32 rounding: pick another seed" % case.name
        probe = case.ref({k: v.clone() for k, v in m.items()})
        gos64 = upstream(case, probe)
        ref_outs, ref_grads = reference(case, m, gos64)
        gos = [g.float().cuda() for g in gos64]
        hold = {}
        outs, grads = run(case, on_device(case, m), gos, hold)
        if case.name in ("mlp_stack_gathered", "mlp_stack_preagg"):
            assert hold["form"] == case.name.split("_")[-1], "%s: the module took the %s form" % (case.name, hold["form"])
        assert_close(case, outs, grads, ref_outs, ref_grads, "contiguous")
        _BASE[case.name] = dict(outs=outs, grads=grads, gos=gos, gos64=gos64, ref_outs=ref_outs, ref_grads=ref_grads)
    return _BASE[case.name]


# ---- 1. views in -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=repr)
def test_views_in(case):
    """every float and index input in turn behind non-standard strides, behind a misaligned slice of a wider buffer and (where a broadcast
    has a meaning) behind stride 0: outputs and gradients as for the contiguous clone, bit for bit"""
    base = baseline(case)
    m = masters(case)
    for name in case.grads + case.params + case.consts + case.ints:
        for kind in KINDS:
            t = on_device(case, m, {name: kind})
            if name in case.declines:                    # the call documents that it refuses such a layer tensor: it must, and before anything runs
                with pytest.raises(NotImplementedError):
                    case.call(t, None)
                continue
            outs, grads = run(case, t, base["gos"])
            assert_same(case, outs, grads, base["outs"], base["grads"], "%s as a %s view" % (name, kind))
    for name in case.expand:
        values = dict(m)
        values[name] = m[name][:1].expand(m[name].shape).clone()
        ref_outs, ref_grads = reference(case, values, base["gos64"])
        flat_outs, flat_grads = run(case, on_device(case, values), base["gos"])
        assert_close(case, flat_outs, flat_grads, ref_outs, ref_grads, "%s broadcast, contiguous" % name)
        outs, grads = run(case, on_device(case, m, {name: "expanded"}), base["gos"])
        assert_same(case, outs, grads, flat_outs, flat_grads, "%s as an expanded view" % name)


# ---- 2. gradients in -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gradients_in(case):
    """backward driven by an expanded scalar (out.sum()), a permuted gradient, a narrow slice with a storage offset (torch.cat downstream)
    and, for the nodes with several outputs, by one output alone: as with that gradient made contiguous (zero-filled), bit for bit"""
    base = baseline(case)
    m = masters(case)
    seen = []
    for kind in KINDS:
        t = on_device(case, m)
        outs = case.call(t, None)
        for o in outs:
            o.register_hook(lambda g: seen.append(g.is_contiguous()))
        torch.autograd.backward(list(outs), [as_view(g, kind) for g in base["gos"]])
        assert_same(case, [o.detach() for o in outs], grads_of(case, t), base["outs"], base["grads"], "gradient as a %s view" % kind)
    assert not all(seen), "every gradient reached the node contiguous: the scenario did not happen"
    # out.sum(): one scalar, expanded with stride 0
    ones64 = [torch.full(tuple(g.shape), 3.0, dtype=torch.float64) for g in base["gos64"]]
    ref_outs, ref_grads = reference(case, m, ones64)
    flat_outs, flat_grads = run(case, on_device(case, m), [g.float().cuda() for g in ones64])
    # (a constant gradient lies in the null space of a batch norm's backward: the true gradient of x, and of whatever feeds it, is zero up
    #  to rounding.  Its error is taken relative to the magnitude the unit-variance gradient of the contiguous run gives the same tensor --
    #  a third of what the terms that cancel here amount to.)
    floors = {k: float(v.abs().max()) for k, v in base["ref_grads"].items() if v is not None}
    assert_close(case, flat_outs, flat_grads, ref_outs, ref_grads, "constant gradient, contiguous", floors)
    t = on_device(case, m)
    outs = case.call(t, None)
    (3.0 * sum(o.sum() for o in outs)).backward()
    assert_same(case, [o.detach() for o in outs], grads_of(case, t), flat_outs, flat_grads, "gradient of 3 * out.sum()")
    # one output used, the others not: None where the contiguous run hands in zeros
    if len(base["outs"]) > 1:
        for i in range(len(base["outs"])):
            zero_filled = [g if j == i else torch.zeros_like(g) for j, g in enumerate(base["gos"])]
            ref_outs, ref_grads = reference(case, m, [base["gos64"][i]], outputs=[i])
            flat_outs, flat_grads = run(case, on_device(case, m), zero_filled)
            assert_close(case, flat_outs, {k: v for k, v in flat_grads.items() if ref_grads.get(k) is not None}, ref_outs, ref_grads,
                         "output %d alone, zero-filled" % i)
            outs, grads = run(case, on_device(case, m), [base["gos"][i]], outputs=[i])
            # (an input that only the unused outputs reach gets no gradient at all from autograd: zeros in the zero-filled run)
            for k, g in grads.items():
                if g is None:
                    assert float(flat_grads[k].abs().max()) == 0.0, (case.name, i, k)
                    grads[k] = torch.zeros_like(flat_grads[k])
            assert_same(case, outs, grads, flat_outs, flat_grads, "output %d alone" % i)


# ---- 3. one upstream gradient, two consumers -----------------------------------------------------------------------------------------

def _two_consumers(case_a, case_b):
    base_a, base_b = baseline(case_a), baseline(case_b)
    assert [o.shape for o in base_a["outs"]] == [o.shape for o in base_b["outs"]]
    ta, tb = on_device(case_a, masters(case_a)), on_device(case_b, masters(case_b))
    oa, ob = case_a.call(ta, None), case_b.call(tb, None)
    kept = []

    def keep(g):
        kept.append((g, g.clone()))
    for o in list(oa) + list(ob):
        o.register_hook(keep)
    sum(((x + y) * w).sum() for x, y, w in zip(oa, ob, base_a["gos"])).backward()
    assert len(kept) == 2 * len(oa)
    for g, copy in kept:
        assert torch.equal(g, copy), "%s + %s: a node wrote into the gradient it was handed" % (case_a.name, case_b.name)
    # the gradients of the two nodes run apart, each on the upstream gradient w
    for case, t, base in ((case_a, ta, base_a), (case_b, tb, base_b)):
        apart = base["grads"]
        if base is not base_a or case_a is not case_b:
            _, apart = run(case, on_device(case, masters(case)), base_a["gos"])
        assert_same(case, [], grads_of(case, t), [], apart, "beside %s" % (case_b.name if case is case_a else case_a.name))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_one_upstream_gradient_two_consumers(case):
    """((node(a) + node(b)) * w).sum(): both nodes are handed the SAME gradient tensor object -- neither may write into it, and both sets
    of gradients are those of the nodes run apart; the rows that name a second kind also share it with a node of another class"""
    _two_consumers(case, case)
    if case.second is not None:
        _two_consumers(case, AC.BY_NAME[case.second])


# ---- 4. a retained graph ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=repr)
def test_retained_graph(case):
    """backward(retain_graph=True) twice: the second pass gives the first's gradients, and no input, parameter, moving statistic or kept
    tensor changes during either"""
    base = baseline(case)
    t = on_device(case, masters(case))
    hold = {}
    outs = case.call(t, hold)
    kept = dict(t, **hold.get("internals", {}))
    before = {k: v.detach().clone() for k, v in kept.items() if v is not None}
    passes = []
    for _ in range(2):
        for k in case.grads + case.params:
            t[k].grad = None
        torch.autograd.backward(list(outs), base["gos"], retain_graph=True)
        passes.append(grads_of(case, t))
        for k, v in before.items():
            assert torch.equal(kept[k].detach(), v), "%s: %s changed during backward" % (case.name, k)
    assert_same(case, [o.detach() for o in outs], passes[0], base["outs"], base["grads"], "first pass over the retained graph")
    assert_same(case, [], passes[1], [], passes[0], "second pass over the retained graph")


# ---- 5. partial requires_grad ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=repr)
def test_partial_requires_grad(case):
    """inputs only, parameters only, neither, and forward under no_grad: what is asked for equals the full run, the rest stays None"""
    base = baseline(case)
    m = masters(case)
    subsets = [("inputs only", case.grads)] + ([("parameters only", case.params)] if case.params else [])
    for what, names in subsets:
        outs, grads = run(case, on_device(case, m, requires=names), base["gos"])
        assert_same(case, outs, grads, base["outs"], base["grads"], what, names=names)
        for k in set(case.grads + case.params) - set(names):
            assert grads[k] is None, "%s %s: %s got a gradient it did not ask for" % (case.name, what, k)
    outs = case.call(on_device(case, m, requires=()), None)
    assert all(not o.requires_grad and o.grad_fn is None for o in outs)
    assert_same(case, [o.detach() for o in outs], {}, base["outs"], {}, "nothing requires a gradient")
    with torch.no_grad():
        outs = case.call(on_device(case, m), None)
    assert all(o.grad_fn is None for o in outs)
    assert_same(case, list(outs), {}, base["outs"], {}, "under no_grad")


# ---- 6. in-place change between forward and backward ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in CASES if c.reread], ids=repr)
def test_in_place_change_between_forward_and_backward_raises(case):
    """every tensor the node's backward reads again, changed in place (by x1: the values stay) after the forward pass: RuntimeError, as
    from torch's own nodes -- never a gradient computed from other values than the forward pass saw"""
    base = baseline(case)
    m = masters(case)
    hold = {}
    case.call(on_device(case, m), hold)
    names = list(case.reread) + ["internal:" + k for k, v in hold.get("internals", {}).items() if v is not None]
    for name in names:
        t = on_device(case, m)
        hold = {}
        outs = case.call(t, hold)
        victim = hold["internals"][name[9:]] if name.startswith("internal:") else t[name]
        with torch.no_grad():
            victim.mul_(1)
        with pytest.raises(RuntimeError):
            torch.autograd.backward(list(outs), base["gos"])


# ---- 7. layer tensors that are views -------------------------------------------------------------------------------------------------

LAYERED = [AC.BY_NAME[n] for n in ("mlp_stack", "mlp_stack_pooled", "mlp_linear", "batch_norm")]


@pytest.mark.parametrize("case", LAYERED, ids=repr)
def test_layer_tensors_that_are_views(case):
    """mlp_stack, mlp_linear and batch_norm_template on a weight that is the .t() of (cout, cin) storage, a weight that is a column slice
    of a wider matrix, a gamma / bias / beta that is a strided slice -- every view spans its logical extent, so a bare-pointer read of
    it stays inside its allocation: results as for the contiguous clones, the gradient arrives with the parameter's shape; a moving
    statistic that is not contiguous is refused before anything runs"""
    base = baseline(case)
    m = masters(case)
    for name in case.params:
        for kind in KINDS:
            t = on_device(case, m, {name: kind})
            assert not t[name].is_contiguous()
            if kind == "permuted" and t[name].dim() == 2:
                assert t[name].t().is_contiguous()                      # the .t() view of (cout, cin) storage
            outs, grads = run(case, t, base["gos"])
            assert grads[name] is not None and grads[name].shape == t[name].shape
            assert_same(case, outs, grads, base["outs"], base["grads"], "%s as a %s view" % (name, kind))
    for name in case.state:
        for kind in KINDS:
            t = on_device(case, m, {name: kind})
            with pytest.raises(ValueError):
                case.call(t, None)
            assert torch.equal(t[name], m[name].float().cuda()), "%s was written to before it was refused" % name


# ---- 8. gradient sinks against the run without them ------------------------------------------------------------------------------------

SINK_ROWS, SINK_CIN, SINK_CHANS = 256, 32, [48, 32]


class _SinkRun:
    """the two-layer stack at 256 x 32 -> [48, 32] over a FlatGradBucket (+ FlatAdam), with or without sinks; the same seeds either way"""

    def __init__(self, sinks, frozen=(), lr=0.0, split=False):
        from gspn_amd import mlp, parallel
        g = torch.Generator().manual_seed(9)
        ms = AC._layer_masters(g, SINK_CHANS, SINK_CIN)
        self.t = {k: (torch.nn.Parameter(v.float().cuda(), requires_grad=k not in frozen) if k[0] in "wbg" else v.float().cuda()) for k, v in ms.items()}
        self.layers = AC.layer_params(self.t, 2)
        self.params = [p for lp in self.layers for p in lp.tensors()]
        self.bucket = parallel.FlatGradBucket(self.params)
        self.opt = parallel.FlatAdam(self.bucket, lr=lr)
        if sinks:
            self.bucket.attach_sinks()
        self.mlp, self.split = mlp, split
        self.xs = [torch.randn(SINK_ROWS, SINK_CIN, generator=g).cuda() for _ in range(3)]
        self.gos = [torch.randn(SINK_ROWS, SINK_CHANS[-1], generator=g).cuda() for _ in range(3)]

    def forward(self, k, hook=None):
        if not self.split:
            return self.mlp.mlp_stack(self.xs[k], SINK_CIN, self.layers, True, AC.DECAY)
        h = self.mlp.mlp_stack(self.xs[k], SINK_CIN, self.layers[:1], True, AC.DECAY)        # two nodes: a hook between them can raise midway
        if hook is not None:
            h.register_hook(hook)
        return self.mlp.mlp_stack(h, SINK_CHANS[0], self.layers[1:], True, AC.DECAY)

    def backward(self, k, hook=None):
        self.forward(k, hook).backward(self.gos[k])

    def reset(self, how):
        if how == "none":
            for p in self.params:
                p.grad = None
        else:
            self.opt.zero_grad()

    def flat(self):
        self.bucket.flatten()
        torch.cuda.synchronize()
        return self.bucket.flat.clone()

    def close(self):
        self.bucket.detach_sinks()
        assert not [k for k, e in self.mlp.GRAD_SINKS.items() if e.bucket is self.bucket] and not self.bucket._written


def _both(script, **kw):
    """script(run) -> tensor, without and with sinks; GRAD_SINKS is clean afterwards either way"""
    res = []
    for sinks in (False, True):
        r = _SinkRun(sinks, **kw)
        try:
            res.append(script(r))
        finally:
            r.close()
    return res


def test_sinks_accumulate_two_backward_passes():
    def script(r):
        r.reset("none")
        r.backward(0)
        assert len(r.bucket._written) == (len(r.params) if r.bucket.sinks else 0)      # with sinks every gradient of the first pass was claimed
        r.backward(1)
        return r.flat()
    plain, sunk = _both(script)
    assert float(plain.abs().max()) > 0 and torch.equal(plain, sunk)


@pytest.mark.parametrize("how", ["none", "zero_grad"])
def test_sinks_forget_a_step_abandoned_after_its_backward(how):
    """a backward pass, then every .grad reset (by hand; by the optimiser's zero_grad) and no flatten(): the next step's bucket holds the next
    step's gradients alone, as without sinks"""
    def script(r):
        r.reset(how)
        r.backward(0)                 # abandoned: no flatten() follows
        r.reset(how)
        r.backward(1)
        return r.flat()

    def clean(r):
        r.reset(how)
        r.backward(1)
        return r.flat()
    plain, sunk = _both(script)
    want, _ = _both(clean)
    assert torch.equal(plain, want) and torch.equal(sunk, plain)


def test_sinks_forget_a_backward_pass_that_raised_midway():
    class Midway(Exception):
        pass

    def stop(g):
        raise Midway()

    def script(r):
        r.reset("none")
        with pytest.raises(Midway):
            r.backward(0, stop)        # the second layer's node has run (and claimed its slices), the first has not
        r.reset("none")
        r.backward(1)
        return r.flat()
    plain, sunk = _both(script, split=True)
    assert float(plain.abs().max()) > 0 and torch.equal(plain, sunk)


def test_sinks_leave_a_frozen_parameter_alone():
    """requires_grad=False inside the bucket: its slice is zero and FlatAdam.step() does not move it, as without sinks"""
    frozen = ("w0", "gamma1")

    def script(r):
        before = {k: r.t[k].detach().clone() for k in r.t}
        r.reset("none")
        r.backward(0)
        flat = r.flat()
        off = 0
        for p, n in zip(r.params, r.bucket.sizes):
            if not p.requires_grad:
                assert float(flat[off:off + n].abs().max()) == 0.0
            off += n
        r.opt.step()
        torch.cuda.synchronize()
        for k in frozen:
            assert torch.equal(r.t[k].detach(), before[k]), "%s is frozen and moved" % k
        assert not torch.equal(r.t["w1"].detach(), before["w1"])
        return torch.cat([flat, r.opt.flat.detach().clone()])
    plain, sunk = _both(script, frozen=frozen, lr=1e-3)
    assert torch.equal(plain, sunk)


def test_autograd_grad_with_sinks_attached_returns_the_gradients_and_leaves_no_claim():
    def script(r):
        r.reset("none")
        out = r.forward(0)
        try:
            got = torch.autograd.grad(out, r.params, r.gos[0])
        except RuntimeError:
            got = None                 # refusing is within the contract; a silent None or a claim left behind is not
        assert not r.bucket._written, "a claim outlived torch.autograd.grad: the next step would be added onto it"
        r.reset("none")
        r.backward(0)
        flat = r.flat()
        if got is not None:
            assert all(g is not None for g in got)
            assert torch.equal(torch.cat([g.reshape(-1) for g in got]), flat)
        return flat
    plain, sunk = _both(script)
    assert torch.equal(plain, sunk)


def test_a_layer_tensor_made_contiguous_takes_no_sink():
    """a weight handed in as the .t() of its stored transpose: its gradient reaches the stored parameter through autograd, with the stored
    shape, and flatten() gathers it -- the same gradient, bit for bit, as when the bucket's parameter is the weight itself and takes the sink"""
    from gspn_amd import mlp, parallel
    g = torch.Generator().manual_seed(3)
    ms = AC._layer_masters(g, SINK_CHANS[:1], SINK_CIN)
    x = torch.randn(SINK_ROWS, SINK_CIN, generator=g).cuda()
    go = torch.randn(SINK_ROWS, SINK_CHANS[0], generator=g).cuda()
    res = []
    for stored_transposed in (False, True):
        t = {k: v.float().cuda() for k, v in ms.items()}
        store = torch.nn.Parameter(t["w0"].t().contiguous() if stored_transposed else t["w0"])
        rest = [torch.nn.Parameter(t[k]) for k in ("b0", "beta0", "gamma0")]
        bucket = parallel.FlatGradBucket([store] + rest).attach_sinks()
        try:
            lp = mlp.LayerParams(store.t() if stored_transposed else store, rest[0], True, rest[1], rest[2], t["mm0"], t["mv0"])
            mlp.mlp_stack(x, SINK_CIN, [lp], True, AC.DECAY).backward(go)
            assert (0 in bucket._written) == (not stored_transposed)
            bucket.flatten()
            torch.cuda.synchronize()
            dw = bucket.flat[:store.numel()].view(store.shape)
            res.append((dw.t() if stored_transposed else dw).clone())
            assert store.grad.shape == store.shape
        finally:
            for k in [k for k, e in mlp.GRAD_SINKS.items() if e.bucket is bucket]:
                del mlp.GRAD_SINKS[k]
    assert float(res[0].abs().max()) > 0 and torch.equal(res[0], res[1])
