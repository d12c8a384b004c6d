"""Every op on a side stream while the null stream is held busy, and behind inputs that arrive late (tests/stream_order.py).

Sweep B: held_default over every builder of the nine arena tables (tests/test_gpu_arena_*.py: each op at its smallest interesting
shape, with its own rule of comparison -- mask, canonical form, or the float64 verify of a float-atomic row), and two mlp_stack rows
under mlp.DEFER_DW, the one place in the package that launches on an internal side stream.  A spin kernel occupies the null stream; the
op runs on a stream on another hardware queue under Arena(0x00) and its results are cloned there.  Whatever part of the op went to the
null stream is still queued behind the spin then, and the clones differ from the plain run.

Scenario A: six ops that do not synchronise the host, enqueued behind [spin, copy of the real inputs] on their own stream, their input
buffers holding a valid decoy until the copy runs.  The GeometryStream / PendingGeometry tests are the prefetch path of bench.py.

The four controls at the end show that the harness can fail: a multiply on the null stream, a read on the null stream, a device-wide
synchronisation (inconclusive, in both scenarios), and a correct op that passes.  Nothing here faults: every mis-ordering is a stale or
zero read of memory the test owns."""
import contextlib
import glob
import importlib
import os
import time

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import data as D
from tests import stream_order as SO
from tests.arena import Case, flatten

pytestmark = pytest.mark.gpu

TABLES = ("components", "geometry", "holes", "layers", "lift", "mask_nms", "nearest", "segments", "stages")
SWEEP = [(t, build) for t in TABLES for build in importlib.import_module("tests.test_gpu_arena_" + t).CASES]

# case id -> (file:line of a device-wide synchronisation, the sentence of the op's docstring that promises it).  Only a row here may be
# inconclusive under the sweep.  In gspn_amd/ only graph.py:29 and geometry.runs_beside synchronise the device and no case reaches them.
DEVICE_WIDE_SYNC = {}

TIMES = {}          # test id -> (seconds, plain ms, spin ms)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def leaf(t):
    return t.detach().requires_grad_(True)


@contextlib.contextmanager
def _defer_dw():
    """mlp.DEFER_DW switched on and put back the way tests/test_gpu_modules.py:306 does, with mlp.py's internal stream on a hardware queue
    of its own (a GeometryStream tested beside the null stream and the caller's).  HIP hands its queues to streams round-robin in
    creation order: in the whole suite the internal stream landed on the NULL stream's queue, its gspn_mlp_bwd_dw was serialised behind
    the spin, the join made the caller's stream wait for it, and both rows came out inconclusive.  Yields the internal stream."""
    from gspn_amd import mlp as M
    _, geo = _streams()
    key = ("cuda", torch.cuda.current_device())
    old, M.DEFER_DW = M.DEFER_DW, True
    had = M._side_streams.get(key)
    M._side_streams[key] = geo.stream
    try:
        yield geo.stream
    finally:
        torch.cuda.synchronize()
        M.DEFER_DW = old
        if had is None:
            del M._side_streams[key]
        else:
            M._side_streams[key] = had


def _held(name, case):
    t0 = time.perf_counter()
    plain_ms, spin_ms = SO.held_default(case, DEVICE_WIDE_SYNC.get(name))
    TIMES[name] = (time.perf_counter() - t0, plain_ms, spin_ms)


# ---- sweep B ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [f for _, f in SWEEP], ids=lambda f: f.__name__)
def test_held_default(build):
    _held(build.__name__, build())


DEFER_ROWS = [
    # name, rows, ld, cin, chans, pool_ns           (tests/test_gpu_arena_layers.py: generic_ragged_rows and pooled_top_layer_ns32)
    ("defer_dw_dense", 3000, 20, 20, [24, 40, 16], None),
    ("defer_dw_pooled_ns32", 4096, 32, 32, [32, 64, 48], 32),
]


@pytest.mark.parametrize("row", DEFER_ROWS, ids=[r[0] for r in DEFER_ROWS])
def test_held_default_defer_dw(row):
    """gspn_mlp_bwd_dw on mlp.py's internal side stream, joined back before backward returns: the caller's clones hold every dW"""
    from tests.test_gpu_arena_layers import stack_case
    name, rows, ld, cin, chans, ns = row
    with _defer_dw():
        _held(name, stack_case("mlp_stack %s under DEFER_DW" % name, rows, ld, cin, chans, ns))


def test_zz_every_arena_table_is_swept():
    here = os.path.dirname(os.path.abspath(__file__))
    found = sorted(os.path.basename(p)[len("test_gpu_arena_"):-3] for p in glob.glob(os.path.join(here, "test_gpu_arena_*.py")))
    assert found == sorted(TABLES), "an arena table is not in TABLES above: %s" % sorted(set(found) ^ set(TABLES))
    swept = {id(f) for _, f in SWEEP}
    total = 0
    for t in found:
        cases = importlib.import_module("tests.test_gpu_arena_" + t).CASES
        assert cases and all(id(f) in swept for f in cases), "tests/test_gpu_arena_%s.py has cases outside the sweep" % t
        total += len(cases)
    assert total == len(SWEEP)
    names = [f.__name__ for _, f in SWEEP]
    assert len(set(names)) == len(names), "two arena cases share a name: the ids of the sweep (and DEVICE_WIDE_SYNC) are the names"
    assert set(DEVICE_WIDE_SYNC) <= set(names)
    for where, promise in DEVICE_WIDE_SYNC.values():
        assert ":" in where and promise
    print("\ntests/test_gpu_stream_order.py: %d arena cases + %d DEFER_DW rows swept, DEVICE_WIDE_SYNC = %r, %.0f _sleep cycles per ms"
          % (len(SWEEP), len(DEFER_ROWS), DEVICE_WIDE_SYNC, SO.cycles_per_ms()))
    if TIMES:
        slow = max(TIMES, key=lambda k: TIMES[k][0])
        print("slowest swept case: %s %.2f s (plain run %.1f ms, spin %.1f ms); all %d: %.1f s"
              % (slow, TIMES[slow][0], TIMES[slow][1], TIMES[slow][2], len(TIMES), sum(v[0] for v in TIMES.values())))


# ---- scenario A ------------------------------------------------------------------------------------------------------------------------
def close(got, ref, scale, tol=1e-5):
    """tests/test_gpu_dropin_grads.py: |got - ref| <= tol * (the sum of |terms| that went into each element)"""
    got, ref = np.asarray(got.detach().cpu().numpy(), np.float64), np.asarray(ref, np.float64)
    bound = tol * np.maximum(np.asarray(scale, np.float64), 1e-30) + 1e-12
    assert np.isfinite(got).all() and (np.abs(got - ref) <= bound).all()


def test_late_farthest_point_sample():
    """n = 8192: the pre-pass and the cells kernel, both behind the copy"""
    from gspn_amd import tf_sampling as S
    assert S.FPS_MODE == "cells" and S.FPS_CELLS_MIN_N <= 8192
    cloud = D.batch("S", 1, 8192, 31)
    real = dev(cloud)
    xyz = torch.empty_like(real)
    want = SO.late_inputs(lambda: S.farthest_point_sample(64, xyz), [(xyz, real, real.flip(1).contiguous())], what="farthest_point_sample n=8192")
    np.testing.assert_array_equal(want.cpu().numpy(), O.farthest_point_sample(64, cloud))


def test_late_query_ball_point():
    from gspn_amd.tf_grouping import query_ball_point
    from tests.test_gpu_ball_query_ragged import grid_case
    cloud, q, radius, ns = grid_case("capped", 8192)
    real, t_q = dev(cloud), dev(q)
    xyz = torch.empty_like(real)
    idx, cnt = SO.late_inputs(lambda: query_ball_point(radius, ns, xyz, t_q), [(xyz, real, real.flip(1).contiguous())],
                              what="query_ball_point n=8192 (gspn_queryballpoint_ws)")
    ridx, rcnt = O.query_ball_point(radius, ns, cloud, q)
    np.testing.assert_array_equal(cnt.cpu().numpy(), rcnt)
    np.testing.assert_array_equal(idx.cpu().numpy()[rcnt > 0], ridx[rcnt > 0])        # (tests/test_gpu_ball_query_ragged.py: rows with a hit)


def test_late_three_nn_three_interpolate():
    """three_nn against a late cloud, three_interpolate forward and its gradient through the inverse lists (built inside backward) with a
    late grad_out"""
    from gspn_amd import invlists
    from gspn_amd.tf_interpolate import three_interpolate, three_nn
    b, n, m, c = 2, 4096, 512, 32
    assert not invlists.use_atomic(c)
    qc, kc = D.batch("U", b, n, 41), D.batch("U", b, m, 42)
    g = torch.Generator().manual_seed(3)
    q, known_real, pts, go_real = dev(qc), dev(kc), torch.randn(b, m, c, generator=g).cuda(), torch.randn(b, n, c, generator=g).cuda()
    known, go = torch.empty_like(known_real), torch.empty_like(go_real)

    def fn():
        x = leaf(pts)
        dist, idx = three_nn(q, known)
        w = 1.0 / dist.clamp_min(1e-10)
        w = w / w.sum(2, keepdim=True)
        out = three_interpolate(x, idx, w)
        out.backward(go)
        return dist, idx, out.detach(), x.grad
    dist, idx, out, dx = SO.late_inputs(fn, [(known, known_real, known_real.flip(1).contiguous()), (go, go_real, -go_real)],
                                        what="three_nn + three_interpolate + gradient")
    rd, ri = O.three_nn(qc, kc)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(dist.cpu().numpy(), rd)
    w = 1.0 / np.maximum(rd.astype(np.float64), 1e-10)
    w = (w / w.sum(2, keepdims=True))
    p64, g64 = pts.cpu().numpy().astype(np.float64), go_real.cpu().numpy().astype(np.float64)
    rout = sum(w[:, :, t, None] * np.take_along_axis(p64, ri[:, :, t, None].astype(np.int64), 1) for t in range(3))
    close(out, rout, sum(w[:, :, t, None] * np.abs(np.take_along_axis(p64, ri[:, :, t, None].astype(np.int64), 1)) for t in range(3)))
    rdx, sdx = np.zeros_like(p64), np.zeros_like(p64)
    for s in range(b):
        for t in range(3):
            np.add.at(rdx[s], ri[s, :, t], w[s, :, t, None] * g64[s])
            np.add.at(sdx[s], ri[s, :, t], w[s, :, t, None] * np.abs(g64[s]))
    close(dx, rdx, sdx)


def test_late_group_point_grad():
    """c = 64: the gather form, its inverse lists built inside the call, behind the late grad_out"""
    from gspn_amd import invlists
    from gspn_amd.tf_grouping import group_point
    from tests.test_gpu_arena_geometry import _group_inputs
    assert not invlists.use_atomic(64)
    pts, idx, go_np = _group_inputs(64)
    t_pts, t_idx, go_real = dev(pts), dev(idx), dev(go_np)
    go = torch.empty_like(go_real)

    def fn():
        x = leaf(t_pts)
        out = group_point(x, t_idx)
        out.backward(go)
        return out.detach(), x.grad
    out, dx = SO.late_inputs(fn, [(go, go_real, -go_real)], what="group_point c=64 + gradient")
    np.testing.assert_array_equal(out.cpu().numpy(), O.group_point(pts, idx))
    close(dx, O.group_point_grad(np.zeros_like(pts), idx, go_np), O.group_point_grad(np.zeros_like(pts), idx, np.abs(go_np)))


def test_late_nn_distance():
    """n + m = 4100: the search both ways, then the gradient as a gather through both inverse lists"""
    from gspn_amd import tf_nndistance as T
    b, n, m = 2, 4000, 100
    assert n + m > T.LDS_GRAD_MAX_POINTS
    rng = np.random.default_rng(3)
    a, c = rng.random((b, n, 3), dtype=np.float32), rng.random((b, m, 3), dtype=np.float32)
    g1, g2 = rng.standard_normal((b, n)).astype(np.float32), rng.standard_normal((b, m)).astype(np.float32)
    a_real, t_c, g1_real, t_g2 = dev(a), dev(c), dev(g1), dev(g2)
    t_a, t_g1 = torch.empty_like(a_real), torch.empty_like(g1_real)

    def fn():
        x, y = leaf(t_a), leaf(t_c)
        d1, i1, d2, i2 = T.nn_distance(x, y)
        (d1 * t_g1).sum().add((d2 * t_g2).sum()).backward()
        return d1.detach(), i1, d2.detach(), i2, x.grad, y.grad
    res = SO.late_inputs(fn, [(t_a, a_real, a_real.flip(1).contiguous()), (t_g1, g1_real, -g1_real)], what="nn_distance + gradient")
    rd1, ri1, rd2, ri2 = O.nn_distance(a, c)
    for got, want in zip(res[:4], (rd1, ri1, rd2, ri2)):
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    rg1, rg2 = O.nn_distance_grad(a, c, g1, ri1, g2, ri2)
    np.testing.assert_allclose(res[4].cpu().numpy(), rg1, rtol=1e-5, atol=1e-5)       # tests/test_gpu_kernel_instances.py:362
    np.testing.assert_allclose(res[5].cpu().numpy(), rg2, rtol=1e-5, atol=1e-5)


def test_late_defer_dw_backward():
    """mlp.DEFER_DW: every layer's dW reduction on the internal side stream must wait for the caller's stream, which still holds the spin
    and the copy of the upstream gradient, and be joined back before the clones.  The expected result is the plain run's (no oracle
    covers this placement of the sums; tests/test_gpu_modules.py holds it to the default placement)."""
    from gspn_amd import mlp as M
    from tests.test_gpu_mlp import make_params, to_layers
    rows, cin, chans = 3000, 20, [24, 40, 16]
    g = torch.Generator().manual_seed(11)
    x0, go_real = torch.randn(rows, cin, generator=g).cuda(), torch.randn(rows, chans[-1], generator=g).cuda()
    go = torch.empty_like(go_real)
    layers = to_layers(make_params(chans, cin, 3))

    def fn():
        for lp in layers:
            for t in lp.tensors():
                t.grad = None
        x = leaf(x0)
        out = M.mlp_stack(x, cin, layers, True, 0.7)
        out.backward(go)
        return out.detach(), x.grad, [[t.grad for t in lp.tensors()] for lp in layers]
    with _defer_dw():
        SO.late_inputs(fn, [(go, go_real, -go_real)], what="mlp_stack backward under DEFER_DW")


# ---- GeometryStream and PendingGeometry ------------------------------------------------------------------------------------------------
_geo = None


def _streams():
    """the main stream (non-null, beside the null stream) and a GeometryStream beside both"""
    global _geo
    from gspn_amd.geometry import GeometryStream
    main = SO.side_stream()
    if _geo is None:
        _geo = GeometryStream(torch.device("cuda", torch.cuda.current_device()), beside=[torch.cuda.default_stream(), main])
        assert not _geo.shares_queue
    return main, _geo


def _sa(x):
    from gspn_amd.geometry import sa_geometry
    return sa_geometry(x, 64, 0.2, 16)


_GEOMETRY = []


def _geometry_inputs():
    """the real cloud, its decoy and the plain run's geometry of the real one: computed once, never written"""
    if not _GEOMETRY:
        real = dev(D.batch("U", 2, 1024, 77))
        decoy = real.flip(1).contiguous()
        want = SO._clone(_sa(real).tensors())
        other = SO._clone(_sa(decoy).tensors())
        torch.cuda.synchronize()
        assert not all(torch.equal(a, b) for a, b in zip(want, other)), "the decoy cloud has the geometry of the real one"
        _GEOMETRY.extend((real, decoy, want))
    return tuple(_GEOMETRY)


def _same_geometry(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), "%s: geometry tensor %d differs from the plain run's on the real cloud" % (what, i)


@pytest.mark.parametrize("after", ["current", "event"])
def test_geometry_submit_waits_for_the_callers_stream(after):
    """(a) submit() behind [spin, xyz <- real] on the caller's non-null stream: the geometry is that of the real cloud"""
    main, geo = _streams()
    real, decoy, want = _geometry_inputs()
    xyz = decoy.clone()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(main):
            torch.cuda._sleep(SO.spin_cycles(30))
            spun = main.record_event()
            xyz.copy_(real)
            pend = geo.submit(_sa, xyz, after="current" if after == "current" else main.record_event())
            value = pend.get()
            running = not spun.query()
            clones = SO._clone(value.tensors())
    finally:
        torch.cuda.synchronize()
    assert running, "inconclusive: the 30 ms spin had ended when get() returned"
    _same_geometry(clones, want, "submit(after=%s)" % after)


@pytest.mark.parametrize("host_wait", [False, True])
def test_pending_geometry_get_waits_for_the_geometry_stream(host_wait):
    """(b) a spin on the geometry stream in front of the work: the consumer's clones behind get() hold the finished geometry"""
    main, geo = _streams()
    real, _, want = _geometry_inputs()
    try:
        with torch.cuda.stream(main):
            with torch.cuda.stream(geo.stream):
                torch.cuda._sleep(SO.spin_cycles(30))
                spun = geo.stream.record_event()
            pend = geo.submit(_sa, real, after=None)
            value = pend.get(host_wait=host_wait)
            running = not spun.query()
            clones = SO._clone(value.tensors())
    finally:
        torch.cuda.synchronize()
    assert running != host_wait, "host_wait=%s: the spin %s when get() returned" % (host_wait, "still ran" if running else "had ended (inconclusive)")
    _same_geometry(clones, want, "get(host_wait=%s)" % host_wait)


def test_pending_geometry_hands_its_blocks_over_to_the_consumer():
    """(c) geometry.py:145, record_stream: the consumer still reads the geometry (behind a spin) when its producer drops it and allocates
    again on the geometry stream.  Without the hand-over the caching allocator gives the same blocks straight back and the zero fill
    below lands under the consumer's clones."""
    main, geo = _streams()
    real, _, want = _geometry_inputs()
    try:
        with torch.cuda.stream(main):
            pend = geo.submit(_sa, real, after=None)
            value = pend.get()
            torch.cuda._sleep(SO.spin_cycles(30))
            spun = main.record_event()
            clones = SO._clone(value.tensors())
        shapes = [(tuple(t.shape), t.dtype) for t in value.tensors()]
        del value, pend
        with torch.cuda.stream(geo.stream):
            again = [torch.zeros(s, dtype=d, device="cuda") for s, d in shapes]
            filled = geo.stream.record_event()
        filled.synchronize()
        running = not spun.query()
    finally:
        torch.cuda.synchronize()
    assert running, "inconclusive: the 30 ms spin had ended before the zero fill on the geometry stream"
    del again
    _same_geometry(clones, want, "clones taken behind a spin while the producer reallocates")


def test_defer_dw_is_joined_back_to_the_callers_stream():
    """mlp.py:391, the join.  The sweep holds the NULL stream busy, which delays nothing on mlp.py's internal side stream, so a missing
    join would only be a race there.  Here the internal stream itself is held by a spin (a stream beside the caller's is put in its
    place for the test): every gspn_mlp_bwd_dw waits behind it, and the clones taken on the caller's stream when backward has returned
    hold every dW only if backward made the caller's stream wait."""
    from tests.arena import Arena, assert_same_bits
    from tests.test_gpu_arena_layers import stack_case
    main, _ = _streams()
    name, rows, ld, cin, chans, ns = DEFER_ROWS[0]
    with _defer_dw() as inner:
        case = stack_case("mlp_stack %s under DEFER_DW, its internal stream held" % name, rows, ld, cin, chans, ns)
        plain = case.fn()
        torch.cuda.synchronize()
        with torch.cuda.stream(inner):
            torch.cuda._sleep(SO.spin_cycles(30))
            spun = inner.record_event()
        with torch.cuda.stream(main):
            with Arena(0x00):
                got = case.fn()
            running = not spun.query()
            clones = SO._clone(got)
    assert running, "inconclusive: the 30 ms spin on the internal stream had ended when backward returned on the host"
    assert_same_bits(clones, plain, "%s: cloned on the caller's stream vs the plain run" % case.name)


# ---- the controls: the harness can fail --------------------------------------------------------------------------------------------------
def test_control_held_default():
    x = torch.arange(4096, dtype=torch.float32, device="cuda") + 1.0

    def wrong_stream():
        with torch.cuda.stream(torch.cuda.default_stream()):
            return torch.mul(x, 2.0, out=torch.empty_like(x))

    def waits_for_the_device():
        out = torch.mul(x, 2.0, out=torch.empty_like(x))
        torch.cuda.synchronize()
        return out
    with pytest.raises(AssertionError, match="other than the caller's"):
        SO.held_default(Case("multiplies on the null stream", wrong_stream))
    with pytest.raises(SO.Inconclusive):
        SO.held_default(Case("synchronises the device", waits_for_the_device))
    SO.held_default(Case("multiplies on its stream", lambda: torch.mul(x, 2.0, out=torch.empty_like(x))))


def test_control_late_inputs():
    real = torch.arange(4096, dtype=torch.float32, device="cuda") + 1.0
    x = torch.empty_like(real)
    late = [(x, real, real.flip(0).contiguous())]

    def reads_on_the_null_stream():
        with torch.cuda.stream(torch.cuda.default_stream()):
            return x * 2.0

    def waits_for_the_device():
        out = x * 2.0
        torch.cuda.synchronize()
        return out
    with pytest.raises(AssertionError, match="before the caller's stream had written it") as e:
        SO.late_inputs(reads_on_the_null_stream, late, spin_ms=30)
    assert "the decoy's" in str(e.value)
    with pytest.raises(SO.Inconclusive):
        SO.late_inputs(waits_for_the_device, late, spin_ms=30)
    want = SO.late_inputs(lambda: x * 2.0, late, spin_ms=30)
    assert torch.equal(want, real * 2.0)
    with pytest.raises(AssertionError, match="cannot show a read that came too early"):
        SO.late_inputs(lambda: x * 0.0, late, spin_ms=30)


def test_control_streams_and_calibration():
    """the side stream runs beside the null stream, and a spin of spin_cycles(ms) lasts about ms"""
    from gspn_amd.geometry import runs_beside
    side = SO.side_stream()
    assert side != torch.cuda.default_stream() and runs_beside(torch.cuda.default_stream(), side, cycles=SO.spin_cycles(2))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(SO.spin_cycles(20))
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    print("\n_sleep: %.0f cycles per ms; a spin asked to last 20 ms lasted %.2f ms" % (SO.cycles_per_ms(), ms))
    assert 10.0 < ms < 40.0
    res = SO.map_tensors({"a": [torch.ones(2), None], "b": (3, torch.zeros(1))}, lambda t: t + 1)
    assert [k for k, _ in flatten(res)] == ["out['a'][0]", "out['b'][1]"] and float(res["a"][0][0]) == 2.0 and res["b"][0] == 3
