"""Stream order: the harness of tests/test_gpu_stream_order.py.

include/gspn_hip.h hands every launcher a stream and every Python wrapper passes torch's current one, and the product never runs on the
null stream (bench.py steps on a prioritised stream, prefetches geometry on GeometryStreams, graph.CapturedStep captures on a side
stream) -- while a value test on the null stream cannot see a kernel launched with 0 instead of `st`, a memset on the wrong stream, a
helper kernel of a multi-launch entry point left behind on another stream, or a side-stream reduction that is never joined.  The contract
("Every op on a side stream"): an entry point enqueues ALL its work on the stream it is given, or joins back to it before
it returns.  Two scenarios make a breach visible as a stale or zero read of memory the test owns; nothing faults.

    B  held_default(case)             the NULL stream is kept busy by a finite spin kernel while the op runs on a side stream that sits on
                                      another hardware queue.  Whatever the op put on the null stream is still waiting behind the spin when
                                      the caller's stream has finished and cloned the results: the clones then differ from a plain run.
    A  late_inputs(fn, late, ...)     the CALLER's stream is busy (spin) and its inputs are written behind the spin, on that stream; until
                                      then they hold a valid decoy.  Work that does not queue up behind the caller's stream reads the decoy.

A plain module like tests/arena.py: no conftest, no plugin, no pytest setting.  The spin length is no tolerance: it only decides whether a
run is CONCLUSIVE (the spin still ran when the observed stream finished).  An inconclusive run fails (Inconclusive)."""
import time

import torch

from tests.arena import Arena, assert_same_bits, flatten

OTHER_STREAM = "part of the op ran on a stream other than the caller's"
READ_EARLY = "the op read an input before the caller's stream had written it"
CAL_CYCLES = 2000000            # the one timed _sleep of the calibration
_side = None                    # the one GeometryStream behind side_stream()
_cycles_per_ms = None


class Inconclusive(AssertionError):
    """the spin had ended when it was looked at: the run cannot tell a right stream from a wrong one"""


def map_tensors(result, f):
    """A nested result (tuples, lists, dicts; None and python scalars kept) with f applied to every tensor: the shape arena.flatten reads."""
    if result is None or isinstance(result, (int, float, bool, str)):
        return result
    if isinstance(result, torch.Tensor):
        return f(result)
    if isinstance(result, dict):
        return {k: map_tensors(v, f) for k, v in result.items()}
    if isinstance(result, (tuple, list)):
        return type(result)(map_tensors(v, f) for v in result)
    raise TypeError("a case returned a %s" % type(result).__name__)


def _null():
    null = torch.cuda.default_stream()
    assert torch.cuda.current_stream() == null, "the harness is entered on the null stream"
    return null


def side_stream():
    """The stream the ops are moved to: one per process, on another hardware queue than the null stream (GeometryStream tests that with
    a spin, not by asking).  Two streams on one queue are serialised and every check of this module would pass vacuously: asserted."""
    global _side
    if _side is None:
        from gspn_amd.geometry import GeometryStream
        null = _null()
        g = GeometryStream(torch.device("cuda", torch.cuda.current_device()), beside=[null])
        assert not g.shares_queue, "no stream runs beside the null stream (%d tried): the hardware queues are taken" % g.tried
        _side = g
    return _side.stream


def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond, measured once per process: one _sleep of CAL_CYCLES between two events (behind a short
    one that loads the kernel)."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        torch.cuda.synchronize()
        torch.cuda._sleep(1000)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(CAL_CYCLES)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.05, "a _sleep of %d cycles took %.4f ms: too short to calibrate on" % (CAL_CYCLES, ms)
        _cycles_per_ms = CAL_CYCLES / ms
    return _cycles_per_ms


def spin_cycles(ms):
    return max(1, int(ms * cycles_per_ms()))


def _clone(result):
    return map_tensors(result, lambda t: t.detach().clone())


def held_default(case, device_wide_sync=None):
    """Scenario B.  case: an arena.Case built on the null stream.  device_wide_sync: the DEVICE_WIDE_SYNC row of a case whose op promises to
    synchronise the device -- only then may the run be inconclusive (the values are compared all the same).  Returns (plain_ms, spin_ms)."""
    null, side = _null(), side_stream()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plain = case.fn()
    torch.cuda.synchronize()
    plain_ms = (time.perf_counter() - t0) * 1e3
    assert flatten(plain), "%s returned no tensor" % case.name
    spin_ms = 3.0 * plain_ms + 20.0
    cycles = spin_cycles(spin_ms)
    try:
        torch.cuda._sleep(cycles)
        spun = null.record_event()
        with torch.cuda.stream(side):
            with Arena(0x00):           # what a mis-streamed kernel has not written yet reads as zeros: a valid index, a finite float
                got = case.fn()
            clones = _clone(got)
            done = side.record_event()
        done.synchronize()
        conclusive = not spun.query()
    finally:
        torch.cuda.synchronize()
    if not conclusive and device_wide_sync is None:
        raise Inconclusive("%s: the %.1f ms spin on the null stream (3 x the plain run's %.2f ms + 20) had ended when the side stream finished: "
                           "the op waited for the device, or the side stream did not run beside the null stream" % (case.name, spin_ms, plain_ms))

    def same(res, what):
        if case.atomic is not None:
            case.verify(res)
        else:
            assert_same_bits(res, plain, "%s, %s vs the plain run" % (case.name, what), case.mask, case.canon)
    try:
        same(clones, "cloned on the side stream")
    except AssertionError as e:
        try:
            same(got, "read after the device synchronised")
        except AssertionError:
            raise AssertionError("%s: the op's results depend on the stream it runs on: beside a busy null stream the clones AND the originals "
                                 "read after a device-wide synchronisation differ from the plain run (work that feeds the op's later "
                                 "kernels may have gone to another stream).\n%s" % (case.name, e)) from e
        raise AssertionError("%s: %s: the results cloned on the caller's stream differ from the plain run, the originals read after a "
                             "device-wide synchronisation agree with it.\n%s" % (case.name, OTHER_STREAM, e)) from e
    return plain_ms, spin_ms


def late_inputs(fn, late, spin_ms=None, same=None, what="late_inputs"):
    """Scenario A.  fn() reads the tensors of `late` = [(tensor, real, decoy)] (all device resident, real and decoy of tensor's shape) and
    returns its results; it must not synchronise the host.  Runs fn plainly on the decoy and on real (null stream, synchronised), asserts
    that the two answers differ (the decoy discriminates), puts the decoy back, and then on the side stream enqueues [spin, tensor <- real,
    fn(), clones].  The spin must still run when fn returns on the host; the clones must be the answer on real.  same(got, want) raises
    AssertionError where two results differ (default: bit equality).  Returns the plain result on real: the caller holds it to its oracle."""
    null, side = _null(), side_stream()
    if same is None:
        def same(got, want):
            assert_same_bits(got, want, what)

    def fill(which):
        for t, real, decoy in late:
            t.copy_(real if which == "real" else decoy)
        torch.cuda.synchronize()

    fill("decoy")
    on_decoy = _clone(fn())
    fill("real")
    t0 = time.perf_counter()
    expected = _clone(fn())
    torch.cuda.synchronize()
    plain_ms = (time.perf_counter() - t0) * 1e3
    assert flatten(expected), "%s returned no tensor" % what
    try:
        same(on_decoy, expected)
    except AssertionError:
        pass
    else:
        raise AssertionError("%s: the decoy gives the answer of the real input: it cannot show a read that came too early" % what)
    fill("decoy")
    spin_ms = 3.0 * plain_ms + 20.0 if spin_ms is None else float(spin_ms)
    cycles = spin_cycles(spin_ms)
    try:
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
            spun = side.record_event()
            for t, real, _ in late:
                t.copy_(real)
            got = fn()
            conclusive = not spun.query()
            clones = _clone(got)
        del got
    finally:
        torch.cuda.synchronize()
    if not conclusive:
        raise Inconclusive("%s: the %.1f ms spin in front of the inputs had ended when the call returned on the host: the op synchronises "
                           "the host (scenario A is for ops that do not), or the spin is too short for the enqueue" % (what, spin_ms))
    try:
        same(clones, expected)
    except AssertionError as e:
        try:
            same(clones, on_decoy)
        except AssertionError:
            raise e
        raise AssertionError("%s: %s: the result is the decoy's.\n%s" % (what, READ_EARLY, e)) from e
    return expected
