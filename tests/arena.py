"""Poisoned, guard-banded allocations: the harness of tests/test_cpu_arena.py and tests/test_gpu_arena_*.py.

include/gspn_hip.h promises that an entry point writes all of what it owns (gradient outputs are zeroed inside), that workspaces and
statistics buffers need not be zeroed, and that every *_ws_bytes / *_work_bytes / *_part_floats answer is the exact size the kernels stay
inside.  A fresh torch.empty in a test process is nearly always a zero page, and a store a few elements past a tensor lands in the
caching allocator's slack, so neither half of that contract is visible to a value test.  Arena makes both visible:

    with Arena(0xFF) as a:            # torch.empty / empty_like / zeros / zeros_like / full now hand out the middle of a larger
        out = wrapper(inputs)         # tensor whose every byte -- guard bands AND payload -- was set to 0xFF first
        a.check()                     # synchronises; both guard bands of every allocation must still be 0xFF, byte for byte

A plain module: no conftest, no plugin, no pytest setting.  sweep() below runs one case unpatched and under the three fills and asserts
guards (A), bit-independence of the fill (B) and the documented-unwritten masks (C) of the issue that introduced it ("Every op on poisoned, guard-banded allocations").
"""
import numbers
import os
import sys

import torch

FILLS = (0x00, 0xFF, 0x7F)          # 0x00 first: the clean run's evidence exists before a dirty one
_PATCHED = ("empty", "empty_like", "zeros", "zeros_like", "full")
_HERE = os.path.abspath(__file__)
_TESTS = os.path.dirname(_HERE) + os.sep
_PKG = os.sep + "gspn_amd" + os.sep
_open = None                        # the one open Arena (nesting is an error)


class GuardError(AssertionError):
    pass


class _Record:
    __slots__ = ("arena", "G", "shape", "dtype", "site")

    def __init__(self, arena, G, shape, dtype, site):
        self.arena, self.G, self.shape, self.dtype, self.site = arena, G, shape, dtype, site


def _site():
    """file:line of the innermost frame inside gspn_amd/ or a test module (this file excluded)."""
    f = sys._getframe(2)
    while f is not None:
        fn = f.f_code.co_filename
        if fn != _HERE and not fn.endswith(os.sep + "arena.py"):
            a = os.path.abspath(fn)
            if _PKG in a or a.startswith(_TESTS):
                return "%s:%d" % (os.path.relpath(a, os.path.dirname(_TESTS[:-1])), f.f_lineno)
        f = f.f_back
    return "<outside gspn_amd and tests>"


def _size_of(args):
    """the shape of torch.empty(*args): one sequence or the dimensions themselves, as Python or numpy integers or 0-d integer tensors"""
    one = lambda a: isinstance(a, numbers.Integral) or (isinstance(a, torch.Tensor) and a.dim() == 0 and not a.is_floating_point())   # noqa: E731
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    if all(one(a) for a in args):
        return tuple(int(a) for a in args)
    return None


def _default_device():
    return torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")


class Arena:
    def __init__(self, fill, device_type="cuda", guard_bytes=256):
        assert 0 <= int(fill) <= 255 and guard_bytes > 0 and guard_bytes % 16 == 0
        self.fill, self.device_type, self.guard_bytes = int(fill), device_type, int(guard_bytes)
        self.records = []
        self.passed = []             # device allocations that went to the original function: (site, shape, dtype, function)
        self._orig = None

    # ---- the patch -------------------------------------------------------------------------------------------------------------
    def __enter__(self):
        global _open
        if _open is not None:
            raise RuntimeError("Arena: nesting two arenas is an error")
        if self.device_type == "cuda" and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Arena: a stream capture is open (the fills would be captured and check() cannot synchronise)")
        self._orig = {n: getattr(torch, n) for n in _PATCHED}
        _open = self
        torch.empty = self._make_plain("empty", None)
        torch.zeros = self._make_plain("zeros", 0)
        torch.full = self._make_full()
        torch.empty_like = self._make_like("empty_like", None)
        torch.zeros_like = self._make_like("zeros_like", 0)
        return self

    def __exit__(self, *exc):
        global _open
        for n, f in self._orig.items():
            setattr(torch, n, f)
        _open = None
        return False

    def _carve(self, shape, dtype, device, value, requires_grad):
        """The patched allocation proper: numel + 2G elements, every byte = fill, the middle returned."""
        numel = 1
        for s in shape:
            numel *= s
        G = self.guard_bytes // torch.tensor([], dtype=dtype).element_size()
        arena = self._orig["empty"](numel + 2 * G, dtype=dtype, device=device)
        arena.view(torch.uint8).fill_(self.fill)
        out = arena[G:G + numel].view(shape)
        if value is not None:
            out.fill_(value)
        self.records.append(_Record(arena, G, tuple(shape), dtype, _site()))
        if requires_grad:
            out.requires_grad_(True)
        return out

    def _pass(self, name, t, kw):
        """An allocation handed to the original.  One that lands on the watched device anyway (a form of the call this patch does not
        read, a memory format it leaves alone) is written down: sweep() refuses a case whose buffers slipped past the guards."""
        if isinstance(t, torch.Tensor) and t.device.type == self.device_type and t.numel() > 0 and kw.get("out") is None:
            self.passed.append((_site(), tuple(t.shape), t.dtype, name))
        return t

    def _wanted(self, shape, dtype, device, kw, allowed):
        """True if this allocation is ours: on device_type, strided, not pinned, no out=, numel > 0, contiguous, no exotic keyword."""
        if shape is None or any(k not in allowed for k in kw):
            return False
        if kw.get("out") is not None or kw.get("pin_memory"):
            return False
        if kw.get("layout", torch.strided) not in (None, torch.strided):
            return False
        if device.type != self.device_type or dtype.is_complex or any(s <= 0 for s in shape):
            return False
        return True

    @staticmethod
    def _device(d):
        if d is None:
            return _default_device()
        return torch.device("cuda", d) if isinstance(d, int) else torch.device(d)

    def _make_plain(self, name, value):
        orig = self._orig[name]
        allowed = {"dtype", "device", "layout", "pin_memory", "requires_grad", "memory_format", "out"}

        def patched(*args, **kw):
            given = dict(kw)
            if not args and "size" in kw:
                kw = dict(kw)
                args = (kw.pop("size"),)
            shape = _size_of(args)
            dtype = kw.get("dtype") or torch.get_default_dtype()
            if kw.get("memory_format", torch.contiguous_format) not in (None, torch.contiguous_format):
                return self._pass(name, orig(*args, **kw), given)
            if not self._wanted(shape, dtype, self._device(kw.get("device")), kw, allowed):
                return self._pass(name, orig(*args, **kw), given)
            return self._carve(shape, dtype, self._device(kw.get("device")), value, bool(kw.get("requires_grad")))
        patched.__name__ = name
        return patched

    def _make_full(self):
        orig = self._orig["full"]
        allowed = {"dtype", "device", "layout", "pin_memory", "requires_grad", "out"}

        def patched(size, fill_value, **kw):
            shape = _size_of((size,)) if isinstance(size, (tuple, list, torch.Size)) else None
            dtype = kw.get("dtype")
            if dtype is None:
                dtype = fill_value.dtype if isinstance(fill_value, torch.Tensor) else torch.tensor(fill_value).dtype
            if not self._wanted(shape, dtype, self._device(kw.get("device")), kw, allowed):
                return self._pass("full", orig(size, fill_value, **kw), kw)
            return self._carve(shape, dtype, self._device(kw.get("device")), fill_value, bool(kw.get("requires_grad")))
        patched.__name__ = "full"
        return patched

    def _make_like(self, name, value):
        orig = self._orig[name]
        allowed = {"dtype", "device", "layout", "pin_memory", "requires_grad", "memory_format"}

        def patched(inp, **kw):
            mf = kw.get("memory_format", torch.preserve_format)
            keeps = mf == torch.contiguous_format or (mf in (None, torch.preserve_format) and inp.is_contiguous())
            if not keeps or inp.layout != torch.strided or kw.get("layout", torch.strided) not in (None, torch.strided):
                return self._pass(name, orig(inp, **kw), kw)
            dtype = kw.get("dtype") or inp.dtype
            device = self._device(kw["device"]) if kw.get("device") is not None else inp.device
            shape = tuple(inp.shape)
            if not self._wanted(shape, dtype, device, kw, allowed):
                return self._pass(name, orig(inp, **kw), kw)
            return self._carve(shape, dtype, device, value, bool(kw.get("requires_grad")))
        patched.__name__ = name
        return patched

    # ---- the check -------------------------------------------------------------------------------------------------------------
    def check(self):
        """Synchronise, then require both guard bands of every recorded allocation to hold `fill`, byte for byte."""
        if self.device_type == "cuda" and torch.cuda.is_available():
            torch.cuda.synchronize()
        if not self.records:
            return 0
        gb = self.guard_bytes
        bands = []
        for r in self.records:
            raw = r.arena.view(torch.uint8)
            bands += [raw[:gb], raw[raw.numel() - gb:]]
        if not bool((torch.cat(bands) != self.fill).any()):        # one reduction for the clean run; the walk below only names a failure
            return len(self.records)
        msgs = []
        for r in self.records:
            raw = r.arena.view(torch.uint8)
            for side, band in (("before", raw[:gb]), ("after", raw[raw.numel() - gb:])):
                dirty = (band != self.fill).nonzero().flatten()
                if dirty.numel():
                    lo, hi = int(dirty[0]), int(dirty[-1])
                    span = "%+d..%+d" % ((lo - gb, hi - gb) if side == "before" else (lo, hi))
                    msgs.append("%s: shape %s %s: guard band %s, %s bytes from the tensor's edge dirty (%d of %d bytes, fill 0x%02X)"
                                % (r.site, tuple(r.shape), str(r.dtype).replace("torch.", ""), side, span, dirty.numel(), gb, self.fill))
        raise GuardError("a kernel wrote outside what it owns:\n  " + "\n  ".join(msgs))


# ---- running a case ------------------------------------------------------------------------------------------------------------------
_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16, torch.bfloat16: torch.int16,
             torch.bool: torch.uint8}


def bits(t):
    """An integer view of t, so that NaNs and signed zeros compare by their bits."""
    t = t.detach().contiguous()
    return t.view(_INT_VIEW[t.dtype]) if t.dtype in _INT_VIEW else t


def flatten(result, prefix="out"):
    """Every tensor of a nested result (tuples, lists, dicts; None and python scalars skipped) as (label, tensor)."""
    if result is None or isinstance(result, (int, float, bool, str)):
        return []
    if isinstance(result, torch.Tensor):
        return [(prefix, result)]
    if isinstance(result, dict):
        return [kv for k in result for kv in flatten(result[k], "%s[%r]" % (prefix, k))]
    if isinstance(result, (tuple, list)):
        return [kv for i, v in enumerate(result) for kv in flatten(v, "%s[%d]" % (prefix, i))]
    raise TypeError("a case returned a %s" % type(result).__name__)


def assert_same_bits(got, want, what, mask=None, canon=None):
    g, w = flatten(got), flatten(want)
    assert [k for k, _ in g] == [k for k, _ in w], "%s: the runs returned differently shaped results" % what
    for i, ((k, a), (_, b)) in enumerate(zip(g, w)):
        assert a.shape == b.shape and a.dtype == b.dtype, "%s: %s is %s %s, was %s %s" % (what, k, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
        if canon is not None:
            a, b = canon(i, a), canon(i, b)
        a, b = bits(a), bits(b)
        if mask is not None:
            keep = mask(i, a, [t for _, t in g])
            if keep is not None:
                a, b = torch.where(keep, a, torch.zeros((), dtype=a.dtype, device=a.device)), torch.where(keep, b, torch.zeros((), dtype=b.dtype, device=b.device))
        if not torch.equal(a, b):
            bad = (a != b).flatten().nonzero().flatten()
            raise AssertionError("%s: %s differs in %d of %d elements, first at flat index %d (%s vs %s): the op read memory it did not write"
                                 % (what, k, bad.numel(), a.numel(), int(bad[0]), a.flatten()[bad[0]].item(), b.flatten()[bad[0]].item()))


class Case:
    """One row of the table: `fn()` builds nothing (inputs are built outside, once) and returns everything the op produced.
    atomic: 'file:line' of the float atomicAdd that makes the bits order-dependent -- then `verify(result)` (the float64 comparison of
    the op's own value test, at that test's tolerance) replaces the bit comparison.  mask(i, tensor, outputs) -> bool tensor of the elements of
    output i that are specified (outputs: all tensors of that run, for a region another output delimits), or None; canon(i, tensor) -> output i in the canonical form of what the header specifies (an order it
    leaves open, sorted); header: the include/gspn_hip.h line that documents the unwritten or unspecified part -- required with either."""

    def __init__(self, name, fn, atomic=None, verify=None, mask=None, canon=None, header=None, note=None):
        assert (atomic is None) == (verify is None) and (mask is None and canon is None) == (header is None)
        self.name, self.fn, self.atomic, self.verify, self.mask, self.canon, self.header, self.note = name, fn, atomic, verify, mask, canon, header, note

    @property
    def masked(self):
        return self.mask is not None or self.canon is not None

    def __repr__(self):
        return self.name


def sweep(case, device_type="cuda", guard_bytes=256):
    """Run a case unpatched, then under 0x00, 0xFF, 0x7F.  A: guards intact.  B: bits equal across all four runs (or, for a float-atomic
    exception, every run within the value test's tolerance and NaN-free).  C: only the documented mask is applied."""
    plain = case.fn()
    if device_type == "cuda":
        torch.cuda.synchronize()
    assert flatten(plain), "%s returned no tensor" % case.name
    runs = [("unpatched", plain)]
    for fill in FILLS:
        with Arena(fill, device_type, guard_bytes) as a:
            got = case.fn()
            n = a.check()
        assert n > 0, "%s allocated nothing through the patched functions: the case does not test what it claims" % case.name
        assert not a.passed, "%s: device allocations went past the guards (a call form the patch does not read):\n  %s" % (
            case.name, "\n  ".join("%s: torch.%s -> %s %s" % (site, fn, shape, dtype) for site, shape, dtype, fn in a.passed))
        runs.append(("fill 0x%02X" % fill, got))
    for label, got in runs:
        if case.atomic is not None:
            for k, t in flatten(got):
                if t.is_floating_point():
                    assert not bool(torch.isnan(t).any()), "%s, %s: NaN in %s" % (case.name, label, k)
            case.verify(got)
        elif label != "unpatched":
            assert_same_bits(got, plain, "%s, %s vs unpatched" % (case.name, label), case.mask, case.canon)
    return runs
