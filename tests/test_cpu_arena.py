"""tests/arena.py tested on itself, on the CPU, with toy functions written in torch: a harness that cannot fail proves nothing, so every
detection it promises is asserted here on a function that is wrong in exactly that way."""
import pytest
import torch

from tests import arena
from tests.arena import Arena, Case, GuardError, bits, sweep

DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool)


def _store_at(out, elem_offset):
    """Write one element `elem_offset` elements from out's first element, through as_strided on the returned tensor."""
    flat = out.as_strided((1,), (1,), out.storage_offset() + elem_offset)
    flat.view(torch.uint8).fill_(0x5A)             # a byte that is none of the fills


# ---- overruns ------------------------------------------------------------------------------------------------------------------------
def test_one_element_past_the_end_is_named():
    with Arena(0x00, "cpu") as a:
        out = torch.empty(5, 7)
        out.fill_(1.0)
        _store_at(out, out.numel())
        with pytest.raises(GuardError) as e:
            a.check()
    msg = str(e.value)
    assert "after, +0..+3" in msg and "test_cpu_arena.py:" in msg and "(5, 7)" in msg and "float32" in msg and "before" not in msg


def test_one_element_before_the_start_is_named():
    with Arena(0xFF, "cpu") as a:
        out = torch.empty(5, 7, dtype=torch.int32)
        _store_at(out, -1)
        with pytest.raises(GuardError) as e:
            a.check()
    msg = str(e.value)
    assert "before, -4..-1" in msg and "int32" in msg and "after" not in msg


@pytest.mark.parametrize("fill", arena.FILLS)
def test_the_far_edge_of_each_band_is_watched(fill):
    gb = 256
    for off, want in ((gb - 1, "after, +255..+255"), (-gb, "before, -256..-256")):
        with Arena(fill, "cpu", gb) as a:
            out = torch.empty(33, dtype=torch.uint8)
            _store_at(out, out.numel() + off if off > 0 else off)
            with pytest.raises(GuardError) as e:
                a.check()
        assert want in str(e.value)
    with Arena(fill, "cpu", gb) as a:           # and a function that stays inside passes
        out = torch.empty(33, dtype=torch.uint8)
        out.fill_(9)
        assert a.check() == 1


def test_the_site_is_the_allocating_line():
    def allocate():
        return torch.empty(3)                   # <- this line
    with Arena(0x7F, "cpu") as a:
        allocate()
    line = allocate.__code__.co_firstlineno + 1
    assert a.records[0].site.endswith("test_cpu_arena.py:%d" % line)


# ---- stale reads ---------------------------------------------------------------------------------------------------------------------
def _accumulates(x):
    out = torch.empty_like(x)
    out += x                                    # wrong: reads what it never wrote
    return out


def _overwrites(x):
    out = torch.empty_like(x)
    torch.mul(x, 2.0, out=out)
    return out


def test_accumulating_into_empty_changes_with_the_fill():
    x = torch.arange(12, dtype=torch.float32).view(3, 4)
    got = {}
    for fill in arena.FILLS:
        with Arena(fill, "cpu") as a:
            got[fill] = _accumulates(x)
            a.check()                           # it stays inside: only B can see this one
    assert torch.equal(bits(got[0x00]), bits(x))
    assert not torch.equal(bits(got[0x00]), bits(got[0xFF])) and bool(torch.isnan(got[0xFF]).all())
    assert not torch.equal(bits(got[0x00]), bits(got[0x7F]))
    with pytest.raises(AssertionError, match="read memory it did not write"):
        sweep(Case("accumulates", lambda: _accumulates(x)), "cpu")


def test_a_correct_function_passes_the_sweep():
    x = torch.arange(12, dtype=torch.float32).view(3, 4)
    runs = sweep(Case("overwrites", lambda: (_overwrites(x), None, {"k": _overwrites(x)})), "cpu")
    assert [label for label, _ in runs] == ["unpatched", "fill 0x00", "fill 0xFF", "fill 0x7F"]
    for _, got in runs:
        assert torch.equal(got[0], 2 * x)


def test_the_sweep_sees_an_overrun_and_an_untested_case():
    def overruns():
        out = torch.zeros(4)
        if out.storage_offset():                # the unpatched run has no room behind its tensor; under the arena the store lands in the band
            _store_at(out, 4)
        return out
    with pytest.raises(GuardError, match=r"after, \+0"):
        sweep(Case("overruns", overruns), "cpu")
    with pytest.raises(AssertionError, match="allocated nothing"):
        sweep(Case("allocates nothing", lambda: torch.arange(3) + 1), "cpu")


def test_a_mask_hides_only_what_it_names():
    def half_written():
        out = torch.empty(2, 6)
        out[:, :3] = 1.0
        return out
    keep = lambda i, t, outs: (torch.arange(6) < outs[0].shape[1] // 2).expand(2, 6)      # noqa: E731
    sweep(Case("half", half_written, mask=keep, header="include/gspn_hip.h:0 (toy)"), "cpu")
    with pytest.raises(AssertionError, match="read memory"):
        sweep(Case("half", half_written), "cpu")


def test_nan_bits_compare():
    a = torch.tensor([float("nan"), -0.0])
    assert torch.equal(bits(a), bits(a.clone())) and not torch.equal(bits(a), bits(torch.tensor([float("nan"), 0.0])))


# ---- zeros / full --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", arena.FILLS)
def test_zeros_and_full_inside_fill_in_the_bands(fill):
    x = torch.ones(2, 3, dtype=torch.int32)
    with Arena(fill, "cpu") as a:
        z = torch.zeros(4, 5)
        zl = torch.zeros_like(x)
        f = torch.full((3, 2), 7, dtype=torch.int64)
        ff = torch.full((2,), 1.5)
        fb = torch.full((2,), True)
        e = torch.empty(6, dtype=torch.uint8)
        assert a.check() == 6
    assert bool((z == 0).all()) and z.dtype == torch.float32 and bool((zl == 0).all()) and zl.dtype == torch.int32 and zl.shape == (2, 3)
    assert bool((f == 7).all()) and bool((ff == 1.5).all()) and ff.dtype == torch.float32 and fb.dtype == torch.bool and bool(fb.all())
    assert bool((e == fill).all())                          # the payload of empty is poisoned too
    for r in a.records:
        raw = r.arena.view(torch.uint8)
        assert raw.numel() == 2 * 256 + torch.Size(r.shape).numel() * r.arena.element_size()
        assert bool((raw[:256] == fill).all()) and bool((raw[-256:] == fill).all())
        assert r.G * r.arena.element_size() == 256


# ---- pass-through --------------------------------------------------------------------------------------------------------------------
def test_what_is_not_ours_passes_through_unrecorded():
    x = torch.ones(2, 3, 4, 5)
    with Arena(0xFF, "cuda") as a:                          # watching CUDA: CPU allocations are not ours
        c = torch.empty(8)
        cz = torch.zeros(8, dtype=torch.int32)
        cl = torch.empty_like(x)
        cf = torch.full((3,), 2.0)
        assert not a.records and bool((cz == 0).all()) and bool((cf == 2).all()) and c.shape == (8,) and cl.shape == x.shape
        assert not a.passed                                 # another device's allocations are nobody's business
    with Arena(0xFF, "cpu") as a:
        buf = torch.ones(8)
        o = torch.zeros(8, out=buf)
        assert o.data_ptr() == buf.data_ptr() and bool((buf == 0).all())
        torch.full((8,), 3.0, out=buf)
        assert bool((buf == 3).all())
        n = torch.empty(0, 3)                               # numel == 0
        cl = torch.empty_like(x, memory_format=torch.channels_last)
        assert cl.is_contiguous(memory_format=torch.channels_last)
        t = torch.empty_like(x.transpose(1, 2))             # preserve_format of a non-contiguous input keeps its strides
        assert t.stride() == x.transpose(1, 2).stride() and n.numel() == 0
        assert not a.records
        # what landed on the watched device without a guard is written down (out= and empty tensors are not allocations of ours)
        assert [(shape, fn) for _, shape, _, fn in a.passed] == [((2, 3, 4, 5), "empty_like"), ((2, 4, 3, 5), "empty_like")]
        assert all(site.startswith("tests/test_cpu_arena.py:") for site, _, _, _ in a.passed)
        if torch.cuda.is_available():
            p = torch.empty(1, dtype=torch.int32, pin_memory=True)
            assert p.is_pinned() and not a.records
        else:
            seen, real = {}, a._orig["empty"]               # no accelerator to pin for: the request must reach the original as it came

            def spy(*size, **kw):
                seen.update(kw)
                return real(*size, dtype=kw["dtype"])
            a._orig["empty"] = spy
            torch.empty = a._make_plain("empty", None)
            torch.empty(1, dtype=torch.int32, pin_memory=True)
            a._orig["empty"] = real
            assert seen == {"dtype": torch.int32, "pin_memory": True} and not a.records


# ---- what a patched call returns -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_shape_dtype_contiguity_alignment(dtype):
    like = torch.ones(3, 1, 5).to(dtype)
    with Arena(0xFF, "cpu") as a:
        outs = [torch.empty(3, 5, 7, dtype=dtype), torch.empty((3, 5, 7), dtype=dtype), torch.empty(torch.Size((3, 5, 7)), dtype=dtype),
                torch.zeros(3, 5, 7, dtype=dtype), torch.full((3, 5, 7), 1, dtype=dtype), torch.empty((), dtype=dtype), torch.empty(1, dtype=dtype),
                torch.empty_like(like), torch.zeros_like(like), torch.empty_like(torch.ones(2), dtype=dtype)]
        assert a.check() == len(outs)
    for o, shape in zip(outs, [(3, 5, 7)] * 5 + [(), (1,), (3, 1, 5), (3, 1, 5), (2,)]):
        assert tuple(o.shape) == shape and o.dtype == dtype and o.is_contiguous() and o.data_ptr() % 16 == 0 and o.device.type == "cpu"
    assert all(r.arena.data_ptr() % 16 == 0 for r in a.records)


def test_every_spelling_of_a_size_is_read():
    import numpy as np
    with Arena(0xFF, "cpu") as a:
        outs = [torch.empty(np.int64(3), np.int32(5)), torch.empty((np.int64(3), 5)), torch.empty(size=(3, 5)), torch.zeros(size=[3, 5]),
                torch.empty(torch.tensor(3), 5), torch.full(size=(3, 5), fill_value=2.0), torch.empty([3, 5], dtype=torch.float32, device="cpu")]
        assert a.check() == len(outs) and not a.passed
    assert all(tuple(o.shape) == (3, 5) for o in outs) and bool((outs[3] == 0).all()) and bool((outs[5] == 2).all())


def test_the_sweep_refuses_a_case_whose_buffer_slipped_past():
    def slips():
        out = torch.empty(4)
        side = torch.empty((1, 2, 2, 2), memory_format=torch.channels_last)      # a form the patch leaves to the original
        side.zero_()
        return out.fill_(1.0) + side.sum()
    with pytest.raises(AssertionError, match=r"went past the guards(.|\n)*test_cpu_arena.py:\d+: torch.empty -> \(1, 2, 2, 2\)"):
        sweep(Case("slips", slips), "cpu")


def test_requires_grad_is_applied_afterwards():
    with Arena(0x00, "cpu") as a:
        z = torch.zeros(3, requires_grad=True)
        e = torch.empty(3)
        a.check()
    assert z.requires_grad and z.is_leaf and not e.requires_grad
    (z * 2).sum().backward()
    assert torch.equal(z.grad, torch.full((3,), 2.0))


# ---- patching and its limits ---------------------------------------------------------------------------------------------------------
def test_the_originals_come_back():
    orig = {n: getattr(torch, n) for n in arena._PATCHED}
    with Arena(0x00, "cpu"):
        assert all(getattr(torch, n) is not orig[n] for n in orig)
    assert all(getattr(torch, n) is orig[n] for n in orig)
    with pytest.raises(ZeroDivisionError):
        with Arena(0xFF, "cpu"):
            torch.empty(3)
            1 / 0
    assert all(getattr(torch, n) is orig[n] for n in orig) and arena._open is None


def test_nesting_raises():
    orig = torch.empty
    with Arena(0x00, "cpu"):
        with pytest.raises(RuntimeError, match="nesting"):
            with Arena(0xFF, "cpu"):
                pass
        assert torch.empty is not orig          # the failed inner open left the outer one in place
    assert torch.empty is orig
    with Arena(0x00, "cpu"):                    # and a new one opens afterwards
        pass


def test_the_fill_order():
    assert arena.FILLS == (0x00, 0xFF, 0x7F)
    with Arena(0xFF, "cpu"):
        assert torch.empty(2).isnan().all() and int(torch.empty(1, dtype=torch.int32)) == -1 and int(torch.empty(1, dtype=torch.int64)) == -1
        assert int(torch.empty(1, dtype=torch.uint8)) == 255
    with Arena(0x7F, "cpu"):
        assert 3.39e38 < float(torch.empty(1)) < 3.4e38 and int(torch.empty(1, dtype=torch.int32)) == 0x7F7F7F7F
