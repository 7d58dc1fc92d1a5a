"""CPU self-checks of the guarded arena (tests/guarded.py): the harness must be able to FAIL — every planted defect is reported
with the right buffer name and offsets — and the coverage of the ABI by the memory-contract table is complete."""
import os

import numpy as np
import pytest
import torch

import guarded
from guarded import Arena, GuardError, run_contract

f32, i32, i64 = torch.float32, torch.int32, torch.int64


def small_arena():
    ar = Arena("cpu")
    x = ar.inp("x", torch.arange(33 * 33, dtype=f32).view(33, 33) + 1.0)
    idx = ar.inp("idx", torch.arange(7, dtype=i32))
    y = ar.out("y", f32, (33, 33))
    return ar, x, idx, y


def wide_view(ar, b):
    """A view of the arena that reaches one element in front of and behind buffer b (what a kernel's raw pointer can touch)."""
    lo = b.start - b.itemsize
    return ar.mem[lo:b.end + b.itemsize].view(b.dtype)


def good(ar):
    ar["y"].t.copy_(ar["x"].t * 2.0)
    return 0


def only(failures, **kw):
    hits = [f for f in failures if all(f.get(k) == v for k, v in kw.items())]
    assert len(hits) == 1, (kw, failures)
    return hits[0]


def test_a_correct_call_passes_and_returns_the_outputs():
    ar, x, idx, y = small_arena()
    outs, reproducible = run_contract(good, ar)
    assert reproducible
    assert torch.equal(outs["y"], x.data.view(33, 33) * 2.0)
    assert set(outs) == {"y"}


def test_write_one_element_in_front_of_a_buffer_is_reported():
    ar, x, idx, y = small_arena()
    ar.build("A")
    good(ar)
    wide_view(ar, y)[0] = 5.0
    with pytest.raises(GuardError) as e:
        ar.check()
    f = only(e.value.failures, buffer="y", side="leading")
    assert (f["first"], f["last"]) == (-4, -1) and 1 <= f["count"] <= 4
    assert len(e.value.failures) == 1 and "y" in str(e.value) and "leading" in str(e.value)


def test_write_one_element_behind_a_buffer_is_reported():
    ar, x, idx, y = small_arena()
    ar.build("B")
    good(ar)
    wide_view(ar, y)[-1] = 5.0
    with pytest.raises(GuardError) as e:
        ar.check()
    f = only(e.value.failures, buffer="y", side="trailing")
    assert f["first"] == 0 and f["last"] <= 3 and 1 <= f["count"] <= 4          # end + 0: the first byte behind the buffer
    assert len(e.value.failures) == 1


def test_write_into_an_input_is_reported():
    ar, x, idx, y = small_arena()
    ar.build("A")
    good(ar)
    x.t[2, 3] = -1.0
    idx.t[6] = 3
    with pytest.raises(GuardError) as e:
        ar.check()
    f = only(e.value.failures, buffer="x", kind="modified input")
    assert f["first"] // 4 == 2 * 33 + 3 and f["last"] // 4 == 2 * 33 + 3
    f = only(e.value.failures, buffer="idx", kind="modified input")
    assert f["first"] // 4 == 6
    assert len(e.value.failures) == 2


def test_output_that_keeps_its_prefill_is_reported():
    def leaves_one(ar):
        good(ar)
        ar["y"].t.view(-1)[40] = float("nan") if ar.fill == "A" else 0.0        # = not written: the pre-fill shows through
        return 0
    ar, x, idx, y = small_arena()
    with pytest.raises(GuardError) as e:
        run_contract(leaves_one, ar)
    f = only(e.value.failures, buffer="y", kind="fill-dependent output (A != B)")
    assert (f["first"], f["last"], f["count"]) == (40, 40, 1)
    assert any(g["kind"].startswith("NaN/Inf (run A") and g["first"] == 40 for g in e.value.failures)


def test_output_that_reads_a_guard_is_reported():
    def reads_past_the_end(ar):
        good(ar)
        ar["y"].t.view(-1)[0] = wide_view(ar, ar["x"])[-1]                      # one element behind the input
        return 0
    ar, x, idx, y = small_arena()
    with pytest.raises(GuardError) as e:
        run_contract(reads_past_the_end, ar)
    f = only(e.value.failures, buffer="y", kind="fill-dependent output (A != B)")
    assert (f["first"], f["count"]) == (0, 1)


def test_bad_return_code_is_reported():
    ar, x, idx, y = small_arena()
    with pytest.raises(AssertionError, match="return code -1"):
        run_contract(lambda a: good(a) - 1, ar)


def test_irreproducible_output_is_compared_with_a_tolerance_only_where_declared():
    state = {"n": 0}

    def noisy(ar):
        good(ar)
        state["n"] += 1
        ar["y"].t.view(-1)[5] += 1e-4 * state["n"]               # an atomically accumulated sum: another rounding every run
        return 0
    ar, x, idx, y = small_arena()
    with pytest.raises(GuardError) as e:                        # undeclared: compared to the bit
        run_contract(noisy, ar)
    f = only(e.value.failures, buffer="y", kind="fill-dependent output (A != B)")
    assert (f["first"], f["count"]) == (5, 1)
    outs, reproducible = run_contract(noisy, ar, tol=1e-3, tol_buffers={"y"})
    assert not reproducible
    with pytest.raises(GuardError):                             # ... and the tolerance is a bound, not a waiver
        run_contract(noisy, ar, tol=1e-9, tol_buffers={"y"})
    with pytest.raises(AssertionError, match="names no output"):
        run_contract(noisy, ar, tol=1e-3, tol_buffers={"x"})


def test_compare_limits_the_defined_elements_and_canon_orders_them():
    def pads(ar):
        t = ar["y"].t.view(-1)
        t[:6] = ar["x"].t.view(-1)[:6].flip(0) if ar.fill == "B" else ar["x"].t.view(-1)[:6]     # defined, in an undefined order
        return 0                                                 # elements 6.. keep their pre-fill: padding
    ar = Arena("cpu")
    ar.inp("x", torch.arange(8, dtype=f32))
    ar.out("y", f32, (8,), compare=6)
    with pytest.raises(GuardError):
        run_contract(pads, ar)

    def canon(outs):
        outs["y"] = torch.cat((outs["y"][:6].sort().values, outs["y"][6:]))
        return outs
    outs, reproducible = run_contract(pads, ar, canon=canon)
    assert reproducible and torch.equal(outs["y"][:6], torch.arange(6, dtype=f32))


def test_layout_alignment_and_trailing_guard_at_end_plus_zero():
    ar, x, idx, y = small_arena()
    ar.build("A")
    assert x.nbytes == 33 * 33 * 4 and x.nbytes % 256 != 0
    for b in ar.buffers:
        assert b.ptr % 256 == 0 and b.start % 256 == 0
    reg = {(b.name, side): (lo, hi) for b, side, lo, hi in ar.regions()}
    for b in ar.buffers:
        lo, hi = reg[(b.name, "trailing")]
        assert lo == b.end and hi - lo == guarded.GUARD                         # alignment slack belongs to the guard
        lo, hi = reg[(b.name, "leading")]
        assert hi == b.start and hi - lo >= guarded.GUARD
    # the bands tile everything that is not a buffer
    covered = np.zeros(ar.mem.numel(), np.int32)
    for _b, _s, lo, hi in ar.regions():
        covered[lo:hi] += 1
    for b in ar.buffers:
        covered[b.start:b.end] += 1
    assert (covered == 1).all()
    assert guarded.GUARD >= 192 * 128 * 4 and guarded.GUARD >= 64 * 128 * 4
    # the first byte behind the float buffer holds guard fill, not alignment padding
    assert int(ar.mem[x.end]) == 0xFF and int(ar.mem[x.end + 255]) == 0xFF


@pytest.mark.parametrize("fill", ["A", "B"])
def test_guard_fills_follow_the_neighbour_dtype(fill):
    ar = Arena("cpu")
    a = ar.inp("a32", torch.arange(5, dtype=i32))
    b = ar.inp("a64", torch.arange(3, dtype=i64))
    c = ar.out("f", f32, (9,))
    h = ar.out("h", torch.bfloat16, (7,))
    ar.build(fill)
    reg = {(x.name, side): ar.mem[lo:hi] for x, side, lo, hi in ar.regions()}
    for nm, dt in (("a32", i32), ("a64", i64)):
        for side in ("leading", "trailing"):
            g = reg[(nm, side)]
            assert int(g.max()) <= 1                                            # int-neighbour guards hold 0 or 1 only
            lo = [lo_ for x, s, lo_, _ in ar.regions() if x.name == nm and s == side][0]
            w = 8 if dt == i64 else 4
            k0 = (-lo) % w
            words = g[k0:k0 + (g.numel() - k0) // w * w].view(dt)
            assert bool((words == (0 if fill == "A" else 1)).all())
    for nm in ("f", "h"):
        for side in ("leading", "trailing"):
            g = reg[(nm, side)]
            lo = [lo_ for x, s, lo_, _ in ar.regions() if x.name == nm and s == side][0]
            k0 = (-lo) % 4
            words = g[k0:k0 + (g.numel() - k0) // 4 * 4].view(f32)
            if fill == "A":
                assert bool((g == 0xFF).all()) and bool(torch.isnan(words).all())
            else:
                assert bool((words == 1e30).all())
    # pre-fills of `out` buffers
    assert bool((ar.mem[c.start:c.end] == (0xFF if fill == "A" else 0)).all())
    assert torch.equal(a.t, torch.arange(5, dtype=i32))


# ---- coverage of the ABI ------------------------------------------------------------------------------------------------
def _device_pointer_symbols():
    import ctypes as C
    from na_mpnn_amd import hip
    host_ptr = (C.POINTER(C.c_float), C.POINTER(C.c_int32))                     # host arrays; device pointers cross as void* / structs of them
    out = []
    for name, (_res, args) in hip._PROTOTYPES.items():
        if any(a is C.c_void_p or (hasattr(a, "_type_") and not isinstance(a._type_, str) and a not in host_ptr) for a in args):
            out.append(name)
    return out


def test_every_entry_point_with_a_device_pointer_is_in_the_contract_table_or_exempt():
    from na_mpnn_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libnamp_hip.so is not built (python -m na_mpnn_amd.build): the coverage check compares against its prototypes")
    import test_gpu_memory_contract as mc
    L = hip.lib()
    table, exempt = set(mc.TABLE), set(mc.EXEMPT)
    for name in table | exempt:
        assert hasattr(L, name), f"{name} is not an exported symbol"
    assert not (table & exempt), sorted(table & exempt)
    for name, reason in mc.EXEMPT.items():
        assert isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name
    assert not (set(mc.REQUIRED) & exempt), sorted(set(mc.REQUIRED) & exempt)
    assert not (set(mc.REQUIRED) - table), sorted(set(mc.REQUIRED) - table)
    missing = [s for s in _device_pointer_symbols() if s not in table and s not in exempt]
    assert not missing, f"decide where these belong (contract table or EXEMPT): {missing}"
