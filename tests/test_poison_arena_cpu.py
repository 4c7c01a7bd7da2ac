"""The poisoned arena of tests/poison_arena.py on the CPU: the detector detects (a byte written into a guard, a flipped input
bit and an output element left poisoned are each reported with the operand's name and offset), and the accounting of
tests/test_poisoned_arena_gpu.py leaves no kernel-launching entry of include/nsdp_hip.h out."""
import fnmatch

import pytest
import torch

from poison_arena import GUARD, ArenaError, PoisonArena


def _arena():
    a = PoisonArena("cpu", capacity=4 << 20)
    x = a.input("x", torch.arange(12, dtype=torch.float32).reshape(3, 4))
    idx = a.input("idx", torch.tensor([2, 0, 1], dtype=torch.int32))
    y = a.output("y", (5, 4), rows=3)
    ws = a.workspace("ws", 64)
    return a, x, idx, y, ws


def test_clean_call_passes_and_layout_is_as_declared():
    a, x, idx, y, ws = _arena()
    assert torch.isnan(y).all() and torch.isnan(ws).all()                # poison is NaN as fp32 ...
    assert torch.isnan(a.buf[:4].view(torch.bfloat16)).all()               # ... and as bf16
    assert all(r.start % 256 == 0 for r in a.regions)
    starts = sorted((r.start, r.end) for r in a.regions)
    assert starts[0][0] >= GUARD and a.capacity - starts[-1][1] >= GUARD
    assert all(s1 - e0 >= 2 * GUARD - 256 for (_, e0), (s1, _) in zip(starts, starts[1:]))
    r = next(r for r in a.regions if r.name == "idx")
    assert int(a.buf[r.start - GUARD:r.start].max()) == 0 and int(a.buf[r.end:r.end + GUARD].max()) == 0     # a valid index
    y[:3] = x[idx.long()]
    ws[:4] = 1.0
    a.check(written=[y[:3]])
    assert torch.isnan(y[3:]).all()


def test_guard_write_is_reported_with_name_and_offset():
    a, x, idx, y, ws = _arena()
    y[:3] = 0.0
    r = next(r for r in a.regions if r.name == "y")
    a.buf[r.end + 7] = 0x01                                              # one byte, 7 bytes past the end of y
    found = a.problems(written=[y[:3]])
    assert any("guard behind 'y'" in p and "7 bytes past its end" in p for p in found), found
    a.buf[r.end + 7] = 0xFF
    a.buf[r.start - 1] = 0x00
    found = a.problems(written=[y[:3]])
    assert any("guard before 'y'" in p and "1 bytes before" in p for p in found), found
    with pytest.raises(ArenaError):
        a.check(written=[y[:3]])


def test_flipped_input_bit_is_reported_with_name_and_offset():
    a, x, idx, y, ws = _arena()
    y[:3] = 0.0
    r = next(r for r in a.regions if r.name == "x")
    a.buf[r.start + 21] ^= 0x10
    found = a.problems(written=[y[:3]])
    assert any("input 'x' at byte offset 21" in p for p in found), found


def test_unwritten_output_element_is_reported_with_name_and_offset():
    a, x, idx, y, ws = _arena()
    y[:3] = 0.0
    r = next(r for r in a.regions if r.name == "y")
    a.buf[r.start + 24:r.start + 28] = 0xFF                              # y[1, 2] as the call found it
    found = a.problems(written=[y[:3]])
    assert any("never written: 'y' element 6 (byte offset 24)" in p for p in found), found


def test_rows_left_alone_by_contract_and_unowned_bytes_are_reported():
    a, x, idx, y, ws = _arena()
    y[:3] = 0.0
    y[4, 0] = 1.0                                                        # a row beyond `rows`
    a.buf[a.capacity - 5] = 0                                            # behind the last operand's guard
    found = a.problems(written=[y[:3]])
    assert any("rows left alone by contract of 'y' at byte offset 64" in p for p in found), found
    assert any(f"arena byte {a.capacity - 5} that belongs to no operand" in p for p in found), found


def test_routing_sends_a_module_s_allocations_into_the_arena():
    import types
    mod = types.SimpleNamespace(torch=torch)
    a = PoisonArena("cpu", capacity=4 << 20)
    from poison_arena import _TorchProxy
    mod.torch = _TorchProxy(a)
    e = mod.torch.empty((3, 4), dtype=torch.float32, device="cpu")
    z = mod.torch.zeros(5, dtype=torch.int32, device=torch.device("cpu"))
    l = mod.torch.empty_like(e)
    assert all(a._region_of(t)[0] is not None for t in (e, z, l)) and torch.isnan(e).all() and int(z.abs().sum()) == 0
    assert a._region_of(mod.torch.empty(3))[0] is None                   # no device given: not the wrappers' GPU allocations
    assert mod.torch.float32 is torch.float32
    with pytest.raises(ArenaError, match="requires_grad"):                # a keyword the arena cannot honour is not dropped
        mod.torch.empty(3, device="cpu", requires_grad=True)
    assert mod.torch.zeros(3, requires_grad=True).requires_grad          # (not routed: torch's own call, keywords and all)


def test_routed_swaps_torch_and_the_library_and_restores_both_after_an_exception(monkeypatch):
    """PoisonArena.routed() on a stand-in wrapper module and a stand-in library: inside the block the module allocates from the
    arena and every nsdp_* entry fetched from the library is recorded (other attributes are not); both are put back when the
    block ends with an exception."""
    import types
    from nsdp_amd import _lib
    fake = types.SimpleNamespace(nsdp_knn=lambda *a: 0, nsdp_last_error=lambda: b"", restype_of_something=7)
    monkeypatch.setattr(_lib, "_lib", fake)                               # what _lib.lib() hands out (no library is loaded)
    mods = [types.SimpleNamespace(torch=torch), types.SimpleNamespace(torch=torch)]
    a = PoisonArena("cpu", capacity=4 << 20)
    with pytest.raises(ZeroDivisionError):
        with a.routed(*mods) as inside:
            assert inside is a and all(m.torch is not torch for m in mods)
            t = mods[1].torch.empty(4, dtype=torch.float32, device="cpu")
            assert a._region_of(t)[0] is not None and torch.isnan(t).all()
            assert _lib.lib() is not fake
            assert _lib.lib().nsdp_knn is fake.nsdp_knn and _lib.lib().restype_of_something == 7
            with pytest.raises(AttributeError):
                _lib.lib().nsdp_no_such_entry
            1 / 0
    assert all(m.torch is torch for m in mods) and _lib._lib is fake
    assert a.called == {"nsdp_knn"}
    with a.routed(mods[0]):                                               # and after a clean exit
        _lib.lib().nsdp_last_error()
    assert mods[0].torch is torch and _lib._lib is fake and a.called == {"nsdp_knn", "nsdp_last_error"}


# ---------------------------------------------------------------------------------------------------------------------------------
# accounting: every entry of the header that launches a kernel is called inside the arena by tests/test_poisoned_arena_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------------
EXEMPT = ["nsdp_abi_version", "nsdp_last_error", "nsdp_debug_set", "nsdp_prof_*", "nsdp_trace_*", "nsdp_graph_exec_*",
          "*_supported", "*_ok", "*_bytes", "*_floats", "*_takes_mask", "*_chunk_elems"]


def test_every_kernel_launching_entry_is_called_inside_the_arena():
    import test_poisoned_arena_gpu as gpu_tests
    from nsdp_amd import _lib
    declared = set(_lib.declared_symbols())
    table = gpu_tests.COVERAGE
    unknown = sorted(set(table) - declared)
    assert not unknown, f"the table names entries the header does not declare: {unknown}"
    for entry, test in table.items():
        assert callable(getattr(gpu_tests, test, None)), f"{entry}: no test function {test}"
    left = sorted(n for n in declared - set(table) if not any(fnmatch.fnmatchcase(n, pat) for pat in EXEMPT))
    assert not left, f"kernel-launching entries no poisoned-arena test calls: {left}"
