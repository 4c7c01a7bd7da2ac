"""A poisoned arena for the kernels' operands: stray writes, reads of memory nobody wrote and output elements nobody wrote.

One allocation filled with 0xFF bytes (NaN as fp32 and as bf16, -1 as int32).  Every operand of a call is carved from it at a
256-byte-aligned offset with a guard band of GUARD bytes on both sides; float guards keep the poison, the guards of integer
operands hold 0 -- a valid index -- so that an over-read of an index tensor stays a wrong number and never becomes a wild
address.  A `shadow` copy records what every byte must still hold after the call and `writable` marks the bytes the call may
change (output and workspace interiors), so ``check()`` is one comparison over the whole arena:

  * a changed byte outside `writable` is a stray write: into a guard, into an input, into rows an output's contract leaves alone,
    or into arena bytes that belong to nothing;
  * an element of a "written whole" output that still holds the poison pattern was never written;
  * a read of memory nobody wrote shows up in the caller's comparison with its reference: the poison is NaN.

Operands are classified by the caller from the header text of include/nsdp_hip.h:
  input(...)      read only;
  output(...)     written whole (`rows`: only the first `rows` rows may be touched, the rest is left alone by contract);
  accum(...)      read and written (accumulate != 0, running statistics, counters): prefilled with the caller's finite values;
  workspace(...)  exactly the byte count of the size query, interior left poisoned.

``routed(modules...)`` sends the torch.empty / empty_like / zeros / zeros_like calls of the wrapper modules into the arena (so their
outputs and workspaces get guards too, without restating their ctypes calls) and puts a recording proxy in place of the loaded
library: `called` then names every nsdp_* entry the wrappers reached.  Works on a CPU arena too (tests/test_poison_arena_cpu.py).
"""
from __future__ import annotations

import contextlib

import torch

POISON = 0xFF
GUARD = 256 * 1024          # the footprint of the largest workgroup tile: 256 rows x 256 channels x 4 B
ALIGN = 256
_INT_DTYPES = (torch.int32, torch.int64, torch.int16, torch.int8)
_AS_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class ArenaError(AssertionError):
    pass


class _Region:
    def __init__(self, name, kind, start, nbytes, tensor):
        self.name, self.kind, self.start, self.nbytes, self.tensor = name, kind, start, nbytes, tensor

    @property
    def end(self):
        return self.start + self.nbytes


class PoisonArena:
    def __init__(self, device, capacity=64 << 20):
        self.device = torch.device(device)
        self.capacity = int(capacity)
        self.buf = torch.full((self.capacity,), POISON, dtype=torch.uint8, device=self.device)
        self.shadow = self.buf.clone()
        self.writable = torch.zeros(self.capacity, dtype=torch.bool, device=self.device)
        self.regions: list[_Region] = []
        self.cursor = 0
        self.called: set[str] = set()
        self._auto = 0

    # ------------------------------------------------------------------ carving
    def _carve(self, name, kind, shape, dtype, int_guard=None):
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = numel * item
        start = (self.cursor + GUARD + ALIGN - 1) // ALIGN * ALIGN
        end = start + nbytes
        if end + GUARD > self.capacity:
            raise ArenaError(f"arena of {self.capacity} bytes is too small for '{name}' ({nbytes} bytes at {start})")
        if int_guard if int_guard is not None else dtype in _INT_DTYPES:
            for lo, hi in ((start - GUARD, start), (end, end + GUARD)):      # a valid index, never -1
                self.buf[lo:hi] = 0
                self.shadow[lo:hi] = 0
        self.cursor = end + GUARD
        t = self.buf[start:end].view(dtype).view(shape)
        self.regions.append(_Region(name, kind, start, nbytes, t))
        return t, start, end

    def _fill(self, start, end, src):
        raw = src.detach().contiguous().reshape(-1).view(torch.uint8).to(self.device)
        self.buf[start:end] = raw
        self.shadow[start:end] = raw

    def input(self, name, t):
        """A read-only operand holding the values of `t` (any device); returns the arena tensor."""
        out, start, end = self._carve(name, "input", t.shape, t.dtype)
        self._fill(start, end, t)
        return out

    def output(self, name, shape, dtype=torch.float32, rows=None):
        """An operand the call writes whole (poisoned on entry).  `rows`: only the first `rows` of shape[0] rows may be touched."""
        out, start, end = self._carve(name, "output", shape, dtype)
        if rows is not None:
            end = start + (end - start) // max(int(shape[0]), 1) * int(rows)
        self.writable[start:end] = True
        return out

    def accum(self, name, t):
        """An operand the call reads and rewrites (accumulate != 0, running statistics, counters), prefilled with `t`."""
        out, start, end = self._carve(name, "accum", t.shape, t.dtype)
        self._fill(start, end, t)
        self.writable[start:end] = True
        return out

    def workspace(self, name, nbytes):
        """Scratch of exactly `nbytes` bytes (fp32 view), poisoned."""
        if nbytes % 4:
            raise ArenaError(f"workspace '{name}': {nbytes} bytes is no whole number of floats")
        out, start, end = self._carve(name, "workspace", (max(nbytes // 4, 0),), torch.float32)
        self.writable[start:end] = True
        return out

    def _routed_alloc(self, shape, dtype, zero):
        self._auto += 1
        out, start, end = self._carve(f"routed#{self._auto}{tuple(shape)}", "routed", shape, dtype)
        self.writable[start:end] = True
        if zero:
            out.zero_()
        return out

    # ------------------------------------------------------------------ routing
    @contextlib.contextmanager
    def routed(self, *modules):
        """Inside the block the modules' torch.empty / empty_like / zeros / zeros_like on the arena's device come from the arena,
        and every nsdp_* entry fetched from the library is noted in `called`."""
        from nsdp_amd import _lib
        proxy = _TorchProxy(self)
        saved = [(m, m.torch) for m in modules]
        real = _lib.lib()
        try:
            for m, _ in saved:
                m.torch = proxy
            _lib._lib = _Recorder(real, self.called)
            yield self
        finally:
            _lib._lib = real
            for m, t in saved:
                m.torch = t

    # ------------------------------------------------------------------ checking
    def _describe(self, off):
        for r in self.regions:
            if r.start - GUARD <= off < r.start:
                return f"guard before '{r.name}' ({r.kind}), {r.start - off} bytes before its first byte (arena offset {off})"
            if r.start <= off < r.end:
                what = "rows left alone by contract of" if r.kind == "output" else r.kind
                return f"{what} '{r.name}' at byte offset {off - r.start} (arena offset {off})"
            if r.end <= off < r.end + GUARD:
                return f"guard behind '{r.name}' ({r.kind}), {off - r.end} bytes past its end (arena offset {off})"
        return f"arena byte {off} that belongs to no operand"

    def _region_of(self, t):
        ptr = t.data_ptr()
        base = self.buf.data_ptr()
        for r in self.regions:
            if base + r.start <= ptr < base + max(r.end, r.start + 1):
                return r, ptr - base - r.start
        return None, 0

    def problems(self, written=()):
        """The list of violations (strings).  `written`: arena tensors (or views of them; the view's element size is the poison
        unit) that the call must have written whole."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        out = []
        bad = (self.buf != self.shadow) & ~self.writable
        n_bad = int(bad.sum())
        if n_bad:
            offs = bad.nonzero().reshape(-1)
            first = [int(o) for o in offs[:4]] + ([int(offs[-1])] if n_bad > 4 else [])
            for off in first:
                out.append(f"stray write: {self._describe(off)} holds 0x{int(self.buf[off]):02x}, expected 0x{int(self.shadow[off]):02x}")
            out.append(f"{n_bad} byte(s) changed outside the operands the call may write")
        for t in written:
            if t is None or t.numel() == 0:
                continue
            r, rel = self._region_of(t)
            if r is None:
                out.append(f"a tensor of shape {tuple(t.shape)} that should have been written does not live in the arena")
                continue
            bits = t.contiguous().reshape(-1).view(_AS_INT[t.element_size()])
            stale = bits == (POISON if t.element_size() == 1 else -1)
            n_stale = int(stale.sum())
            if n_stale:
                i = int(stale.nonzero()[0])
                out.append(f"never written: '{r.name}' element {i} (byte offset {rel + i * t.element_size()}) still holds the poison "
                           f"pattern ({n_stale} of {t.numel()} elements)")
        return out

    def check(self, written=()):
        found = self.problems(written)
        if found:
            raise ArenaError("\n".join(found))


class _Recorder:
    """Stands in for the ctypes library: hands out its functions and notes the name of every nsdp_* entry asked for."""

    def __init__(self, real, called):
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "_called", called)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.startswith("nsdp_"):
            self._called.add(name)
        return fn


class _TorchProxy:
    """`torch` as a wrapper module sees it inside PoisonArena.routed()."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def _mine(self, device):
        return device is not None and torch.device(device).type == self._arena.device.type

    @staticmethod
    def _shape(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            return tuple(size[0])
        return tuple(size)

    @staticmethod
    def _plain(what, kw):
        """A routed allocation is a plain contiguous tensor: a keyword the arena cannot honour is an error, never dropped."""
        if kw:
            raise ArenaError(f"routed torch.{what}: keyword arguments {sorted(kw)} cannot be carried into the arena")

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        self._plain("empty", kw)
        return self._arena._routed_alloc(self._shape(size), dtype or torch.float32, False)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        self._plain("zeros", kw)
        return self._arena._routed_alloc(self._shape(size), dtype or torch.float32, True)

    def empty_like(self, t, **kw):
        if kw or not self._mine(t.device) or not t.is_contiguous():
            return torch.empty_like(t, **kw)
        return self._arena._routed_alloc(t.shape, t.dtype, False)

    def zeros_like(self, t, **kw):
        if kw or not self._mine(t.device) or not t.is_contiguous():
            return torch.zeros_like(t, **kw)
        return self._arena._routed_alloc(t.shape, t.dtype, True)
