"""Guarded arena: every buffer handed to an ABI entry point is carved from ONE uint8 allocation with a guard band on each side,
so that a write past an end, a modified `const` input or an output that depends on bytes outside the declared inputs is
reported by name instead of landing silently in memory the process owns anyway.  Helper only (no tests in this file).

Layout.  Buffers start 256-byte aligned (the library's own carving granule).  The trailing guard of a buffer begins at its last
byte + 1, not at the next aligned address; the leading guard of the next buffer ends where that buffer starts.  Each guard is at
least GUARD bytes wide: 256 KiB, more than the largest single tile a workgroup of this library can emit past an end (one K-row of
an edge tensor at NAMP_MAX_K: 192 x 128 x 4 B = 96 KiB; a 64-row x 128 fp32 tile: 32 KiB).

Fills.  A run uses fill "A" or fill "B"; the dtype of the neighbouring buffer decides the guard bytes:
    float / bf16 neighbour   A: 0xFF bytes (NaN)      B: the fp32 value 1e30
    integer neighbour        A: all zero               B: the integer 1 (of the neighbour's width)
(0 and 1 are valid indices and masks at every shape used, so a stray index read moves a gather instead of leaving the arena.)
`out` and `ws` buffers are pre-filled with NaN bytes in A and 0x00 in B; `in` and `inout` buffers hold their data.

check() compares on the device and reads one flag back: every guard byte equals its fill, every `in` buffer equals its snapshot.
run_contract() runs a call under A (twice: is it bit-reproducible?) and under B and asserts the memory contract.  A buffer may
declare that only its first `compare` elements are defined by the header (padding rows a launch may fill with anything).
"""
from __future__ import annotations

import numpy as np
import torch

ALIGN = 256
GUARD = 256 * 1024
ROLES = ("in", "out", "inout", "ws")
NAMP_OK = 0


class GuardError(AssertionError):
    """A violated memory contract; .failures is a list of dicts (buffer, kind, side, first, last, count)."""

    def __init__(self, failures):
        self.failures = failures
        super().__init__("memory contract violated:\n  " + "\n  ".join(_describe(f) for f in failures))


def _describe(f):
    where = f"{f['kind']} {f['buffer']}" + (f" ({f['side']} guard)" if f.get("side") else "")
    return f"{where}: {f['count']} damaged {f.get('unit', 'byte')}s, first at offset {f['first']}, last at offset {f['last']}"


def _is_int(dtype):
    return not dtype.is_floating_point


class Buffer:
    """One registered buffer: a handle whose tensor / pointer are valid after Arena.build()."""

    def __init__(self, arena, name, role, dtype, shape, data, compare):
        assert role in ROLES, role
        self.arena, self.name, self.role, self.dtype = arena, name, role, dtype
        self.shape = tuple(int(s) for s in shape)
        self.numel = int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.nbytes = self.numel * self.itemsize
        self.compare = compare                    # number of leading elements the header defines (None: all of them)
        self.data = None
        if data is not None:
            self.data = data.detach().to("cpu", dtype).contiguous().view(-1).clone()
            assert self.data.numel() == self.numel, (name, self.data.numel(), self.numel)
        assert (self.data is not None) == (role in ("in", "inout")), f"{name}: `in` / `inout` buffers carry data, `out` / `ws` do not"
        self.start = self.end = None              # byte offsets in the arena

    @property
    def t(self):
        return self.arena.mem[self.start:self.end].view(self.dtype).view(self.shape)

    @property
    def ptr(self):
        return self.arena.mem.data_ptr() + self.start

    def __int__(self):
        return self.ptr


class Arena:
    def __init__(self, device="cpu", guard=GUARD):
        self.device = torch.device(device)
        self.guard = int(guard)
        self.buffers = []
        self.by_name = {}
        self.mem = None
        self.image = None
        self.fill = None
        self._cache = {}

    # ---- registration -------------------------------------------------------------------------------------------------
    def add(self, name, role, dtype, shape, data=None, compare=None):
        assert self.mem is None, "register every buffer before the first build()"
        assert name not in self.by_name, name
        b = Buffer(self, name, role, dtype, shape, data, compare)
        self.buffers.append(b)
        self.by_name[name] = b
        return b

    def inp(self, name, data, dtype=None):
        return self.add(name, "in", dtype or data.dtype, data.shape, data)

    def inout(self, name, data, dtype=None, compare=None):
        return self.add(name, "inout", dtype or data.dtype, data.shape, data, compare)

    def out(self, name, dtype, shape, compare=None):
        return self.add(name, "out", dtype, shape, None, compare)

    def ws(self, name, nbytes):
        return self.add(name, "ws", torch.uint8, (int(nbytes),))

    def __getitem__(self, name):
        return self.by_name[name]

    # ---- layout -------------------------------------------------------------------------------------------------------
    def _plan(self):
        off = self.guard                                          # leading guard of the first buffer
        for b in self.buffers:
            off = (off + ALIGN - 1) // ALIGN * ALIGN
            b.start, b.end = off, off + b.nbytes
            off = b.end + 2 * self.guard                          # its trailing guard + the next buffer's leading guard
        return off - self.guard

    def regions(self):
        """[(buffer, side, first byte, end byte)]: the guard bands.  A buffer's trailing guard starts at its last byte + 1."""
        out = []
        for i, b in enumerate(self.buffers):
            lead0 = 0 if i == 0 else self.buffers[i - 1].end + self.guard
            out.append((b, "leading", lead0, b.start))
            out.append((b, "trailing", b.end, b.end + self.guard))
        return out

    def _pattern(self, dtype, fill, lo, hi):
        """Guard bytes for arena offsets [lo, hi) beside a buffer of `dtype` (phase taken from the absolute offset)."""
        if _is_int(dtype):
            if fill == "A":
                return np.zeros(hi - lo, np.uint8)
            width = 8 if dtype == torch.int64 else 4
            word = np.frombuffer(np.array([1], dtype=f"<i{width}").tobytes(), np.uint8)
        else:
            if fill == "A":
                return np.full(hi - lo, 0xFF, np.uint8)
            width = 4
            word = np.frombuffer(np.array([1e30], dtype="<f4").tobytes(), np.uint8)
        return np.resize(np.roll(word, -(lo % width)), hi - lo)      # byte at offset o = word[o % width]

    def build(self, fill):
        """(Re)fill the whole arena for a run under fill "A" or "B": guards, pre-fills, input data, snapshot."""
        assert fill in ("A", "B")
        total = self._plan() if self.buffers else self.guard
        slack = ALIGN                                             # so that the first byte used can be put on a 256-byte address
        if self.mem is None:
            self._raw = torch.empty(total + slack, dtype=torch.uint8, device=self.device)
            shift = (-self._raw.data_ptr()) % ALIGN
            self.mem = self._raw[shift:shift + total]
        key = (fill, tuple(id(b.data) for b in self.buffers))
        if self._cache.get("key") == key and fill in self._cache:  # the same fill again (run A twice): a device copy
            self.fill = fill
            self.image, self.checked = self._cache[fill]
            self.mem.copy_(self.image)
            return self
        if self._cache.get("key") != key:
            self._cache = {"key": key}
        host = np.zeros(total, np.uint8)
        mask = np.zeros(total, np.uint8)                          # 1: guard byte, 2: byte of an `in` buffer
        for b, _side, lo, hi in self.regions():
            host[lo:hi] = self._pattern(b.dtype, fill, lo, hi)
            mask[lo:hi] = 1
        for b in self.buffers:
            if b.data is not None:
                host[b.start:b.end] = b.data.view(torch.uint8).numpy()
                if b.role == "in":
                    mask[b.start:b.end] = 2
            else:
                host[b.start:b.end] = 0xFF if fill == "A" else 0x00
        self.fill = fill
        self.image = torch.from_numpy(host).to(self.device)       # the snapshot: guards + inputs as they must still be afterwards
        self.checked = torch.from_numpy(mask).to(self.device)
        self._cache[fill] = (self.image, self.checked)
        self.mem.copy_(self.image)
        return self

    # ---- verification -------------------------------------------------------------------------------------------------
    def _damage(self, lo, hi):
        d = torch.nonzero(self.mem[lo:hi] != self.image[lo:hi]).view(-1)
        return None if d.numel() == 0 else (int(d[0]), int(d[-1]), int(d.numel()))

    def failures(self):
        """Guard bands (a) and `in` buffers (b) that differ from the snapshot; one device reduction when nothing is wrong."""
        bad = bool((((self.mem != self.image) & (self.checked != 0)).any()).item())
        if not bad:
            return []
        out = []
        for b, side, lo, hi in self.regions():
            dmg = self._damage(lo, hi)
            if dmg:
                first, last, count = dmg
                if side == "leading":                             # offsets relative to the buffer: negative in front of it
                    first, last = lo + first - b.start, lo + last - b.start
                else:                                             # ... and counted from the buffer's end behind it (end + 0 = first guard byte)
                    first, last = lo + first - b.end, lo + last - b.end
                out.append(dict(buffer=b.name, kind="guard write beside", side=side, first=first, last=last, count=count))
        for b in self.buffers:
            if b.role == "in":
                dmg = self._damage(b.start, b.end)
                if dmg:
                    out.append(dict(buffer=b.name, kind="modified input", side=None, first=dmg[0], last=dmg[1], count=dmg[2]))
        return out

    def check(self):
        """(a) guards intact, (b) inputs unchanged — GuardError otherwise; (c) returns copies of the `out` / `inout` buffers."""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        f = self.failures()
        if f:
            raise GuardError(f)
        return {b.name: b.t.clone() for b in self.buffers if b.role in ("out", "inout")}


def _defined(b, t):
    flat = t.reshape(-1)
    return flat if b.compare is None else flat[:b.compare]


def _bit_diff(b, x, y):
    """None when the defined elements of two copies of buffer b are bit-identical, else a failure record (element offsets)."""
    xb = _defined(b, x).contiguous().view(torch.uint8).view(-1, b.itemsize)
    yb = _defined(b, y).contiguous().view(torch.uint8).view(-1, b.itemsize)
    d = torch.nonzero((xb != yb).any(1)).view(-1)
    if d.numel() == 0:
        return None
    return dict(buffer=b.name, side=None, first=int(d[0]), last=int(d[-1]), count=int(d.numel()), unit="element")


def run_contract(fn, arena, *, tol=None, tol_buffers=(), canon=None):
    """Run fn(arena) -> return code under fill A (twice) and fill B and assert the memory contract:
      1. guards intact and `in` buffers unchanged in every run,
      2. `out` / `inout` bit-identical between A and B (nothing outside the declared inputs, and no initial content of `out` or
         `ws`, reaches an output).  Only the buffers named in `tol_buffers` — sums an entry point accumulates with fp32 atomics, in
         no fixed order — are compared at `tol` instead (relative to the largest entry; the caller names the tolerance's source),
      3. no NaN / Inf in a floating-point output (of either run: that is what the NaN guards and pre-fills of fill A are for),
      4. every return code is NAMP_OK.
    canon(outputs) -> outputs, optional: brings outputs whose order the header leaves undefined into a canonical order first.
    Returns (outputs of run A, reproducible): reproducible = the two runs under fill A agree to the bit in every output."""
    runs = {}
    for tag, fill in (("A", "A"), ("A2", "A"), ("B", "B")):
        arena.build(fill)
        rc = fn(arena)
        assert rc == NAMP_OK, f"run {tag}: return code {rc}, expected NAMP_OK"
        runs[tag] = arena.check()
        if canon is not None:
            runs[tag] = canon(runs[tag])
    outs = [b for b in arena.buffers if b.role in ("out", "inout")]
    unknown = set(tol_buffers) - {b.name for b in outs}
    assert not unknown, f"tol_buffers names no output: {sorted(unknown)}"
    reproducible = all(_bit_diff(b, runs["A"][b.name], runs["A2"][b.name]) is None for b in outs)
    fails = []
    for b in outs:
        for tag in ("A", "B"):
            t = runs[tag][b.name]
            if t.dtype.is_floating_point:
                d = torch.nonzero(~torch.isfinite(_defined(b, t).float())).view(-1)
                if d.numel():
                    fails.append(dict(buffer=b.name, kind=f"NaN/Inf (run {tag}: untouched pre-fill or bytes from outside) in output", side=None,
                                      first=int(d[0]), last=int(d[-1]), count=int(d.numel()), unit="element"))
        if b.name not in tol_buffers:
            d = _bit_diff(b, runs["A"][b.name], runs["B"][b.name])
            if d:
                d["kind"] = "fill-dependent output (A != B)"
                fails.append(d)
        else:
            assert tol is not None and b.dtype.is_floating_point, f"{b.name}: compared with a tolerance, but none was given"
            a, c = _defined(b, runs["A"][b.name]).double(), _defined(b, runs["B"][b.name]).double()
            bar = tol * max(float(a.abs().max()), 1e-30)
            d = torch.nonzero(~((a - c).abs() <= bar)).view(-1)
            if d.numel():
                fails.append(dict(buffer=b.name, kind=f"fill-dependent output (|A - B| > {tol:g} of the largest entry)", side=None,
                                  first=int(d[0]), last=int(d[-1]), count=int(d.numel()), unit="element"))
    if fails:
        raise GuardError(fails)
    return runs["A"], reproducible
