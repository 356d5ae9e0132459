"""Guarded arenas for footprint tests of the device kernels (DESIGN.md,
"Footprint tests").

Everything a call may touch lives in one flat host array filled with a guard
byte. Rows are cut out of it with guard bytes on every side, inputs hold
seeded random bytes, outputs a poison byte. A test uploads the arena, runs one
entry point on strided views of the device copy, downloads the whole arena and
compares it with `expected(...)`: the pre-call image with exactly the named
output rows replaced by the reference. That one comparison covers the outputs,
the guards, the inputs and every output row the call must leave alone.

Only to_device() needs torch and a device; the rest is numpy.
"""
import numpy as np

GUARD = 0xC3
POISON = 0xA5
GUARD_WORD = 0xC3C3C3C3
POISON_WORD = 0xA5A5A5A5
ROW_MARGIN = 64       # guard bytes before and after every row of every stripe
ARENA_MARGIN = 4096   # guard bytes before the first row and behind the last: two 2 KiB windows


def _describe(off, regions, unit):
    """Classifies flat offset `off`: regions are (name, kind, stripe, start, length)."""
    best = None
    for name, kind, s, start, length in regions:
        if start <= off < start + length:
            return f"{kind} {name} stripe {s} {unit} {off - start}"
        d = off - start if off < start else off - (start + length - 1)
        if best is None or abs(d) < abs(best[0]):
            best = (d, name, s)
    if best is None:
        return f"guard at offset {off}"
    return f"guard near {best[1]} stripe {best[2]} at {best[0]:+d}"


def _diff(after, expected, regions, unit, limit=4):
    after, expected = np.asarray(after), np.asarray(expected)
    if after.shape != expected.shape or after.dtype != expected.dtype:
        return f"arena images differ in shape or type: {after.shape} {after.dtype} vs {expected.shape} {expected.dtype}"
    bad = np.flatnonzero(after != expected)
    if bad.size == 0:
        return None
    parts = [f"{_describe(int(o), regions, unit)}: got {int(after[o]):#x}, want {int(expected[o]):#x}"
             for o in bad[:limit]]
    return f"{bad.size} mismatches; " + "; ".join(parts)


class Arena:
    """S stripes of named rows of L bytes. Row number r of stripe s starts at
    base + shift + r * row_pitch + s * stripe_stride; rows are numbered in the
    order they are added, so rows added one after the other form a [S, m, L]
    block with one row pitch (stack())."""

    def __init__(self, S, L, shift=0, stripe_pad=0, seed=0):
        if shift not in (0, 1) or S < 1 or L < 1 or stripe_pad < 0:
            raise ValueError("bad arena parameters")
        self.S, self.L, self.shift, self.stripe_pad = S, L, shift, stripe_pad
        self.row_pitch = (L + ROW_MARGIN + 15) // 16 * 16
        self.base = ARENA_MARGIN
        self.names, self.kinds = [], {}
        self._rng = np.random.default_rng(seed)
        self._data = {}
        self.host = None

    # -- building
    def add(self, name, kind):
        if self.host is not None or name in self.kinds or kind not in ("input", "output"):
            raise ValueError(f"cannot add {kind} row {name!r}")
        self.names.append(name)
        self.kinds[name] = kind
        if kind == "input":
            self._data[name] = self._rng.integers(0, 256, (self.S, self.L), dtype=np.uint8)
        return name

    def add_rows(self, prefix, count, kind):
        return [self.add(f"{prefix}{i}", kind) for i in range(count)]

    def build(self):
        """Lays the rows out; returns the pre-call host image (read-only)."""
        if self.host is None:
            self.stripe_stride = len(self.names) * self.row_pitch + self.stripe_pad
            last_end = self.offset(self.names[-1], self.S - 1) + self.L
            self.size = last_end + ARENA_MARGIN
            host = np.full(self.size, GUARD, dtype=np.uint8)
            for name in self.names:
                for s in range(self.S):
                    o = self.offset(name, s)
                    host[o:o + self.L] = self._data[name][s] if self.kinds[name] == "input" else POISON
            host.setflags(write=False)
            self.host = host
        return self.host

    # -- geometry (offsets into the flat array)
    def offset(self, name, stripe=0):
        return self.base + self.shift + self.names.index(name) * self.row_pitch + stripe * self.stripe_stride

    def regions(self):
        return [(n, self.kinds[n], s, self.offset(n, s), self.L) for n in self.names for s in range(self.S)]

    def aligned16(self):
        """Every row of every stripe starts on a 16-byte boundary of the arena
        (whose device copy starts on one)."""
        return all(start % 16 == 0 for _, _, _, start, _ in self.regions())

    def pre(self, name):
        """The pre-call bytes [S, L] of a row (a copy)."""
        host = self.build()
        return np.stack([host[self.offset(name, s):self.offset(name, s) + self.L] for s in range(self.S)])

    # -- device
    def to_device(self, device="cuda:0"):
        """Uploads the arena: (flat device tensor, {name: [S, L] strided view})."""
        import torch
        flat = torch.from_numpy(self.build().copy()).to(device)
        assert flat.data_ptr() % 16 == 0
        views = {n: torch.as_strided(flat, (self.S, self.L), (self.stripe_stride, 1), self.offset(n))
                 for n in self.names}
        return flat, views

    def stack(self, flat, names):
        """The [S, m, L] view over rows that were added one after the other."""
        import torch
        idx = [self.names.index(n) for n in names]
        if idx != list(range(idx[0], idx[0] + len(idx))):
            raise ValueError("rows of a stack must be consecutive")
        return torch.as_strided(flat, (self.S, len(idx), self.L), (self.stripe_stride, self.row_pitch, 1),
                                self.offset(names[0]))

    # -- checking
    def expected(self, outputs):
        """The pre-call image with exactly the named output rows replaced by
        outputs[name] ([S, L]). Output rows not named keep their poison."""
        exp = self.build().copy()
        for name, rows in outputs.items():
            if self.kinds.get(name) != "output":
                raise ValueError(f"{name!r} is not an output row")
            rows = np.asarray(rows, dtype=np.uint8)
            if rows.shape != (self.S, self.L):
                raise ValueError(f"output {name!r} must be [{self.S}, {self.L}]")
            for s in range(self.S):
                o = self.offset(name, s)
                exp[o:o + self.L] = rows[s]
        return exp

    def diff(self, after, expected):
        """None, or a short description of the first mismatches, each one
        classified: guard (nearest row, signed distance: -1 is the byte just
        before it, +1 the byte just after), input or output (row, stripe, byte)."""
        return _diff(after, expected, self.regions(), "byte")


class CrcArena:
    """The int32 counterpart for CRC words: crc_in (optional, seeded random)
    and crc_out (poison), each a contiguous [S, ncols] block as the entry
    points take them, between guard words."""

    def __init__(self, S, ncols, with_in, seed=0):
        self.S, self.ncols = S, ncols
        n = S * ncols
        margin, gap = ARENA_MARGIN // 4, ROW_MARGIN // 4
        self.in_at = margin if with_in else None
        self.out_at = margin + (n + gap if with_in else 0)
        host = np.full(self.out_at + n + margin, GUARD_WORD, dtype=np.uint32)
        if with_in:
            host[self.in_at:self.in_at + n] = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint32)
        host[self.out_at:self.out_at + n] = POISON_WORD
        host.setflags(write=False)
        self.host = host

    def regions(self):
        r = []
        for name, kind, at in (("crc_in", "input", self.in_at), ("crc_out", "output", self.out_at)):
            if at is not None:
                r += [(name, kind, s, at + s * self.ncols, self.ncols) for s in range(self.S)]
        return r

    def crc_in(self):
        """Pre-call running CRCs [S, ncols] (uint32), or None."""
        if self.in_at is None:
            return None
        return self.host[self.in_at:self.in_at + self.S * self.ncols].reshape(self.S, self.ncols).copy()

    def to_device(self, device="cuda:0"):
        """(flat int32 device tensor, crc_in pointer or None, crc_out pointer)."""
        import torch
        flat = torch.from_numpy(self.host.view(np.int32).copy()).to(device)
        p = flat.data_ptr()
        return flat, (None if self.in_at is None else p + 4 * self.in_at), p + 4 * self.out_at

    def expected(self, crc_out):
        exp = self.host.copy()
        if crc_out is not None:
            words = np.asarray(crc_out, dtype=np.uint32)
            if words.shape != (self.S, self.ncols):
                raise ValueError(f"crc_out must be [{self.S}, {self.ncols}]")
            exp[self.out_at:self.out_at + words.size] = words.reshape(-1)
        return exp

    def diff(self, after, expected):
        return _diff(np.asarray(after).view(np.uint32), expected, self.regions(), "word")
