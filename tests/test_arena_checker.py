"""The guarded-arena checker (gpu_arena.py) cannot hide a failure: every
planted single-byte corruption is reported and classified, the layout keeps
its margins, and the footprint case table keeps its coverage. CPU only."""
import itertools

import numpy as np
import pytest

import test_gpu_footprint as fp
from gpu_arena import ARENA_MARGIN, GUARD, POISON, ROW_MARGIN, Arena, CrcArena

S = 3
LAYOUTS = list(itertools.product((0, 1), (0, 16, 5), (1, 17, 2049)))


def _arena(shift, pad, L):
    """Two inputs, the output y = a ^ b, and an output z the call must not write."""
    a = Arena(S, L, shift=shift, stripe_pad=pad, seed=L + pad)
    a.add("a", "input")
    a.add("b", "input")
    a.add("y", "output")
    a.add("z", "output")
    a.build()
    return a, a.expected({"y": a.pre("a") ^ a.pre("b")})


@pytest.mark.parametrize("shift,pad,L", LAYOUTS)
def test_layout_margins_and_alignment(shift, pad, L):
    a, _ = _arena(shift, pad, L)
    regs = sorted(a.regions(), key=lambda r: r[3])
    assert len(regs) == 4 * S
    assert regs[0][3] >= ARENA_MARGIN and a.size - (regs[-1][3] + L) >= ARENA_MARGIN
    for prev, cur in zip(regs, regs[1:]):
        assert cur[3] - (prev[3] + prev[4]) >= ROW_MARGIN  # no overlap, 64 guard bytes between any two rows
    host = a.host
    inside = np.zeros(a.size, bool)
    for _, kind, _, start, length in regs:
        inside[start:start + length] = True
        if kind == "output":
            assert (host[start:start + length] == POISON).all()
    assert (host[~inside] == GUARD).all() and inside.sum() == 4 * S * L
    assert a.aligned16() == (shift == 0 and pad % 16 == 0)
    assert (a.stripe_stride % 16 == 0) == (pad % 16 == 0) and a.row_pitch % 16 == 0
    assert all(r[3] % 16 == shift for r in regs if r[2] == 0)


@pytest.mark.parametrize("shift,pad,L", LAYOUTS)
def test_views_address_the_rows(shift, pad, L):
    """The strided views to_device() hands out (here on the CPU) are the rows."""
    a, _ = _arena(shift, pad, L)
    flat, v = a.to_device("cpu")
    for name in a.names:
        assert v[name].shape == (S, L) and v[name].stride() == (a.stripe_stride, 1)
        assert np.array_equal(v[name].numpy(), a.pre(name))
        assert v[name].data_ptr() - flat.data_ptr() == a.offset(name)
    st = a.stack(flat, ["b", "y", "z"])
    assert st.shape == (S, 3, L) and st.stride() == (a.stripe_stride, a.row_pitch, 1)
    assert all(np.array_equal(st[:, i].numpy(), a.pre(n)) for i, n in enumerate(["b", "y", "z"]))
    with pytest.raises(ValueError):
        a.stack(flat, ["a", "y"])
    v["y"][1, L - 1] ^= 0xFF  # a write through a view lands in the arena image
    assert flat.numpy()[a.offset("y", 1) + L - 1] == POISON ^ 0xFF


@pytest.mark.parametrize("shift,pad,L", LAYOUTS)
def test_planted_corruptions_are_reported(shift, pad, L):
    a, exp = _arena(shift, pad, L)
    assert a.diff(exp.copy(), exp) is None
    assert a.diff(a.host, exp) is not None  # an output left unwritten
    c = L // 2
    plants = [
        (a.offset("b", 1) - 1, "guard near b stripe 1 at -1"),
        (a.offset("y", 0) + L, "guard near y stripe 0 at +1"),
        (a.size - 1, f"guard near z stripe {S - 1} at +{ARENA_MARGIN}"),
        (0, f"guard near a stripe 0 at -{ARENA_MARGIN + shift}"),
        (a.offset("a", 2) + c, f"input a stripe 2 byte {c}"),
        (a.offset("y", 1) + L - 1, f"output y stripe 1 byte {L - 1}"),
        (a.offset("z", 2), "output z stripe 2 byte 0"),  # poison of the row declared "not written"
    ]
    for off, text in plants:
        after = exp.copy()
        after[off] ^= 0x01
        d = a.diff(after, exp)
        assert d is not None and d.startswith(f"1 mismatches; {text}: got {int(after[off]):#x}, want {int(exp[off]):#x}"), (d, text)
    after = exp.copy()
    for off, _ in plants:
        after[off] ^= 0x80
    assert a.diff(after, exp).startswith(f"{len(plants)} mismatches; guard near a stripe 0 at -")
    assert a.diff(exp[:-1], exp) is not None  # a truncated download is not "equal"


def test_expected_replaces_only_named_outputs():
    a, exp = _arena(0, 0, 17)
    changed = np.flatnonzero(exp != a.host)
    own = np.concatenate([np.arange(a.offset("y", s), a.offset("y", s) + 17) for s in range(S)])
    assert set(changed) <= set(own)
    with pytest.raises(ValueError):
        a.expected({"a": a.pre("a")})
    with pytest.raises(ValueError):
        a.expected({"y": np.zeros((S, 16), np.uint8)})


@pytest.mark.parametrize("with_in", [False, True])
def test_crc_arena(with_in):
    ncols = 14
    a = CrcArena(S, ncols, with_in, seed=3)
    words = (np.arange(S * ncols, dtype=np.uint64).reshape(S, ncols) * 2654435761 % (1 << 32)).astype(np.uint32)
    exp = a.expected(words)
    regs = sorted(a.regions(), key=lambda r: r[3])
    assert regs[0][3] * 4 >= ARENA_MARGIN and (a.host.size - (regs[-1][3] + ncols)) * 4 >= ARENA_MARGIN
    if with_in:
        assert (a.out_at - (a.in_at + S * ncols)) * 4 >= ROW_MARGIN
        assert np.array_equal(a.crc_in().reshape(-1), a.host[a.in_at:a.in_at + S * ncols])
    else:
        assert a.crc_in() is None
    assert a.diff(exp.view(np.int32).copy(), exp) is None
    plants = [(a.out_at - 1, "guard near crc_out stripe 0 at -1"),
              (a.out_at + S * ncols, f"guard near crc_out stripe {S - 1} at +1"),
              (a.host.size - 1, f"guard near crc_out stripe {S - 1} at +{ARENA_MARGIN // 4}"),
              (a.out_at + ncols + 3, "output crc_out stripe 1 word 3")]
    if with_in:
        plants.append((a.in_at + 2 * ncols, "input crc_in stripe 2 word 0"))
    for off, text in plants:
        after = exp.copy()
        after[off] ^= 1
        d = a.diff(after.view(np.int32), exp)
        assert d is not None and d.startswith(f"1 mismatches; {text}:"), (d, text)
    assert a.diff(a.host, exp) is not None


def test_footprint_table_keeps_its_coverage():
    fp.check_table()
    for fam in fp.FAMILIES:
        assert any(c.family == fam for c in fp.TABLE)
    # thinning the table trips the check
    for drop in (lambda c: c.place == "shift" and c.family == "xor_kernel",
                 lambda c: c.place == "pad5" and c.family == "batch_stream_kernel",
                 lambda c: c.family == "encode_cauchy_kernel",
                 lambda c: c.family == "decode_crc" and c.L % 2048 != 0,
                 lambda c: c.L == 65536):
        with pytest.raises(AssertionError):
            fp.check_table([c for c in fp.TABLE if not drop(c)])
    # every unaligned case expects a byte-granular kernel (or none), every entry point has cases
    assert {c.entry for c in fp.TABLE} == {"encode", "decode", "apply", "decode_batch", "encode_crc", "decode_crc",
                                           "crc32"}
