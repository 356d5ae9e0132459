"""CPU tests of the argument rules of the ragged repair + CRC entry points
(hrs_decode_batch_ragged_crc_dev, hrs_decode_batch_ragged_host_crc) on a
host-only handle, in the order include/hrs.h states them: (1) the handle,
(2) the sibling's argument block, (3) with work to do a NULL crc_out and then
the overlap rule, (4) valid, (5) the empty batch, (6) len and the valid
entries, (7) the plans, (8) the 32-survivor limit, (9) the device. Each case
breaks one rule and every later rule it can, so the order shows: the answer is
the first broken rule's. A refused or empty call touches nothing, the CRC
arrays included."""
import ctypes

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, HrsError, _lib, device

NONE = -2  # HRS_DEVICE_NONE
K, P, S, L = 10, 4, 3, 256
N = K + P
FILL = 0xA5
CRC_FILL = 0xC3C3C3C3
NAMES = ("hrs_decode_batch_ragged_crc_dev", "hrs_decode_batch_ragged_host_crc")


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


class Buffers:
    """One small host batch under a fill pattern (host addresses: no call here
    gets as far as a device), its erasure lists, a valid array and CRC arrays.
    later_rules_broken() breaks rules 6, 7 and 8's neighbours at once: a valid
    entry beyond len and an erased location out of range."""

    def __init__(self, k=K, p=P, s=S):
        self.n, self.p, self.s = k + p, p, s
        self.st = np.full((s, k + p, L), FILL, np.uint8)
        self.out = np.full((s, p, L), FILL, np.uint8)
        self.erased = np.full((s, p), -1, np.int32)
        self.erased[:, 0] = p  # every stripe lost data cell 0
        self.valid = np.full((s, k + p), L // 2, np.uint32)
        self.crcs = np.full(2 * s * p, CRC_FILL, np.uint32)  # crc_in, then crc_out
        self.snap()

    def later_rules_broken(self):
        self.valid[1, 2] = L + 1
        self.erased[2, 0] = self.n
        self.snap()
        return self

    def snap(self):
        self.before = (self.valid.copy(), self.erased.copy())

    def untouched(self):
        return bool((self.st == FILL).all() and (self.out == FILL).all() and (self.valid == self.before[0]).all()
                    and (self.erased == self.before[1]).all() and (self.crcs == CRC_FILL).all())


def call(name, h, b, *, stripes=True, out=True, erased=True, valid=True, nstripes=None, length=L, max_erased=None,
         crc_in="in", crc_out="out"):
    """One call; the keyword flags replace an argument by NULL. crc_in / crc_out:
    None, "in" / "out" (the two halves of b.crcs), or a word offset into b.crcs."""
    words = b.s * b.p

    def crc_ptr(x):
        if x is None:
            return None
        at = {"in": 0, "out": words}.get(x, x)
        return b.crcs.ctypes.data + 4 * at

    args = [h, b.st.ctypes.data if stripes else None, L, b.n * L, b.erased.ctypes.data if erased else None,
            b.p if max_erased is None else max_erased, b.out.ctypes.data if out else None, L, b.p * L, length,
            b.s if nstripes is None else nstripes, b.valid.ctypes.data if valid else None, crc_ptr(crc_in),
            crc_ptr(crc_out)]
    if name.endswith("_dev"):
        args.append(None)
    return getattr(_lib.lib(), name)(*args)


def last_error(code):
    return _lib.lib().hrs_last_error(code._handle()).decode()


def test_the_symbols_are_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert hasattr(device, "decode_batch_ragged_crc") and hasattr(device, "decode_batch_host_ragged_crc")
    blob = open(_lib.LIB_PATH, "rb").read()
    for nout in (1, 2, 3, 4):
        for ninb in (4, 8, 12):
            present = b"23batch_ragged_crc_kernelILi%dELi%dELi768EE" % (nout, ninb) in blob
            assert present == (not (nout == 4 and ninb == 12))
    assert b"batch_ragged_crc_fold_kernel" in blob
    header = open(_lib.LIB_PATH.rsplit("/", 2)[0] + "/include/hrs.h").read()
    for name in NAMES:
        assert name + "(" in header
    assert "ragged repair + CRC-32" in header


@pytest.mark.parametrize("name", NAMES)
def test_rule_1_null_handle(name):
    b = Buffers().later_rules_broken()
    for kw in (dict(), dict(stripes=False), dict(crc_out=None), dict(valid=False), dict(nstripes=0)):
        assert call(name, None, b, **kw) == _lib.HRS_EINVAL
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kw", [dict(stripes=False), dict(out=False), dict(erased=False), dict(max_erased=-1),
                                dict(max_erased=9)], ids=["stripes", "out", "erased", "negative", "nine"])
def test_rule_2_the_siblings_argument_block(code, name, kw):
    """Before the CRC arrays, valid and the empty batch, with the sibling's message."""
    b = Buffers().later_rules_broken()
    for more in (dict(), dict(crc_out=None), dict(crc_in=1), dict(valid=False), dict(nstripes=0), dict(length=0),
                 dict(crc_out=None, valid=False, length=2**32)):
        assert call(name, code._handle(), b, **kw, **more) == _lib.HRS_EINVAL
        assert "bad batch decode arguments" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_3_null_crc_out_then_the_overlap_rule(code, name):
    """With work to do: before valid, len, the valid entries and the plans."""
    b = Buffers().later_rules_broken()
    for more in (dict(), dict(valid=False), dict(length=2**32), dict(crc_in=None), dict(crc_in=1)):
        assert call(name, code._handle(), b, crc_out=None, **more) == _lib.HRS_EINVAL
        assert "crc_out is NULL" in last_error(code)
    words = S * P
    for cin, cout in ((0, 1), (1, 0), (0, words - 1), (words - 1, 0)):
        for more in (dict(), dict(valid=False), dict(length=2**32)):
            assert call(name, code._handle(), b, crc_in=cin, crc_out=cout, **more) == _lib.HRS_EINVAL
            assert "overlap" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_3_aliasing_and_adjacent_arrays_pass_on(code, name):
    """crc_out may be crc_in itself, arrays that only touch are apart, a NULL
    crc_in is a fresh CRC32: each reaches the next broken rule (valid)."""
    b = Buffers().later_rules_broken()
    for cin, cout in ((0, 0), (0, S * P), (S * P, 0), (None, 0)):
        assert call(name, code._handle(), b, crc_in=cin, crc_out=cout, valid=False) == _lib.HRS_EINVAL
        assert "valid is NULL" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_4_null_valid_comes_before_the_empty_batch(code, name):
    b = Buffers().later_rules_broken()
    for kw in (dict(), dict(nstripes=0), dict(length=0), dict(max_erased=0), dict(length=2**32)):
        assert call(name, code._handle(), b, valid=False, **kw) == _lib.HRS_EINVAL
        assert "valid is NULL" in last_error(code)
    # an empty batch has no work to do: rule 3 does not apply, rule 4 does
    assert call(name, code._handle(), b, valid=False, crc_out=None, nstripes=0) == _lib.HRS_EINVAL
    assert "valid is NULL" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_5_empty_batches_touch_nothing(code, name):
    """Not the CRC arrays either, which need not even exist; later rules are not looked at."""
    b = Buffers().later_rules_broken()
    for kw in (dict(nstripes=0), dict(length=0), dict(max_erased=0)):
        for crcs in (dict(), dict(crc_out=None, crc_in=None), dict(crc_in=1)):
            assert call(name, code._handle(), b, **kw, **crcs) == _lib.HRS_OK
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("stripe,loc", [(0, 0), (1, 7), (S - 1, N - 1)])
def test_rule_6_valid_beyond_len_names_the_stripe_and_location(code, name, stripe, loc):
    """Before the plans are built: stripe 2's erasure list is out of range."""
    b = Buffers()
    b.valid[stripe, loc] = L + 1
    b.erased[S - 1, 0] = N
    b.snap()
    assert call(name, code._handle(), b) == _lib.HRS_EINVAL
    assert f"stripe {stripe} location {loc}" in last_error(code) and f"exceeds len {L}" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_6_len_beyond_uint32(code, name):
    b = Buffers().later_rules_broken()
    assert call(name, code._handle(), b, length=2**32) == _lib.HRS_EINVAL
    assert "exceeds 2^32 - 1" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_7_the_plans_refuse_as_the_siblings_do(code, name):
    b = Buffers()
    b.erased[1, 0] = N
    b.snap()
    assert call(name, code._handle(), b) == _lib.HRS_EINVAL
    assert "stripe 1: erased location %d out of range" % N in last_error(code)
    b = Buffers()
    more = np.full((S, P + 1), -1, np.int32)
    more[2] = range(P + 1)
    b.erased, b.out = more, np.full((S, P + 1, L), FILL, np.uint8)
    crcs = np.full(2 * S * (P + 1), CRC_FILL, np.uint32)
    b.snap()
    args = [code._handle(), b.st.ctypes.data, L, N * L, more.ctypes.data, P + 1, b.out.ctypes.data, L, (P + 1) * L, L,
            S, b.valid.ctypes.data, crcs.ctypes.data, crcs.ctypes.data + 4 * S * (P + 1)]
    assert getattr(_lib.lib(), name)(*(args + [None] * name.endswith("_dev"))) == _lib.HRS_ETOOMANY
    assert b.untouched() and (crcs == CRC_FILL).all()


@pytest.mark.parametrize("name", NAMES)
def test_rule_8_more_than_32_survivors_is_refused_before_the_device(name):
    wide = HipReedSolomonCode(40, 4, device=NONE)
    b = Buffers(40, 4, 3)
    b.erased[0, 0] = -1  # stripe 0 lost nothing: stripe 1 is the first with such a pattern
    b.snap()
    assert call(name, wide._handle(), b) == _lib.HRS_EINVAL
    msg = _lib.lib().hrs_last_error(wide._handle()).decode()
    assert "stripe 1" in msg and "40 survivors" in msg and "32" in msg
    b.valid[...] = L  # an all-full batch is refused too: the rule comes before the route
    b.snap()
    assert call(name, wide._handle(), b) == _lib.HRS_EINVAL
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fill", [0, L // 2, L], ids=["all_dead", "half", "all_full"])
def test_rule_9_valid_arguments_reach_the_device(code, name, fill):
    b = Buffers()
    b.valid[...] = fill
    b.snap()
    for crcs in (dict(), dict(crc_in=None), dict(crc_in="out")):
        assert call(name, code._handle(), b, **crcs) == _lib.HRS_EDEVICE
        assert "device" in last_error(code)
    assert _lib.lib().hrs_last_host_path(code._handle()) == b""  # set only on success
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_9_a_batch_that_lost_nothing_still_needs_the_device(code, name):
    """Its CRCs continue over no bytes, on the device: the fold runs."""
    b = Buffers()
    b.erased[...] = -1
    b.snap()
    assert call(name, code._handle(), b) == _lib.HRS_EDEVICE
    assert b.untouched()


# ---- the Python mirror

def test_mirror_checks_shapes_before_the_library(code):
    st = np.zeros((S, N, L), np.uint8)
    out = np.zeros((S, 1, L), np.uint8)
    with pytest.raises(ValueError, match=r"valid must be \[S, 14\]"):
        device.decode_batch_host_ragged_crc(code, st, [[P]] * S, out, np.zeros((S, K), np.uint32))
    valid = np.full((S, N), L // 2, np.uint32)
    with pytest.raises(ValueError, match="crc_in must be"):
        device.decode_batch_host_ragged_crc(code, st, [[P]] * S, out, valid, crc_in=np.zeros((S, 2), np.uint32))
    with pytest.raises(ValueError, match="crc_out must be"):
        device.decode_batch_host_ragged_crc(code, st, [[P]] * S, out, valid, crc_out=np.zeros((S, 1), np.int32))


def test_mirror_passes_valid_arguments_on(code):
    st = np.zeros((S, N, L), np.uint8)
    out = np.zeros((S, 1, L), np.uint8)
    crc = np.zeros((S, 1), np.uint32)
    for valid in ([[L // 2] * N] * S, np.full((S, N), L, np.int64)):
        with pytest.raises(HrsError) as ei:
            device.decode_batch_host_ragged_crc(code, st, [[P]] * S, out, valid, crc_in=crc, crc_out=crc)
        assert ei.value.status == _lib.HRS_EDEVICE
    with pytest.raises(HrsError) as ei:
        device.decode_batch_host_ragged_crc(code, st, [[P]] * S, out, np.full((S, N), L + 1))
    assert ei.value.status == _lib.HRS_EINVAL
