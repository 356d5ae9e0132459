"""CPU tests of the argument rules of the ragged repair entry points
(hrs_decode_batch_ragged_dev, hrs_decode_batch_ragged_host) on a host-only
handle, in the order include/hrs.h states them: the handle, the sibling's
argument block, valid, the empty batch, len and the valid entries (the stripe
and location named), the plans (HRS_EINVAL / HRS_ETOOMANY), the 32-survivor
limit, then the device. A refused or empty call touches nothing. And the
Python mirror's own rule: a valid array of the wrong shape is a ValueError
before the library is called."""
import ctypes

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, HrsError, _lib, device

NONE = -2  # HRS_DEVICE_NONE
K, P, S, L = 10, 4, 3, 256
N = K + P
FILL = 0xA5
NAMES = ("hrs_decode_batch_ragged_dev", "hrs_decode_batch_ragged_host")


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


class Buffers:
    """One small host batch under a fill pattern (host addresses: no call here
    gets as far as a device), its erasure lists and a valid array."""

    def __init__(self, k=K, p=P, s=S):
        self.n, self.p, self.s = k + p, p, s
        self.st = np.full((s, k + p, L), FILL, np.uint8)
        self.out = np.full((s, p, L), FILL, np.uint8)
        self.erased = np.full((s, p), -1, np.int32)
        self.erased[:, 0] = p  # every stripe lost data cell 0
        self.valid = np.full((s, k + p), L // 2, np.uint32)
        self.snap()

    def snap(self):
        self.before = (self.valid.copy(), self.erased.copy())

    def untouched(self):
        return bool((self.st == FILL).all() and (self.out == FILL).all() and (self.valid == self.before[0]).all()
                    and (self.erased == self.before[1]).all())


def call(name, h, b, *, stripes=True, out=True, erased=True, valid=True, nstripes=None, length=L, max_erased=None):
    """One ragged repair call; the keyword flags replace an argument by NULL."""
    args = [h, b.st.ctypes.data if stripes else None, L, b.n * L, b.erased.ctypes.data if erased else None,
            b.p if max_erased is None else max_erased, b.out.ctypes.data if out else None, L, b.p * L, length,
            b.s if nstripes is None else nstripes, b.valid.ctypes.data if valid else None]
    if name.endswith("_dev"):
        args.append(None)
    return getattr(_lib.lib(), name)(*args)


def last_error(code):
    return _lib.lib().hrs_last_error(code._handle()).decode()


def test_the_symbols_are_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert hasattr(device, "decode_batch_ragged") and hasattr(device, "decode_batch_host_ragged")
    blob = open(_lib.LIB_PATH, "rb").read()
    for nout in (1, 2, 3, 4):
        for ninb in (4, 8, 12, 16):
            assert b"19batch_ragged_kernelILi%dELi%dEE" % (nout, ninb) in blob
    assert b"batch_ragged_bytewise_kernel" in blob
    header = open(_lib.LIB_PATH.rsplit("/", 2)[0] + "/include/hrs.h").read()
    for name in NAMES:
        assert name + "(" in header


@pytest.mark.parametrize("name", NAMES)
def test_rule_1_null_handle(name):
    b = Buffers()
    for kw in (dict(), dict(nstripes=0), dict(valid=False), dict(stripes=False)):
        assert call(name, None, b, **kw) == _lib.HRS_EINVAL
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kw", [dict(stripes=False), dict(out=False), dict(erased=False), dict(max_erased=-1),
                                dict(max_erased=9)], ids=["stripes", "out", "erased", "negative", "nine"])
def test_rule_2_the_siblings_argument_block(code, name, kw):
    """Before valid and before the empty batch, with the sibling's message."""
    b = Buffers()
    for more in (dict(), dict(valid=False), dict(nstripes=0), dict(length=0)):
        assert call(name, code._handle(), b, **kw, **more) == _lib.HRS_EINVAL
        assert "bad batch decode arguments" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_3_null_valid_comes_before_the_empty_batch(code, name):
    b = Buffers()
    for kw in (dict(), dict(nstripes=0), dict(length=0), dict(max_erased=0)):
        assert call(name, code._handle(), b, valid=False, **kw) == _lib.HRS_EINVAL
        assert "valid is NULL" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_4_empty_batches_touch_nothing(code, name):
    b = Buffers()
    b.valid[1, 2] = L + 1  # never looked at: the empty batch comes first
    b.erased[0, :] = 0     # nor is a bad erasure list
    b.snap()
    for kw in (dict(nstripes=0), dict(length=0), dict(max_erased=0)):
        assert call(name, code._handle(), b, **kw) == _lib.HRS_OK
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("stripe,loc", [(0, 0), (1, 7), (S - 1, N - 1)])
def test_rule_5_valid_beyond_len_names_the_stripe_and_location(code, name, stripe, loc):
    """Every entry is range-checked, those of locations neither read nor lost
    too (location 0 is neither here), and before the plans are built."""
    b = Buffers()
    b.valid[stripe, loc] = L + 1
    b.erased[S - 1, :] = range(P + 1, P + 1 + P)
    b.erased[S - 1, 1] = N  # out of range: rule 6 would refuse it
    b.snap()
    assert call(name, code._handle(), b) == _lib.HRS_EINVAL
    assert f"stripe {stripe} location {loc}" in last_error(code) and f"exceeds len {L}" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_5_len_beyond_uint32(code, name):
    """len = 2^32 is refused before any valid entry and any byte is read."""
    b = Buffers()
    b.valid[...] = 0xFFFFFFFF
    b.snap()
    assert call(name, code._handle(), b, length=2**32) == _lib.HRS_EINVAL
    assert "exceeds 2^32 - 1" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_6_the_plans_refuse_as_the_siblings_do(code, name):
    b = Buffers()
    b.erased[1, 0] = N
    b.snap()
    assert call(name, code._handle(), b) == _lib.HRS_EINVAL
    assert "stripe 1: erased location %d out of range" % N in last_error(code)
    b = Buffers()
    more = np.full((S, P + 1), -1, np.int32)
    more[2] = range(P + 1)
    b.erased, b.out = more, np.full((S, P + 1, L), FILL, np.uint8)
    b.snap()
    args = [code._handle(), b.st.ctypes.data, L, N * L, more.ctypes.data, P + 1, b.out.ctypes.data, L, (P + 1) * L, L,
            S, b.valid.ctypes.data]
    assert getattr(_lib.lib(), name)(*(args + [None] * name.endswith("_dev"))) == _lib.HRS_ETOOMANY
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_7_more_than_32_survivors_is_refused_with_the_stripe_named(name):
    """RS(40,4): the plain call repairs such a stripe through run_apply, one
    stripe at a time; the ragged batch kernels read at most 32 survivors."""
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
def test_rule_8_valid_arguments_reach_the_device(code, name, fill):
    b = Buffers()
    b.valid[...] = fill
    b.snap()
    assert call(name, code._handle(), b) == _lib.HRS_EDEVICE
    assert "device" in last_error(code)
    assert _lib.lib().hrs_last_host_path(code._handle()) == b""  # set only on success
    assert b.untouched()


# ---- the Python mirror

BAD_VALID = {
    "rank_1": lambda: np.zeros(S * N, np.uint32),
    "per_data_cell": lambda: np.zeros((S, K), np.uint32),
    "one_stripe_more": lambda: np.zeros((S + 1, N), np.uint32),
    "nested_list": lambda: [[0] * N] * (S - 1),
}


@pytest.mark.parametrize("bad", BAD_VALID, ids=list(BAD_VALID))
def test_mirror_refuses_a_wrong_valid_shape_before_the_library(code, bad):
    st = np.zeros((S, N, L), np.uint8)
    out = np.zeros((S, 1, L), np.uint8)
    with pytest.raises(ValueError, match=r"valid must be \[S, 14\]"):
        device.decode_batch_host_ragged(code, st, [[P]] * S, out, BAD_VALID[bad]())


def test_mirror_passes_valid_arguments_on(code):
    """Lists, other integer types and non-contiguous arrays are converted; the
    host-only handle then answers HRS_EDEVICE, and a bad entry HRS_EINVAL."""
    st = np.zeros((S, N, L), np.uint8)
    out = np.zeros((S, 1, L), np.uint8)
    for valid in ([[L // 2] * N] * S, np.full((S, N), L, np.int64), np.zeros((N, S), np.uint16).T):
        with pytest.raises(HrsError) as ei:
            device.decode_batch_host_ragged(code, st, [[P]] * S, out, valid)
        assert ei.value.status == _lib.HRS_EDEVICE
    with pytest.raises(HrsError) as ei:
        device.decode_batch_host_ragged(code, st, [[P]] * S, out, np.full((S, N), L + 1))
    assert ei.value.status == _lib.HRS_EINVAL
