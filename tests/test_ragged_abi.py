"""CPU tests of the argument rules of the ragged encode entry points
(hrs_encode_ragged_dev, hrs_encode_ragged_batch_host) on a host-only handle,
in the order include/hrs.h states them: the handle, the pointer arguments
(valid included), the empty batch, len and the valid entries (the stripe and
row named), then the device. A refused or empty call touches nothing. And the
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
NAMES = ("hrs_encode_ragged_dev", "hrs_encode_ragged_batch_host")


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


class Buffers:
    """One small host batch under a fill pattern, its row pointer arrays (host
    addresses: no call here gets as far as a device) and a valid array."""

    def __init__(self):
        self.st = np.full((S, N, L), FILL, np.uint8)
        self.valid = np.full((S, K), L // 2, np.uint32)
        base = self.st.ctypes.data
        self.ins = _lib.ptr_array([base + (P + j) * L for j in range(K)])
        self.outs = _lib.ptr_array([base + r * L for r in range(P)])
        self.valid_before = self.valid.copy()

    def untouched(self):
        return bool((self.st == FILL).all() and (self.valid == self.valid_before).all())


def call(name, h, b, *, rows=True, outs=True, valid=True, nstripes=S, length=L):
    """One ragged call; the keyword flags replace an argument by NULL."""
    v = b.valid.ctypes.data if valid else None
    if name.endswith("_dev"):
        return _lib.lib().hrs_encode_ragged_dev(h, b.ins if rows else None, N * L, b.outs if outs else None, N * L,
                                                length, nstripes, v, None)
    return _lib.lib().hrs_encode_ragged_batch_host(h, b.st.ctypes.data if rows and outs else None, L, N * L, length,
                                                   nstripes, v)


def last_error(code):
    return _lib.lib().hrs_last_error(code._handle()).decode()


def test_the_symbols_are_declared_exported_and_mirrored():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert hasattr(device, "encode_stripes_ragged") and hasattr(device, "encode_batch_host_ragged")
    blob = open(_lib.LIB_PATH, "rb").read()
    for k, p in [(3, 2), (6, 3), (10, 4), (12, 4)]:
        assert b"2rs20encode_ragged_kernelILi%dELi%dEE" % (k, p) in blob
    for k, p in [(10, 4), (6, 3)]:
        assert b"3nrs20encode_ragged_kernelILi%dELi%dEE" % (k, p) in blob
    assert b"encode_ragged_bytewise_kernel" in blob


@pytest.mark.parametrize("name", NAMES)
def test_rule_1_null_handle(name):
    b = Buffers()
    for kw in (dict(), dict(nstripes=0), dict(valid=False), dict(rows=False)):
        assert call(name, None, b, **kw) == _lib.HRS_EINVAL
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("null", ["rows", "outs", "valid"])
def test_rule_2_null_pointers_come_before_the_empty_batch(code, name, null):
    b = Buffers()
    for kw in (dict(), dict(nstripes=0), dict(length=0)):
        assert call(name, code._handle(), b, **{null: False}, **kw) == _lib.HRS_EINVAL
        assert "NULL" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_3_empty_batches_touch_nothing(code, name):
    b = Buffers()
    b.valid[1, 2] = L + 1  # never looked at: the empty batch comes first
    b.valid_before = b.valid.copy()
    assert call(name, code._handle(), b, nstripes=0) == _lib.HRS_OK
    assert call(name, code._handle(), b, length=0) == _lib.HRS_OK
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("stripe,row", [(0, 0), (1, 7), (S - 1, K - 1)])
def test_rule_4_valid_beyond_len_names_the_stripe_and_row(code, name, stripe, row):
    b = Buffers()
    b.valid[stripe, row] = L + 1
    b.valid_before = b.valid.copy()
    assert call(name, code._handle(), b) == _lib.HRS_EINVAL
    assert f"stripe {stripe} row {row}" in last_error(code) and f"exceeds len {L}" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_rule_4_len_beyond_uint32(code, name):
    """len = 2^32 is refused before any valid entry and any byte is read."""
    b = Buffers()
    assert call(name, code._handle(), b, length=2**32) == _lib.HRS_EINVAL
    assert "exceeds 2^32 - 1" in last_error(code)
    assert b.untouched()


def test_rule_4_null_row_pointer(code):
    b = Buffers()
    b.ins[3] = None
    assert call("hrs_encode_ragged_dev", code._handle(), b) == _lib.HRS_EINVAL
    assert "input row 3 is NULL" in last_error(code)
    b = Buffers()
    b.outs[1] = None
    assert call("hrs_encode_ragged_dev", code._handle(), b) == _lib.HRS_EINVAL
    assert "output row 1 is NULL" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fill", [0, L // 2, L], ids=["all_dead", "half", "all_full"])
def test_rule_5_valid_arguments_reach_the_device(code, name, fill):
    b = Buffers()
    b.valid[...] = fill
    b.valid_before = b.valid.copy()
    assert call(name, code._handle(), b) == _lib.HRS_EDEVICE
    assert "device" in last_error(code)
    assert _lib.lib().hrs_last_host_path(code._handle()) == b""  # set only on success
    assert b.untouched()


# ---- the Python mirror

BAD_VALID = {
    "rank_1": lambda: np.zeros(S * K, np.uint32),
    "one_row_short": lambda: np.zeros((S, K - 1), np.uint32),
    "one_stripe_more": lambda: np.zeros((S + 1, K), np.uint32),
    "per_location": lambda: np.zeros((S, N), np.uint32),
    "nested_list": lambda: [[0] * K] * (S - 1),
}


@pytest.mark.parametrize("bad", BAD_VALID, ids=list(BAD_VALID))
def test_mirror_refuses_a_wrong_valid_shape_before_the_library(code, bad):
    st = np.zeros((S, N, L), np.uint8)
    with pytest.raises(ValueError, match=r"valid must be \[S, 10\]"):
        device.encode_batch_host_ragged(code, st, BAD_VALID[bad]())


def test_mirror_passes_valid_arguments_on(code):
    """Lists, other integer types and non-contiguous arrays are converted; the
    host-only handle then answers HRS_EDEVICE, and a bad entry HRS_EINVAL."""
    st = np.zeros((S, N, L), np.uint8)
    for valid in ([[L // 2] * K] * S, np.full((S, K), L, np.int64), np.zeros((K, S), np.uint16).T):
        with pytest.raises(HrsError) as ei:
            device.encode_batch_host_ragged(code, st, valid)
        assert ei.value.status == _lib.HRS_EDEVICE
    with pytest.raises(HrsError) as ei:
        device.encode_batch_host_ragged(code, st, np.full((S, K), L + 1))
    assert ei.value.status == _lib.HRS_EINVAL
    with pytest.raises(ValueError):
        device.encode_batch_host_ragged(code, np.zeros((S, N - 1, L), np.uint8), np.zeros((S, K)))
