"""CPU tests of the argument rules of the repair-batch and host-batch entry
points (hrs_decode_batch_dev, hrs_decode_batch_crc_dev, hrs_decode_batch_host,
hrs_decode_batch_host_crc, hrs_encode_batch_host, hrs_encode_batch_host_crc) on
a host-only handle: every rule that is settled before a device is selected,
in the order the library applies them (handle, argument block, empty batch,
stripe count, CRC arrays, erased locations, device). The CRC arrays' own rules
are in test_batch_crc_abi.py."""
import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, _lib

NONE = -2  # HRS_DEVICE_NONE
K, P, S, E, L = 10, 4, 3, 2, 256
N = K + P
DECODE = ("hrs_decode_batch_dev", "hrs_decode_batch_crc_dev", "hrs_decode_batch_host", "hrs_decode_batch_host_crc")
ENCODE = ("hrs_encode_batch_host", "hrs_encode_batch_host_crc")
FILL = 0xA5


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


class Buffers:
    """One small host batch; the outputs and CRC words carry a fill pattern so
    a test can tell that a refused or empty call wrote nothing."""

    def __init__(self):
        self.st = np.full((S, N, L), FILL, np.uint8)
        self.out = np.full((S, E, L), FILL, np.uint8)
        self.er = np.array([[0, 5], [3, -1], [-1, -1]], np.int32)
        self.crc = np.full(S * N, 0xA5A5A5A5, np.uint32)

    def untouched(self):
        return bool((self.st == FILL).all() and (self.out == FILL).all() and (self.crc == 0xA5A5A5A5).all())


def call_decode(name, h, b, *, stripes=True, out=True, erased=True, max_erased=E, nstripes=S, length=L, crc_out=True):
    """One decode-batch call; the keyword flags replace an argument by NULL."""
    args = [h, b.st.ctypes.data if stripes else None, L, N * L, b.er.ctypes.data if erased else None, max_erased,
            b.out.ctypes.data if out else None, L, E * L, length, nstripes]
    if "crc" in name:
        args += [None, b.crc.ctypes.data if crc_out else None]
    if name.endswith("_dev"):
        args.append(None)  # stream
    return getattr(_lib.lib(), name)(*args)


def call_encode(name, h, b, *, stripes=True, nstripes=S, length=L, crc_out=True):
    args = [h, b.st.ctypes.data if stripes else None, L, N * L, length, nstripes]
    if "crc" in name:
        args += [None, b.crc.ctypes.data if crc_out else None]
    return getattr(_lib.lib(), name)(*args)


def last_error(code):
    return _lib.lib().hrs_last_error(code._handle()).decode()


# (case id, keyword arguments of call_decode, status, message substring or None)
BAD_BLOCK = "bad batch decode arguments"
DECODE_CASES = [
    ("null_stripes", dict(stripes=False), _lib.HRS_EINVAL, BAD_BLOCK),
    ("null_out", dict(out=False), _lib.HRS_EINVAL, BAD_BLOCK),
    ("max_erased_negative", dict(max_erased=-1), _lib.HRS_EINVAL, BAD_BLOCK),
    ("max_erased_9", dict(max_erased=9), _lib.HRS_EINVAL, BAD_BLOCK),
    ("null_erased_list", dict(erased=False), _lib.HRS_EINVAL, BAD_BLOCK),
    # the argument block comes before the empty batch
    ("null_stripes_empty", dict(stripes=False, nstripes=0), _lib.HRS_EINVAL, BAD_BLOCK),
    ("null_out_empty", dict(out=False, nstripes=0), _lib.HRS_EINVAL, BAD_BLOCK),
    ("max_erased_negative_empty", dict(max_erased=-1, nstripes=0), _lib.HRS_EINVAL, BAD_BLOCK),
    ("max_erased_9_empty", dict(max_erased=9, nstripes=0), _lib.HRS_EINVAL, BAD_BLOCK),
    ("null_erased_list_empty", dict(erased=False, nstripes=0), _lib.HRS_EINVAL, BAD_BLOCK),
    # nothing can be lost: an empty call, whatever crc_out is
    ("max_erased_0", dict(max_erased=0, erased=False, crc_out=False), _lib.HRS_OK, None),
    ("no_stripes", dict(nstripes=0, crc_out=False), _lib.HRS_OK, None),
    ("no_bytes", dict(length=0, crc_out=False), _lib.HRS_OK, None),
    # the stripe count is refused before crc_out is looked at and before any buffer is read
    ("too_many_stripes", dict(nstripes=2**31), _lib.HRS_EINVAL, "too many stripes"),
    ("too_many_stripes_null_crc_out", dict(nstripes=2**31, crc_out=False), _lib.HRS_EINVAL, "too many stripes"),
    ("valid", dict(), _lib.HRS_EDEVICE, "device"),
]


@pytest.mark.parametrize("name", DECODE)
@pytest.mark.parametrize("case", DECODE_CASES, ids=[c[0] for c in DECODE_CASES])
def test_decode_batch_argument_rules(code, name, case):
    _, kw, status, message = case
    b = Buffers()
    assert call_decode(name, code._handle(), b, **kw) == status
    if message:
        assert message in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", DECODE)
def test_decode_batch_null_handle_is_einval(name):
    b = Buffers()
    assert call_decode(name, None, b) == _lib.HRS_EINVAL
    assert call_decode(name, None, b, nstripes=0) == _lib.HRS_EINVAL
    assert b.untouched()


@pytest.mark.parametrize("name", DECODE)
def test_decode_batch_erased_location_out_of_range_beats_the_device(code, name):
    b = Buffers()
    b.er[1, 0] = N
    assert call_decode(name, code._handle(), b) == _lib.HRS_EINVAL
    assert "out of range" in last_error(code)
    assert b.untouched()


@pytest.mark.parametrize("name", ENCODE)
def test_encode_batch_argument_rules(code, name):
    h = code._handle()
    b = Buffers()
    assert call_encode(name, None, b) == _lib.HRS_EINVAL
    assert call_encode(name, None, b, nstripes=0) == _lib.HRS_EINVAL
    for kw in (dict(), dict(nstripes=0), dict(length=0)):  # before the empty batch
        assert call_encode(name, h, b, stripes=False, **kw) == _lib.HRS_EINVAL
        assert "stripes is NULL" in last_error(code)
    for kw in (dict(nstripes=0), dict(length=0)):
        assert call_encode(name, h, b, crc_out=False, **kw) == _lib.HRS_OK
        assert call_encode(name, h, b, **kw) == _lib.HRS_OK
    assert call_encode(name, h, b) == _lib.HRS_EDEVICE
    assert "device" in last_error(code)
    assert b.untouched()
