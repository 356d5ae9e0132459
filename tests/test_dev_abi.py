"""CPU tests of the argument rules of the six device entry points of
hrs_dispatch.cpp (hrs_encode_dev, hrs_decode_dev, hrs_apply_dev) and
hrs_crc_api.cpp (hrs_crc32_dev, hrs_encode_crc_dev, hrs_decode_crc_dev) on a
host-only handle: every rule that
is settled before a device is selected, in the order each entry applies them
(handle, argument block, NULL rows, empty call, erased / not-to-read
locations, device). The pointers stand for device memory and are never read:
a host-only handle ends every valid call with HRS_EDEVICE."""
import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, _lib

NONE = -2  # HRS_DEVICE_NONE
K, P, S, L = 10, 4, 3, 256
N = K + P
FILL = 0xA5
CRC_FILL = 0xA5A5A5A5
ENTRIES = ("hrs_encode_dev", "hrs_decode_dev", "hrs_apply_dev", "hrs_crc32_dev", "hrs_encode_crc_dev",
           "hrs_decode_crc_dev")
NO_DEVICE = "cannot select HIP device"


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


class Buffers:
    """Three stripes of n cells and of p output cells, the matrix of an apply
    and n CRC words per stripe; cells and CRC words carry a fill pattern so a
    test can tell that a refused or empty call wrote nothing."""

    def __init__(self):
        self.cells = np.full((S, N, L), FILL, np.uint8)
        self.out = np.full((S, P, L), FILL, np.uint8)
        self.m = np.full((2, 3), 7, np.uint8)
        self.crc = np.full(S * N, CRC_FILL, np.uint32)

    def rows(self, count, null=()):
        return _lib.ptr_array([None if i in null else self.cells[0, i].ctypes.data for i in range(count)])

    def outs(self, count, null=()):
        return _lib.ptr_array([None if o in null else self.out[0, o].ctypes.data for o in range(count)])

    def untouched(self):
        return bool((self.cells == FILL).all() and (self.out == FILL).all() and (self.m == 7).all() and
                    (self.crc == CRC_FILL).all())


def last_error(code):
    return _lib.lib().hrs_last_error(code._handle()).decode()


# One call of each entry; a keyword flag set to False replaces the argument by NULL.

def call_encode(h, b, *, in_rows=True, out_rows=True, length=L, nstripes=S, crc=False, crc_out=True, null_in=(),
                null_out=()):
    args = [h, b.rows(K, null_in) if in_rows else None, N * L, b.outs(P, null_out) if out_rows else None, P * L,
            length, nstripes]
    if crc:
        args += [None, b.crc.ctypes.data if crc_out else None]
    return getattr(_lib.lib(), "hrs_encode_crc_dev" if crc else "hrs_encode_dev")(*args, None)


def call_apply(h, b, *, m=True, in_rows=True, out_rows=True, nout=2, nin=3, length=L, nstripes=S):
    return _lib.lib().hrs_apply_dev(h, b.m.ctypes.data if m else None, nout, nin,
                                    b.rows(3) if in_rows else None, N * L, b.outs(2) if out_rows else None, P * L,
                                    length, nstripes, None)


def call_decode(h, b, *, rows=True, out_rows=True, erased=(5,), ne=None, erased_list=True, ntr=(5,), nn=None,
                ntr_list=True, length=L, nstripes=S, crc=False, crc_out=True):
    ne = len(erased) if ne is None else ne
    nn = len(ntr) if nn is None else nn
    args = [h, b.rows(N, null=ntr) if rows else None, N * L, b.outs(P) if out_rows else None, P * L,
            _lib.int_array(erased) if erased_list else None, ne, _lib.int_array(ntr) if ntr_list else None, nn,
            length, nstripes]
    if crc:
        args += [None, b.crc.ctypes.data if crc_out else None]
    return getattr(_lib.lib(), "hrs_decode_crc_dev" if crc else "hrs_decode_dev")(*args, None)


def call_crc32(h, b, *, rows=True, crc_out=True, nrows=5, null=(), length=L, nstripes=S):
    return _lib.lib().hrs_crc32_dev(h, b.rows(min(max(nrows, 1), N), null) if rows else None, nrows, N * L, length,
                                    nstripes, None, b.crc.ctypes.data if crc_out else None, None)


CALLS = {
    "hrs_encode_dev": call_encode,
    "hrs_decode_dev": call_decode,
    "hrs_apply_dev": call_apply,
    "hrs_crc32_dev": call_crc32,
    "hrs_encode_crc_dev": lambda h, b, **kw: call_encode(h, b, crc=True, **kw),
    "hrs_decode_crc_dev": lambda h, b, **kw: call_decode(h, b, crc=True, **kw),
}


def check(code, name, kw, status, message):
    b = Buffers()
    assert CALLS[name](code._handle(), b, **kw) == status
    if message:
        assert message in last_error(code)
    assert b.untouched()


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("name", ENTRIES)
def test_null_handle_is_einval(name):
    b = Buffers()
    assert CALLS[name](None, b) == _lib.HRS_EINVAL
    assert CALLS[name](None, b, nstripes=0) == _lib.HRS_EINVAL
    assert b.untouched()


# (case id, keyword arguments of the call, status, message substring or None)
ENCODE_CASES = [
    ("null_in_rows", dict(in_rows=False), _lib.HRS_EINVAL, "row arrays are NULL"),
    ("null_out_rows", dict(out_rows=False), _lib.HRS_EINVAL, "row arrays are NULL"),
    ("null_in_rows_empty", dict(in_rows=False, nstripes=0), _lib.HRS_EINVAL, "row arrays are NULL"),
    ("valid", dict(), _lib.HRS_EDEVICE, NO_DEVICE),
    # the device is selected before the empty call is looked at
    ("no_stripes", dict(nstripes=0), _lib.HRS_EDEVICE, NO_DEVICE),
    ("no_bytes", dict(length=0), _lib.HRS_EDEVICE, NO_DEVICE),
]


@pytest.mark.parametrize("case", ENCODE_CASES, ids=_ids(ENCODE_CASES))
def test_encode_dev_argument_rules(code, case):
    check(code, "hrs_encode_dev", *case[1:])


BAD_APPLY = "bad apply arguments"
APPLY_CASES = [
    ("null_m", dict(m=False), _lib.HRS_EINVAL, BAD_APPLY),
    ("null_in_rows", dict(in_rows=False), _lib.HRS_EINVAL, BAD_APPLY),
    ("null_out_rows", dict(out_rows=False), _lib.HRS_EINVAL, BAD_APPLY),
    ("nout_0", dict(nout=0), _lib.HRS_EINVAL, BAD_APPLY),
    ("nin_0", dict(nin=0), _lib.HRS_EINVAL, BAD_APPLY),
    ("nout_256", dict(nout=256), _lib.HRS_EINVAL, BAD_APPLY),
    ("nin_256", dict(nin=256), _lib.HRS_EINVAL, BAD_APPLY),
    ("null_m_empty", dict(m=False, nstripes=0), _lib.HRS_EINVAL, BAD_APPLY),
    ("valid", dict(), _lib.HRS_EDEVICE, NO_DEVICE),
    ("no_stripes", dict(nstripes=0), _lib.HRS_EDEVICE, NO_DEVICE),
    ("no_bytes", dict(length=0), _lib.HRS_EDEVICE, NO_DEVICE),
]


@pytest.mark.parametrize("case", APPLY_CASES, ids=_ids(APPLY_CASES))
def test_apply_dev_argument_rules(code, case):
    check(code, "hrs_apply_dev", *case[1:])


BAD_DECODE = "bad decode arguments"
# the rules hrs_decode_dev and hrs_decode_crc_dev share
DECODE_CASES = [
    ("null_rows", dict(rows=False), _lib.HRS_EINVAL, BAD_DECODE),
    ("ne_negative", dict(ne=-1), _lib.HRS_EINVAL, BAD_DECODE),
    ("nn_negative", dict(nn=-1), _lib.HRS_EINVAL, BAD_DECODE),
    ("null_out_rows", dict(out_rows=False), _lib.HRS_EINVAL, BAD_DECODE),
    ("null_erased", dict(erased_list=False), _lib.HRS_EINVAL, BAD_DECODE),
    ("null_ntr", dict(ntr_list=False), _lib.HRS_EINVAL, BAD_DECODE),
    # the argument block comes before the empty call
    ("null_rows_nothing_erased", dict(rows=False, erased=(), ntr=()), _lib.HRS_EINVAL, BAD_DECODE),
    ("null_ntr_nothing_erased", dict(erased=(), ntr_list=False), _lib.HRS_EINVAL, BAD_DECODE),
    ("null_rows_empty", dict(rows=False, nstripes=0), _lib.HRS_EINVAL, BAD_DECODE),
    # nothing erased: an empty call, whatever the output and erased arrays are
    ("nothing_erased", dict(erased=(), ntr=()), _lib.HRS_OK, None),
    ("nothing_erased_null_arrays", dict(erased=(), ntr=(), out_rows=False, erased_list=False, ntr_list=False,
                                        crc_out=False), _lib.HRS_OK, None),
    ("nothing_erased_ntr_out_of_range", dict(erased=(), ntr=(N,)), _lib.HRS_OK, None),
    # what decode5_matrix refuses comes before the device
    ("ntr_out_of_range", dict(ntr=(5, N)), _lib.HRS_EINVAL, "out of range"),
    ("ntr_negative", dict(ntr=(-1,)), _lib.HRS_EINVAL, "out of range"),
    ("ntr_more_than_p", dict(ntr=(5, 6, 7, 8, 9)), _lib.HRS_EINVAL, "not-to-read locations > parity size"),
    ("valid", dict(), _lib.HRS_EDEVICE, NO_DEVICE),
    ("valid_four_erased", dict(erased=(0, 5, 9, 13), ntr=(0, 5, 9, 13)), _lib.HRS_EDEVICE, NO_DEVICE),
    ("no_bytes", dict(length=0), _lib.HRS_EDEVICE, NO_DEVICE),
]
# hrs_decode_dev selects the device before run_apply looks at the stripe count
DECODE_ONLY = [
    ("no_stripes", dict(nstripes=0), _lib.HRS_EDEVICE, NO_DEVICE),
    ("no_stripes_ntr_out_of_range", dict(nstripes=0, ntr=(N,)), _lib.HRS_EINVAL, "out of range"),
]
# hrs_decode_crc_dev: crc_out belongs to the argument block, and no stripes is
# an empty call settled before the locations are looked at
DECODE_CRC_ONLY = [
    ("null_crc_out", dict(crc_out=False), _lib.HRS_EINVAL, BAD_DECODE),
    ("null_crc_out_empty", dict(crc_out=False, nstripes=0), _lib.HRS_EINVAL, BAD_DECODE),
    ("no_stripes", dict(nstripes=0), _lib.HRS_OK, None),
    ("no_stripes_ntr_out_of_range", dict(nstripes=0, ntr=(N,)), _lib.HRS_OK, None),
]


def _without(kw, key):
    return {k: v for k, v in kw.items() if k != key}


@pytest.mark.parametrize("case", DECODE_CASES + DECODE_ONLY, ids=_ids(DECODE_CASES + DECODE_ONLY))
def test_decode_dev_argument_rules(code, case):
    check(code, "hrs_decode_dev", _without(case[1], "crc_out"), *case[2:])


@pytest.mark.parametrize("case", DECODE_CASES + DECODE_CRC_ONLY, ids=_ids(DECODE_CASES + DECODE_CRC_ONLY))
def test_decode_crc_dev_argument_rules(code, case):
    check(code, "hrs_decode_crc_dev", *case[1:])


BAD_CRC32 = "bad crc32 arguments"
CRC32_CASES = [
    ("null_rows", dict(rows=False), _lib.HRS_EINVAL, BAD_CRC32),
    ("null_crc_out", dict(crc_out=False), _lib.HRS_EINVAL, BAD_CRC32),
    ("nrows_0", dict(nrows=0), _lib.HRS_EINVAL, BAD_CRC32),
    ("nrows_256", dict(nrows=256), _lib.HRS_EINVAL, BAD_CRC32),
    ("null_crc_out_empty", dict(crc_out=False, nstripes=0), _lib.HRS_EINVAL, BAD_CRC32),
    # a NULL row is refused only when there are bytes to read, and before the empty call
    ("null_row", dict(null=(3,)), _lib.HRS_EINVAL, "row 3 is NULL"),
    ("null_row_empty", dict(null=(3,), nstripes=0), _lib.HRS_EINVAL, "row 3 is NULL"),
    ("null_row_no_bytes", dict(null=(3,), length=0), _lib.HRS_EDEVICE, NO_DEVICE),
    ("null_row_no_bytes_empty", dict(null=(3,), length=0, nstripes=0), _lib.HRS_OK, None),
    ("no_stripes", dict(nstripes=0), _lib.HRS_OK, None),
    ("no_bytes", dict(length=0), _lib.HRS_EDEVICE, NO_DEVICE),
    ("valid", dict(), _lib.HRS_EDEVICE, NO_DEVICE),
    ("valid_one_row", dict(nrows=1), _lib.HRS_EDEVICE, NO_DEVICE),
]


@pytest.mark.parametrize("case", CRC32_CASES, ids=_ids(CRC32_CASES))
def test_crc32_dev_argument_rules(code, case):
    check(code, "hrs_crc32_dev", *case[1:])


NULL_ARRAYS = "row or crc arrays are NULL"
ENCODE_CRC_CASES = [
    ("null_in_rows", dict(in_rows=False), _lib.HRS_EINVAL, NULL_ARRAYS),
    ("null_out_rows", dict(out_rows=False), _lib.HRS_EINVAL, NULL_ARRAYS),
    ("null_crc_out", dict(crc_out=False), _lib.HRS_EINVAL, NULL_ARRAYS),
    ("null_crc_out_empty", dict(crc_out=False, nstripes=0), _lib.HRS_EINVAL, NULL_ARRAYS),
    # a NULL row is refused only when there are bytes to code, and before the empty call
    ("null_input_row", dict(null_in=(2,)), _lib.HRS_EINVAL, "input row 2 is NULL"),
    ("null_output_row", dict(null_out=(1,)), _lib.HRS_EINVAL, "output row 1 is NULL"),
    ("null_input_and_output_row", dict(null_in=(2,), null_out=(1,)), _lib.HRS_EINVAL, "input row 2 is NULL"),
    ("null_input_row_empty", dict(null_in=(2,), nstripes=0), _lib.HRS_EINVAL, "input row 2 is NULL"),
    ("null_input_row_no_bytes", dict(null_in=(2,), length=0), _lib.HRS_EDEVICE, NO_DEVICE),
    ("null_output_row_no_bytes", dict(null_out=(1,), length=0), _lib.HRS_EDEVICE, NO_DEVICE),
    ("null_output_row_no_bytes_empty", dict(null_out=(1,), length=0, nstripes=0), _lib.HRS_OK, None),
    ("no_stripes", dict(nstripes=0), _lib.HRS_OK, None),
    ("no_bytes", dict(length=0), _lib.HRS_EDEVICE, NO_DEVICE),
    ("valid", dict(), _lib.HRS_EDEVICE, NO_DEVICE),
]


@pytest.mark.parametrize("case", ENCODE_CRC_CASES, ids=_ids(ENCODE_CRC_CASES))
def test_encode_crc_dev_argument_rules(code, case):
    check(code, "hrs_encode_crc_dev", *case[1:])
