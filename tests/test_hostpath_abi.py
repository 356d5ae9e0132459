"""CPU tests of the rules the host-buffer entry points (hrs_encode,
hrs_encode_crc, hrs_decode, hrs_decode_crc, hrs_decode3, hrs_encode_submit,
hrs_decode_submit, hrs_collect, hrs_wait, hrs_release, hrs_ticket_shape,
hrs_set_timing, hrs_ticket_gpu_ms, hrs_pending) settle without a device, on a
host-only handle: the argument blocks and their messages, the order of the
checks (arguments, locations, empty call, device, rows), the empty
synchronous calls and the whole life of a zero-length asynchronous round."""
import ctypes

import numpy as np
import pytest

from lambdafs_amd import HipNativeReedSolomonCode, HipReedSolomonCode, HipSimpleRegeneratingCode, _lib
from lambdafs_amd._lib import int_array, ptr_array

NONE = -2  # HRS_DEVICE_NONE
K, P, L = 10, 4, 256
N = K + P
ERASED = [0, 5]
FILL = 0xA5A5A5A5
OK, EINVAL, EDEVICE = _lib.HRS_OK, _lib.HRS_EINVAL, _lib.HRS_EDEVICE
BAD_DECODE = "bad decode arguments"
NO_DEVICE = "cannot select HIP device"


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


def last_error(code):
    return _lib.lib().hrs_last_error(code._handle()).decode()


class Rows:
    """The buffers of one call: N read rows, P write rows, the location lists
    of a two-erasure decode, and CRC words that carry a fill pattern."""

    def __init__(self, code=None):
        self.data = np.full((N, L), 0x5A, np.uint8)
        self.out = np.full((P, L), 0xA5, np.uint8)
        self.reads = ptr_array([self.data[i].ctypes.data for i in range(N)])
        self.ins = ptr_array([self.data[P + i].ctypes.data for i in range(K)])
        self.writes = ptr_array([self.out[i].ctypes.data for i in range(P)])
        self.erased = int_array(ERASED)
        to_read = sorted(code.locationsToReadForDecode(ERASED)) if code else []
        self.to_read = int_array(to_read)
        self.nr = len(to_read)
        ntr = [x for x in range(N) if x not in to_read]
        self.ntr = int_array(ntr)
        self.nn = len(ntr)
        self.crc = np.full(N, FILL, np.uint32)

    def untouched(self):
        return bool((self.out == 0xA5).all() and (self.crc == FILL).all())


def decode_call(name, h, b, *, reads=True, writes=True, erased=True, ne=len(ERASED), to_read=True, nr=None, ntr=True,
                nn=None, length=L, crc_out=True, ticket=None):
    """One 5-argument decode through `name`; a False flag passes NULL."""
    loc = [b.erased if erased else None, ne, b.to_read if to_read else None, b.nr if nr is None else nr,
           b.ntr if ntr else None, b.nn if nn is None else nn]
    reads = b.reads if reads else None
    writes = b.writes if writes else None
    lib = _lib.lib()
    if name == "hrs_decode":
        return lib.hrs_decode(h, reads, writes, *loc, length)
    if name == "hrs_decode_crc":
        return lib.hrs_decode_crc(h, reads, writes, *loc, length, None, b.crc.ctypes.data if crc_out else None)
    t = ctypes.c_uint64(0) if ticket is None else ticket
    return lib.hrs_decode_submit(h, reads, *loc, length, 0, ctypes.byref(t))


DECODES = ("hrs_decode", "hrs_decode_crc", "hrs_decode_submit")


def test_null_handle_is_einval_everywhere():
    lib = _lib.lib()
    b = Rows()
    t = ctypes.c_uint64(7)
    ms = ctypes.c_float(0)
    assert lib.hrs_encode(None, b.ins, b.writes, L) == EINVAL
    assert lib.hrs_encode_crc(None, b.ins, b.writes, L, None, b.crc.ctypes.data) == EINVAL
    assert lib.hrs_encode_submit(None, b.ins, L, 1, ctypes.byref(t)) == EINVAL
    for name in DECODES:
        assert decode_call(name, None, b, ticket=t) == EINVAL
    assert lib.hrs_decode3(None, b.reads, b.writes, b.erased, 2, L) == EINVAL
    assert lib.hrs_collect(None, 1, b.writes, b.crc.ctypes.data) == EINVAL
    assert lib.hrs_wait(None, 1) == EINVAL
    assert lib.hrs_release(None, 1) == EINVAL
    assert lib.hrs_ticket_shape(None, 1, None, None, None) == EINVAL
    assert lib.hrs_set_timing(None, 1) == EINVAL
    assert lib.hrs_ticket_gpu_ms(None, 1, ctypes.byref(ms)) == EINVAL
    assert lib.hrs_pending(None) == -1
    assert t.value == 7 and b.untouched()


def test_encode_null_arguments(code):
    lib, h, b = _lib.lib(), code._handle(), Rows()
    t = ctypes.c_uint64(7)
    crc = b.crc.ctypes.data
    for ins, outs in ((None, b.writes), (b.ins, None), (None, None)):
        assert lib.hrs_encode(h, ins, outs, L) == EINVAL
        assert last_error(code) == "inputs/outputs is NULL"
    for ins, outs, cout in ((None, b.writes, crc), (b.ins, None, crc), (b.ins, b.writes, None)):
        assert lib.hrs_encode_crc(h, ins, outs, L, None, cout) == EINVAL
        assert last_error(code) == "inputs/outputs/crc_out is NULL"
        assert lib.hrs_encode_crc(h, ins, outs, 0, None, cout) == EINVAL  # before the empty call
    assert lib.hrs_encode_submit(h, None, L, 0, ctypes.byref(t)) == EINVAL
    assert last_error(code) == "inputs is NULL"
    assert lib.hrs_encode_submit(h, None, L, 0, None) == EINVAL
    assert last_error(code) == "inputs is NULL"
    assert lib.hrs_encode_submit(h, b.ins, L, 0, None) == EINVAL
    assert last_error(code) == "ticket is NULL"
    assert lib.hrs_encode_submit(h, b.ins, 0, 0, None) == EINVAL
    assert last_error(code) == "ticket is NULL"
    assert lib.hrs_pending(h) == 0 and t.value == 7 and b.untouched()


# (case id, keyword arguments of decode_call, the calls that refuse it)
BAD_DECODE_CASES = [
    ("null_reads", dict(reads=False), DECODES),
    ("null_reads_no_erasures", dict(reads=False, ne=0), DECODES),
    ("ne_negative", dict(ne=-1), DECODES),
    ("nn_negative", dict(nn=-1), DECODES),
    ("nr_negative", dict(nr=-1), DECODES),
    ("null_erased", dict(erased=False), DECODES),
    ("null_ntr", dict(ntr=False), DECODES),
    ("null_writes", dict(writes=False), ("hrs_decode", "hrs_decode_crc")),  # the submit takes no write_bufs
    ("null_crc_out", dict(crc_out=False), ("hrs_decode_crc",)),
]


@pytest.mark.parametrize("name,kw", [(n, c[1]) for c in BAD_DECODE_CASES for n in c[2]],
                         ids=[f"{n}-{c[0]}" for c in BAD_DECODE_CASES for n in c[2]])
def test_decode_argument_block(code, name, kw):
    b = Rows(code)
    t = ctypes.c_uint64(7)
    for length in (L, 0):  # before the empty call
        assert decode_call(name, code._handle(), b, ticket=t, length=length, **kw) == EINVAL
        assert last_error(code) == BAD_DECODE
    assert _lib.lib().hrs_pending(code._handle()) == 0 and t.value == 7 and b.untouched()


@pytest.mark.parametrize("name", DECODES)
def test_decode_location_out_of_range(code, name):
    h = code._handle()
    b = Rows(code)
    b.ntr[0] = N
    for length in (L, 0):
        assert decode_call(name, h, b, length=length) == EINVAL
        assert last_error(code) == f"location out of range [0,{N})"
    assert decode_call(name, h, b, ne=0) == EINVAL  # before the call without erasures
    assert last_error(code) == f"location out of range [0,{N})"
    assert decode_call(name, h, b, reads=False) == EINVAL  # the argument block comes first
    assert last_error(code) == BAD_DECODE
    assert _lib.lib().hrs_pending(h) == 0 and b.untouched()


@pytest.mark.parametrize("name", DECODES)
def test_decode_without_erasures_is_ok(code, name):
    """ne == 0 on an RS handle: nothing to write, so write_bufs, erased and
    crc_out may be NULL; the submit issues a ticket with no outputs."""
    h = code._handle()
    b = Rows(code)
    t = ctypes.c_uint64(0)
    assert decode_call(name, h, b, ne=0, writes=False, erased=False, crc_out=False, ticket=t) == OK
    assert b.untouched()
    if name == "hrs_decode_submit":
        nout, ln, ncrc = ctypes.c_int(-1), ctypes.c_size_t(99), ctypes.c_int(-1)
        assert t.value == 1
        assert _lib.lib().hrs_ticket_shape(h, t.value, ctypes.byref(nout), ctypes.byref(ln), ctypes.byref(ncrc)) == OK
        assert (nout.value, ln.value, ncrc.value) == (0, 0, 0)
        assert _lib.lib().hrs_collect(h, t.value, None, None) == OK
    assert _lib.lib().hrs_pending(h) == 0


def test_decode3_rules(code):
    lib, h, b = _lib.lib(), code._handle(), Rows()
    assert lib.hrs_decode3(h, b.reads, b.writes, b.erased, -1, L) == EINVAL
    assert last_error(code) == "bad decode3 arguments"
    for reads, writes, erased in ((None, b.writes, b.erased), (b.reads, None, b.erased), (b.reads, b.writes, None)):
        assert lib.hrs_decode3(h, reads, writes, erased, 2, L) == EINVAL
        assert last_error(code) == "bad decode3 arguments"
    assert lib.hrs_decode3(h, None, None, None, 0, L) == OK
    five = int_array([0, 1, 2, 3, 4])
    assert lib.hrs_decode3(h, b.reads, b.writes, five, 5, L) == EINVAL
    assert last_error(code) == f"5 erasures > parity size {P}"
    assert lib.hrs_decode3(h, b.reads, b.writes, five, 5, 0) == EINVAL  # before the empty call
    assert b.untouched()


@pytest.mark.parametrize("make", [lambda: HipNativeReedSolomonCode(K, P, device=NONE),
                                  lambda: HipSimpleRegeneratingCode(K, P, 2, device=NONE)], ids=["nrs", "src"])
def test_decode3_is_refused_by_nrs_and_src(make):
    other = make()
    b = Rows()
    for ne in (2, 0):
        assert _lib.lib().hrs_decode3(other._handle(), b.reads, b.writes, b.erased, ne, L) == EINVAL
        assert last_error(other) == "decodeBulk(readBufs, writeBufs, erasedLocations) is not supported by this code"
    assert _lib.lib().hrs_decode3(other._handle(), b.reads, b.writes, b.erased, -1, L) == EINVAL
    assert last_error(other) == "bad decode3 arguments"  # the argument block comes first
    assert b.untouched()


SYNC = ("hrs_encode", "hrs_encode_crc", "hrs_decode", "hrs_decode_crc", "hrs_decode3")
ASYNC = ("hrs_encode_submit", "hrs_encode_submit_crc", "hrs_decode_submit")


def valid_call(name, h, b, length, ticket=None, crc_in=None):
    lib = _lib.lib()
    t = ctypes.c_uint64(0) if ticket is None else ticket
    crc = b.crc.ctypes.data
    if name == "hrs_encode":
        return lib.hrs_encode(h, b.ins, b.writes, length)
    if name == "hrs_encode_crc":
        return lib.hrs_encode_crc(h, b.ins, b.writes, length, crc_in, crc)
    if name == "hrs_decode3":
        return lib.hrs_decode3(h, b.reads, b.writes, b.erased, len(ERASED), length)
    if name == "hrs_encode_submit":
        return lib.hrs_encode_submit(h, b.ins, length, 0, ctypes.byref(t))
    if name == "hrs_encode_submit_crc":
        return lib.hrs_encode_submit(h, b.ins, length, 1, ctypes.byref(t))
    if name == "hrs_decode_crc":
        return lib.hrs_decode_crc(h, b.reads, b.writes, b.erased, len(ERASED), b.to_read, b.nr, b.ntr, b.nn, length,
                                  crc_in, crc)
    return decode_call(name, h, b, length=length, ticket=t)


@pytest.mark.parametrize("null_row", [False, True], ids=["rows", "null_input_row"])
@pytest.mark.parametrize("name", SYNC + ASYNC)
def test_device_is_selected_before_the_rows_are_scanned(code, name, null_row):
    """A valid call with len > 0 needs the device, and says so even when an
    input row it would read is NULL: the rows are scanned after the guard."""
    h = code._handle()
    b = Rows(code)
    if null_row:
        b.ins[1] = None
        b.reads[P + 1] = None
    t = ctypes.c_uint64(7)
    assert valid_call(name, h, b, L, ticket=t) == EDEVICE
    assert NO_DEVICE in last_error(code)
    if name in ASYNC:  # no ticket, and the slot stays free
        assert t.value == 0 and _lib.lib().hrs_pending(h) == 0
    assert (b.out == 0xA5).all()  # (a checksummed call has set its running values by then)


@pytest.mark.parametrize("name", SYNC)
def test_empty_synchronous_call_needs_no_device(code, name):
    """len == 0: HRS_OK without a device; a checksummed call hands the running
    values through (crc_out[r] = crc_in[r], 0 for NULL crc_in)."""
    h = code._handle()
    b = Rows(code)
    ncrc = {"hrs_encode_crc": N, "hrs_decode_crc": len(ERASED)}.get(name, 0)
    assert valid_call(name, h, b, 0) == OK
    assert (b.crc[:ncrc] == 0).all() and (b.crc[ncrc:] == FILL).all() and (b.out == 0xA5).all()
    if ncrc:
        running = np.arange(1, N + 1, dtype=np.uint32) * np.uint32(0x01010101)
        assert valid_call(name, h, b, 0, crc_in=running.ctypes.data) == OK
        assert (b.crc[:ncrc] == running[:ncrc]).all() and (b.crc[ncrc:] == FILL).all()
        b.crc[:N] = running  # crc_out may be crc_in itself
        assert valid_call(name, h, b, 0, crc_in=b.crc.ctypes.data) == OK
        assert (b.crc == running).all()


def shape(h, ticket):
    nout, ln, ncrc = ctypes.c_int(-1), ctypes.c_size_t(99), ctypes.c_int(-1)
    st = _lib.lib().hrs_ticket_shape(h, ticket, ctypes.byref(nout), ctypes.byref(ln), ctypes.byref(ncrc))
    return st, (nout.value, ln.value, ncrc.value)


def submit_empty(h, b, name):
    """A zero-length round; returns its ticket."""
    lib = _lib.lib()
    t = ctypes.c_uint64(0)
    if name == "decode_crc":
        st = lib.hrs_decode_submit(h, b.reads, b.erased, len(ERASED), b.to_read, b.nr, b.ntr, b.nn, 0, 1, ctypes.byref(t))
    else:
        st = lib.hrs_encode_submit(h, b.ins, 0, int(name == "encode_crc"), ctypes.byref(t))
    assert st == OK
    return t.value


NO_TICKET = "no uncollected operation with ticket %d"


@pytest.mark.parametrize("name,want", [("encode", (P, 0, 0)), ("encode_crc", (P, 0, N)),
                                       ("decode_crc", (len(ERASED), 0, len(ERASED)))])
def test_zero_length_round(code, name, want):
    lib, h, b = _lib.lib(), code._handle(), Rows(code)
    ms = ctypes.c_float(-1)
    assert lib.hrs_set_timing(h, 1) == OK
    t = submit_empty(h, b, name)
    assert t == 1 and lib.hrs_pending(h) == 1
    assert shape(h, t) == (OK, want)
    assert lib.hrs_ticket_shape(h, t, None, None, None) == OK
    assert lib.hrs_wait(h, t) == OK
    assert lib.hrs_ticket_gpu_ms(h, t, ctypes.byref(ms)) == EINVAL
    assert last_error(code) == f"operation {t} was submitted without timing"
    assert lib.hrs_ticket_gpu_ms(h, t, None) == EINVAL
    assert lib.hrs_collect(h, t, None, b.crc.ctypes.data) == OK  # no outputs to copy: the rows may be NULL
    assert b.untouched() and ms.value == -1
    assert lib.hrs_pending(h) == 0
    assert lib.hrs_collect(h, t, None, b.crc.ctypes.data) == EINVAL
    assert last_error(code) == NO_TICKET % t
    assert submit_empty(h, b, name) == 2  # tickets count on


def test_unknown_ticket(code):
    lib, h, b = _lib.lib(), code._handle(), Rows()
    ms = ctypes.c_float(-1)
    assert lib.hrs_collect(h, 999, b.writes, b.crc.ctypes.data) == EINVAL
    assert last_error(code) == NO_TICKET % 999
    assert lib.hrs_wait(h, 998) == EINVAL
    assert last_error(code) == NO_TICKET % 998
    assert lib.hrs_release(h, 997) == EINVAL
    assert last_error(code) == NO_TICKET % 997
    assert lib.hrs_ticket_gpu_ms(h, 996, ctypes.byref(ms)) == EINVAL
    assert last_error(code) == NO_TICKET % 996
    assert shape(h, 995) == (EINVAL, (-1, 99, -1))
    assert last_error(code) == NO_TICKET % 996  # hrs_ticket_shape sets no message
    assert lib.hrs_collect(h, 0, b.writes, b.crc.ctypes.data) == EINVAL  # ticket 0 is never issued
    assert last_error(code) == NO_TICKET % 0
    assert b.untouched()


def test_four_slots_release_and_collect(code):
    lib, h, b = _lib.lib(), code._handle(), Rows(code)
    tickets = [submit_empty(h, b, "encode") for _ in range(4)]
    assert tickets == [1, 2, 3, 4] and lib.hrs_pending(h) == 4
    t = ctypes.c_uint64(7)
    for _ in range(2):
        assert lib.hrs_encode_submit(h, b.ins, 0, 0, ctypes.byref(t)) == EINVAL
        assert last_error(code) == "all 4 asynchronous slots hold uncollected operations: collect one first"
        assert t.value == 0 and lib.hrs_pending(h) == 4
    assert lib.hrs_release(h, 2) == OK
    assert lib.hrs_pending(h) == 3
    assert lib.hrs_release(h, 2) == EINVAL
    assert last_error(code) == NO_TICKET % 2
    assert submit_empty(h, b, "encode_crc") == 5
    assert shape(h, 5) == (OK, (P, 0, N))
    assert lib.hrs_collect(h, 5, None, None) == EINVAL
    assert last_error(code) == "crc_io is NULL for a checksummed operation"
    assert lib.hrs_pending(h) == 4  # a refused collect keeps the operation
    assert lib.hrs_collect(h, 5, None, b.crc.ctypes.data) == OK
    for tk in (4, 1, 3):  # out of order
        assert lib.hrs_collect(h, tk, None, None) == OK
    assert lib.hrs_pending(h) == 0 and b.untouched()
