"""CPU tests of the argument rules of lambdafs_amd/device.py, on a host-only
handle: what every host-batch wrapper refuses with ValueError before the
library is called (rank, row count, byte stride, dtype, read-only arrays,
the decode family's erased and out arrays, the CRC arrays), that valid
arguments reach the library (HRS_EDEVICE on this handle), the pre-fill of the
host CRC arrays for empty cells, and that every device wrapper refuses a host
tensor instead of handing its address to a kernel."""
import numpy as np
import pytest
import torch

from lambdafs_amd import HipReedSolomonCode, HrsError, _lib, device

NONE = -2  # HRS_DEVICE_NONE
K, P, S, E, L = 6, 3, 3, 2, 64
N = K + P
ERASED_SE = np.array([[0, 5], [3, -1], [-1, -1]], np.int32)  # the decode family's [S, E]
ERASED_LISTS = [[2], [], [0, 8]]  # the heal-with-erasures form

# name -> (family, writes the stripes, width of its CRC arrays or None)
HOST = {
    "decode_batch_host": ("decode", False, None),
    "decode_batch_host_crc": ("decode", False, E),
    "decode_batch_host_multi": ("decode", False, None),
    "encode_batch_host": ("plain", True, None),
    "encode_batch_host_crc": ("plain", True, N),
    "encode_batch_host_multi": ("plain", True, None),
    "scrub_batch_host": ("plain", False, None),
    "scrub_batch_host_crc": ("plain", False, N),
    "heal_batch_host": ("plain", True, None),
    "heal_batch_host_crc": ("plain", True, N),
    "heal_erased_batch_host": ("erased", True, None),
    "heal_erased_batch_host_crc": ("erased", True, N),
}
DECODE = [name for name, (family, _, _) in HOST.items() if family == "decode"]
WRITERS = [name for name, (_, writes, _) in HOST.items() if writes]
READERS = [name for name in HOST if name not in WRITERS]
WITH_CRC = [name for name, (_, _, width) in HOST.items() if width is not None]


@pytest.fixture(scope="module")
def code():
    return HipReedSolomonCode(K, P, device=NONE)


def stripes_array(length=L):
    # cut from whole cells: numpy gives a new empty array no byte stride
    return np.zeros((S, N, L), np.uint8)[:, :, :length]


def out_array(length=L):
    return np.zeros((S, E, L), np.uint8)[:, :, :length]


def read_only(a):
    a.setflags(write=False)
    return a


def host_call(code, name, stripes, erased=None, out=None, length=L, **crc):
    """The wrapper `name` over `stripes`, its other arguments valid unless given."""
    fn, family = getattr(device, name), HOST[name][0]
    first = [code] if name.endswith("_multi") else code
    if family == "decode":
        return fn(first, stripes, ERASED_SE if erased is None else erased, out_array(length) if out is None else out,
                  **crc)
    if family == "erased":
        return fn(first, stripes, ERASED_LISTS if erased is None else erased, **crc)
    return fn(first, stripes, **crc)


BAD_STRIPES = {
    "rank_2": lambda: np.zeros((S, N * L), np.uint8),
    "rank_4": lambda: np.zeros((S, N, L, 1), np.uint8),
    "one_row_short": lambda: np.zeros((S, N - 1, L), np.uint8),
    "one_row_more": lambda: np.zeros((S, N + 1, L), np.uint8),
    "byte_stride_2": lambda: np.zeros((S, N, 2 * L), np.uint8)[:, :, ::2],
    "int8": lambda: np.zeros((S, N, L), np.int8),
    "uint16": lambda: np.zeros((S, N, L), np.uint16),
    "int8_tensor": lambda: torch.zeros((S, N, L), dtype=torch.int8),
    "byte_stride_2_tensor": lambda: torch.zeros((S, N, 2 * L), dtype=torch.uint8)[:, :, ::2],
}


@pytest.mark.parametrize("bad", list(BAD_STRIPES))
@pytest.mark.parametrize("name", list(HOST))
def test_host_wrappers_refuse_bad_stripes(code, name, bad):
    with pytest.raises(ValueError):
        host_call(code, name, BAD_STRIPES[bad]())


@pytest.mark.parametrize("name", WRITERS)
def test_host_wrappers_that_write_refuse_read_only_stripes(code, name):
    with pytest.raises(ValueError):
        host_call(code, name, read_only(stripes_array()))


def expect_edevice(call):
    with pytest.raises(HrsError) as err:
        call()
    assert err.value.status == _lib.HRS_EDEVICE


@pytest.mark.parametrize("name", list(HOST))
def test_valid_host_arguments_reach_the_library(code, name):
    """HRS_EDEVICE is the library's answer on a host-only handle, given after
    its own argument checks: numpy arrays, CPU tensors, and cells that are
    strided but whole."""
    expect_edevice(lambda: host_call(code, name, stripes_array()))
    expect_edevice(lambda: host_call(code, name, torch.zeros((S, N, L), dtype=torch.uint8)))
    expect_edevice(lambda: host_call(code, name, np.zeros((S, N + 1, L + 8), np.uint8)[:, :N, :L]))
    if HOST[name][0] == "decode":
        expect_edevice(lambda: host_call(code, name, stripes_array(), out=torch.zeros((S, E, L), dtype=torch.uint8)))
        wide = np.zeros((S, E + 1, L + 8), np.uint8)
        expect_edevice(lambda: host_call(code, name, stripes_array(), out=wide[:, :E, :L]))
        expect_edevice(lambda: host_call(code, name, stripes_array(), erased=ERASED_SE.tolist()))


@pytest.mark.parametrize("name", READERS)
def test_host_wrappers_that_only_read_take_read_only_stripes(code, name):
    expect_edevice(lambda: host_call(code, name, read_only(stripes_array())))


BAD_ERASED = {
    "one_row_more": np.full((S + 1, E), -1, np.int32),
    "one_row_short": np.full((S - 1, E), -1, np.int32),
    "rank_1": np.full(S * E, -1, np.int32),
    "rank_3": np.full((S, E, 1), -1, np.int32),
}
BAD_OUT = {
    "one_cell_more": lambda: np.zeros((S, E + 1, L), np.uint8),
    "one_stripe_more": lambda: np.zeros((S + 1, E, L), np.uint8),
    "one_byte_more": lambda: np.zeros((S, E, L + 1), np.uint8),
    "rank_2": lambda: np.zeros((S, E * L), np.uint8),
    "byte_stride_2": lambda: np.zeros((S, E, 2 * L), np.uint8)[:, :, ::2],
    "int8": lambda: np.zeros((S, E, L), np.int8),
    "read_only": lambda: read_only(out_array()),
    "int8_tensor": lambda: torch.zeros((S, E, L), dtype=torch.int8),
}


@pytest.mark.parametrize("bad", list(BAD_ERASED))
@pytest.mark.parametrize("name", DECODE)
def test_host_decode_refuses_bad_erased(code, name, bad):
    with pytest.raises(ValueError):
        host_call(code, name, stripes_array(), erased=BAD_ERASED[bad])


@pytest.mark.parametrize("bad", list(BAD_OUT))
@pytest.mark.parametrize("name", DECODE)
def test_host_decode_refuses_bad_out(code, name, bad):
    with pytest.raises(ValueError):
        host_call(code, name, stripes_array(), out=BAD_OUT[bad]())


def bad_crcs(width):
    return {
        "one_column_more": np.zeros((S, width + 1), np.uint32),
        "one_row_more": np.zeros((S + 1, width), np.uint32),
        "flat": np.zeros(S * width, np.uint32),
        "int32": np.zeros((S, width), np.int32),
        "int64": np.zeros((S, width), np.int64),
        "transposed": np.zeros((width, S), np.uint32).T,
        "a_list": np.zeros((S, width), np.uint32).tolist(),
    }


@pytest.mark.parametrize("bad", list(bad_crcs(1)))
@pytest.mark.parametrize("name", WITH_CRC)
def test_host_wrappers_refuse_bad_crc_arrays(code, name, bad):
    arr = bad_crcs(HOST[name][2])[bad]
    with pytest.raises(ValueError):
        host_call(code, name, stripes_array(), crc_in=arr)
    with pytest.raises(ValueError):
        host_call(code, name, stripes_array(), crc_out=arr)


@pytest.mark.parametrize("name", WITH_CRC)
def test_host_crc_out_must_be_writable_and_crc_in_need_not_be(code, name):
    width = HOST[name][2]
    with pytest.raises(ValueError):
        host_call(code, name, stripes_array(), crc_out=read_only(np.zeros((S, width), np.uint32)))
    crcs = np.zeros((S, width), np.uint32)
    expect_edevice(lambda: host_call(code, name, stripes_array(), crc_in=read_only(np.zeros((S, width), np.uint32)),
                                     crc_out=crcs))
    expect_edevice(lambda: host_call(code, name, stripes_array(), crc_in=crcs, crc_out=crcs))  # aliased: valid
    assert not crcs.any()  # nothing written


@pytest.mark.parametrize("name", WITH_CRC)
def test_host_crcs_of_empty_cells_continue_over_no_bytes(code, name):
    """L == 0: the library has nothing to do and says HRS_OK; the wrapper's
    CRCs are zeros without crc_in, crc_in's values with it, and a crc_out that
    is crc_in itself is left as it is."""
    width = HOST[name][2]
    empty = stripes_array(0)
    start = np.random.default_rng(width).integers(1, 1 << 32, (S, width), dtype=np.uint32)

    def crcs_of(result):
        return result[1] if isinstance(result, tuple) else result  # the scrubs and heals return (reports, crcs)

    got = crcs_of(host_call(code, name, empty, length=0))
    assert got.dtype == np.uint32 and got.shape == (S, width) and not got.any()
    got = crcs_of(host_call(code, name, empty, length=0, crc_in=start))
    assert got is not start and (got == start).all()
    mine = np.full((S, width), 0xA5A5A5A5, np.uint32)
    assert crcs_of(host_call(code, name, empty, length=0, crc_out=mine)) is mine and not mine.any()
    mine[...] = 0xA5A5A5A5
    assert crcs_of(host_call(code, name, empty, length=0, crc_in=start, crc_out=mine)) is mine and (mine == start).all()
    alias = start.copy()
    assert crcs_of(host_call(code, name, empty, length=0, crc_in=alias, crc_out=alias)) is alias
    assert (alias == start).all()


# ---------------------------------------------------------- device wrappers

def _stripes(length=L):
    return torch.zeros((S, N, length), dtype=torch.uint8)


def _views(t=None):
    t = _stripes() if t is None else t
    return [t[:, l] for l in range(N)]


def _stored():
    return torch.zeros((S, N), dtype=torch.int32)


def _out():
    return torch.zeros((S, E, L), dtype=torch.uint8)


# every wrapper that hands addresses to a kernel, over CPU tensors of the right shapes and dtypes
DEVICE = {
    "encode_stripes": lambda c: device.encode_stripes(c, _stripes()),
    "encode_stripes_crc": lambda c: device.encode_stripes_crc(c, _stripes()),
    "encode_rows": lambda c: device.encode_rows(c, _views()[P:], _views()[:P]),
    "decode_stripes": lambda c: device.decode_stripes(c, _stripes(), [0, 5], [1], _out()),
    "decode_stripes_crc": lambda c: device.decode_stripes_crc(c, _stripes(), [0, 5], [1], _out()),
    "decode_batch": lambda c: device.decode_batch(c, _stripes(), ERASED_SE, _out()),  # differs at the parent
    "decode_batch_crc": lambda c: device.decode_batch_crc(c, _stripes(), ERASED_SE, _out()),  # differs at the parent
    "apply_rows": lambda c: device.apply_rows(c, np.ones((P, K), np.uint8), _views()[P:], _views()[:P]),
    "crc32_rows": lambda c: device.crc32_rows(c, _views()),
    "scrub_stripes": lambda c: device.scrub_stripes(c, _stripes()),
    "scrub_rows": lambda c: device.scrub_rows(c, _views()),
    "scrub_stripes_crc": lambda c: device.scrub_stripes_crc(c, _stripes()),
    "scrub_rows_crc": lambda c: device.scrub_rows_crc(c, _views()),
    "heal_stripes": lambda c: device.heal_stripes(c, _stripes()),
    "heal_rows": lambda c: device.heal_rows(c, _views()),
    "heal_stripes_crc": lambda c: device.heal_stripes_crc(c, _stripes()),
    "heal_rows_crc": lambda c: device.heal_rows_crc(c, _views()),
    "heal_erased_stripes": lambda c: device.heal_erased_stripes(c, _stripes(), ERASED_LISTS),
    "heal_erased_rows": lambda c: device.heal_erased_rows(c, _views(), ERASED_LISTS),
    "heal_erased_stripes_crc": lambda c: device.heal_erased_stripes_crc(c, _stripes(), ERASED_LISTS),
    "heal_erased_rows_crc": lambda c: device.heal_erased_rows_crc(c, _views(), ERASED_LISTS),
    "repair_checked_stripes": lambda c: device.repair_checked_stripes(c, _stripes(), _stored()),
    "repair_checked_rows": lambda c: device.repair_checked_rows(c, _views(), _stored()),
}


@pytest.mark.parametrize("name", list(DEVICE))
def test_device_wrappers_refuse_host_tensors(code, name):
    """A CPU tensor is a ValueError, never an address passed on. (decode_batch
    and decode_batch_crc are the two that did pass it on before they took
    _stripe_rows' rule.)"""
    with pytest.raises(ValueError):
        DEVICE[name](code)


def test_device_decode_batch_refuses_a_host_out_and_bad_shapes(code):
    """The rest of decode_batch's rules that need no device to be judged."""
    for call in (device.decode_batch, device.decode_batch_crc):
        with pytest.raises(ValueError):
            call(code, torch.zeros((S, N - 1, L), dtype=torch.uint8), ERASED_SE, _out())
        with pytest.raises(ValueError):
            call(code, torch.zeros((S, N * L), dtype=torch.uint8), ERASED_SE, _out())
