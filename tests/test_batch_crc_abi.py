"""CPU tests of the batch + CRC-32 entry points' boundary
(hrs_decode_batch_crc_dev, hrs_decode_batch_host_crc, hrs_encode_batch_host_crc):
exported and declared, and on a host-only handle the argument rules that are
settled before any device is selected: a NULL crc_out with work to do is
HRS_EINVAL, valid arguments are HRS_EDEVICE, an empty batch is HRS_OK."""
import ctypes

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, _lib
from test_abi import declared_symbols

NONE = -2  # HRS_DEVICE_NONE
NAMES = ("hrs_decode_batch_crc_dev", "hrs_decode_batch_host_crc", "hrs_encode_batch_host_crc")
K, P, S, E, L = 10, 4, 3, 2, 4096


def test_symbols_exported_and_declared():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert set(declared_symbols()) == set(_lib.EXPORTS)


def _calls(code, crc_in, crc_out, nstripes=S):
    """The three entry points over one host batch (the _dev form is only ever
    asked for its argument checks here): {name: status}."""
    lib, h = _lib.lib(), code._handle()
    st = np.zeros((S, K + P, L), np.uint8)
    out = np.zeros((S, E, L), np.uint8)
    er = np.array([[0, 5], [3, -1], [-1, -1]], np.int32)
    n = K + P
    dec = (h, st.ctypes.data, L, n * L, er.ctypes.data, E, out.ctypes.data, L, E * L, L, nstripes)
    return {
        "hrs_decode_batch_crc_dev": lib.hrs_decode_batch_crc_dev(*dec, crc_in, crc_out, None),
        "hrs_decode_batch_host_crc": lib.hrs_decode_batch_host_crc(*dec, crc_in, crc_out),
        "hrs_encode_batch_host_crc": lib.hrs_encode_batch_host_crc(h, st.ctypes.data, L, n * L, L, nstripes,
                                                                   crc_in, crc_out),
    }


@pytest.fixture
def code():
    return HipReedSolomonCode(K, P, device=NONE)


def test_null_crc_out_is_einval(code):
    assert _calls(code, None, None) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert b"crc_out" in _lib.lib().hrs_last_error(code._handle())


def test_overlapping_crc_arrays_are_einval(code):
    """crc_out may be crc_in itself; any other overlap is refused, before the
    device is looked at."""
    words = np.zeros(S * (K + P) + 1, np.uint32)
    base = words.ctypes.data
    assert _calls(code, base, base + 4) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert _calls(code, base + 4, base) == dict.fromkeys(NAMES, _lib.HRS_EINVAL)
    assert _calls(code, base, base) == dict.fromkeys(NAMES, _lib.HRS_EDEVICE)  # aliased: valid


def test_valid_arguments_on_host_only_handle_are_edevice(code):
    words = np.zeros(2 * S * (K + P), np.uint32)
    base = words.ctypes.data
    assert _calls(code, None, base) == dict.fromkeys(NAMES, _lib.HRS_EDEVICE)
    assert _calls(code, base + 4 * S * (K + P), base) == dict.fromkeys(NAMES, _lib.HRS_EDEVICE)
    assert not words.any()  # nothing written


def test_empty_batch_is_ok_and_touches_nothing(code):
    words = np.full(S * (K + P), 0xA5A5A5A5, np.uint32)
    assert _calls(code, None, words.ctypes.data, nstripes=0) == dict.fromkeys(NAMES, _lib.HRS_OK)
    assert _calls(code, None, None, nstripes=0) == dict.fromkeys(NAMES, _lib.HRS_OK)
    assert (words == 0xA5A5A5A5).all()


def test_python_mirror_checks_crc_arguments(code):
    """device.py refuses wrong shapes and dtypes before the library is called."""
    from lambdafs_amd import device
    st = np.zeros((S, K + P, L), np.uint8)
    out = np.zeros((S, E, L), np.uint8)
    er = np.full((S, E), -1, np.int32)
    for bad in (np.zeros((S, E + 1), np.uint32), np.zeros((S, E), np.int32), np.zeros((E, S), np.uint32).T):
        with pytest.raises(ValueError):
            device.decode_batch_host_crc(code, st, er, out, crc_in=bad)
        with pytest.raises(ValueError):
            device.decode_batch_host_crc(code, st, er, out, crc_out=bad)
    for bad in (np.zeros((S, K + P - 1), np.uint32), np.zeros((S, K + P), np.int64)):
        with pytest.raises(ValueError):
            device.encode_batch_host_crc(code, st, crc_in=bad)
