"""Expectations and calls shared by the ragged encode + CRC tests
(test_gpu_ragged_crc*.py), on top of ragged_inputs (batches, oracle parity).

Expected CRCs are zlib.crc32 over the zero-filled data cells and over the
oracle's parity rows, continued from crc_in when there is one; layout
[S, k + p]: data rows 0..k-1, then parity rows 0..p-1."""
import zlib

import numpy as np

from lambdafs_amd import _lib
from ragged_inputs import STATIC, vector_kernel, zero_filled

FUSED = "encode_ragged_crc_kernel<%d, %d, hrs::gf::%s<%d, %d>, 1024, 2>"


def fused_kernel(cfg):
    kind, k, p, _ = cfg
    return FUSED % (k, p, "CauchyMatrix" if kind == "nrs" else "EncodeMatrix", k, p)


def route_kernel(cfg, L, mode=0):
    """hrs_last_kernel of a ragged (not all-full) aligned batch: the fused
    kernel for the static shapes on whole 2 KiB windows in modes 0 and 3, else
    the ragged encode's own name."""
    if cfg in STATIC and L % 2048 == 0 and mode in (0, 3):
        return fused_kernel(cfg)
    return vector_kernel(cfg)


def seeded_crc_in(S, n, seed):
    """Non-zero running CRCs [S, n] (uint32)."""
    return np.random.default_rng([77, seed, S, n]).integers(1, 1 << 32, (S, n), dtype=np.uint32)


def expected_crcs(p, stripes, valid, want, crc_in=None):
    """stripes[S, n, L] as given to the call, want = ragged_inputs.expected(...)."""
    S, n, _ = stripes.shape
    z = zero_filled(stripes[:, p:], valid)
    out = np.zeros((S, n), np.uint32)
    for s in range(S):
        rows = [z[s, j] for j in range(n - p)] + [want[s, r] for r in range(p)]
        for r, row in enumerate(rows):
            out[s, r] = zlib.crc32(row.tobytes(), int(crc_in[s, r]) if crc_in is not None else 0)
    return out


def crc_mismatch(got, want, k):
    got, want = np.asarray(got).view(np.uint32).reshape(want.shape), np.asarray(want)
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    s, r = (int(x) for x in bad[0])
    what = "data row %d" % r if r < k else "parity row %d" % (r - k)
    return "%d CRCs differ; first: stripe %d %s: got %#010x, want %#010x" % (len(bad), s, what, int(got[s, r]),
                                                                              int(want[s, r]))


def abi_call_dev(torch, code, t, valid, crc_in, crc_out):
    """hrs_encode_ragged_crc_dev over the device batch t[S, n, L]; crc_in (or
    None) and crc_out are int32 device tensors [S, n]."""
    k, p = code.stripeSize(), code.paritySize()
    S, n, L = t.shape
    ins = _lib.ptr_array([t[:, p + j].data_ptr() for j in range(k)])
    outs = _lib.ptr_array([t[:, r].data_ptr() for r in range(p)])
    v = np.ascontiguousarray(valid, dtype=np.uint32)
    st = _lib.lib().hrs_encode_ragged_crc_dev(code._handle(), ins, n * L, outs, n * L, L, S, v.ctypes.data,
                                              None if crc_in is None else crc_in.data_ptr(), crc_out.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
    v[...] = 0xFFFFFFFF  # the caller's array is free as soon as the call returns
    code._check(st)


def dev_words(torch, a):
    """A uint32 host array as an int32 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to("cuda:0")
