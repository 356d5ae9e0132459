"""Device-resident stripe batches on MI355X (the hot path of bench.py).

HBM layout: a batch of S stripes is one uint8 tensor `stripes[S, n, L]` in
hops location order — rows [0, p) parity, [p, p+k) data — i.e. exactly the
`data` array ReedSolomonCode.encodeBulk assembles per call
(ReedSolomonCode.java:114-121), with S stripes stacked. A row view
`stripes[:, loc, :]` is handed to libhrs as (pointer of stripe 0, stride n*L).
Decode outputs go to a separate `out[S, e, L]` tensor.

All calls are asynchronous on the current torch stream of the tensors' device.

Every argument rule is stated once, in the helpers of the first section; a
family of library calls that share a signature has one private body, which
takes `crcs`: None for the call without CRCs, else its (crc_in[, crc_out]).
"""
import numpy as np

from . import _lib
from ._lib import int_array, ptr_array


# ---- device arguments

def _rows(views):
    """[S, L] row views -> (pointer array, stride bytes, L, S)."""
    if not views:
        raise ValueError("no rows")
    strides, shapes = set(), set()
    for v in views:
        if v is None:
            continue
        if v.dtype != _lib.torch.uint8 or v.dim() != 2 or v.stride(1) != 1 or not v.is_cuda:
            raise ValueError("row views must be [S, L] uint8 device tensors with unit byte stride")
        strides.add(v.stride(0) if v.shape[0] > 1 else None)
        shapes.add(tuple(v.shape))
    if len(shapes) != 1:
        raise ValueError("row views differ in shape")
    strides.discard(None)
    if len(strides) > 1:
        raise ValueError("row views differ in stripe stride")
    S, L = shapes.pop()
    stride = strides.pop() if strides else L
    ptrs = ptr_array([None if v is None else v.data_ptr() for v in views])
    return ptrs, stride, L, S


def _stripe_rows(t, locs, n=None):
    """Rows `locs` (None = not passed) of a [S, m, L] uint8 device tensor ->
    (pointer array, stride bytes, L, S), the same as _rows over the views
    t[:, loc, :] but computed from t's own pointer and strides: building m
    tensor views costs ~3 us each in Python, more than a small launch. With n,
    t is a batch of a code with n locations and must be [S, n, L]."""
    torch = _lib.torch
    if t.dtype != torch.uint8 or t.dim() != 3 or t.stride(2) != 1 or not t.is_cuda:
        raise ValueError("stripes must be a [S, m, L] uint8 device tensor with unit byte stride")
    S, m, L = t.shape
    if n is not None and m != n:
        raise ValueError(f"stripes must be [S, {n}, L]")
    if locs is None:  # decode_batch: the library takes t's own pointer and both strides
        return None, None, L, S
    base, s_stripe, s_row = t.data_ptr(), t.stride(0), t.stride(1)
    for loc in locs:
        if loc is not None and not 0 <= loc < m:
            raise ValueError(f"row {loc} outside [0, {m})")
    ptrs = ptr_array([None if loc is None else base + loc * s_row for loc in locs])
    return ptrs, (s_stripe if S > 1 else L), L, S


def _code_stripes(code, stripes):
    """A device batch stripes[S, n, L] of this code -> (pointer array of its n
    rows, stride bytes, L, S, stripes): _stripe_rows' tuple and the tensor
    whose device and stream the call uses."""
    n = code.stripeSize() + code.paritySize()
    return (*_stripe_rows(stripes, range(n), n), stripes)


def _code_rows(code, row_views):
    """The same batch as n explicit [S, L] row views, one per location in hops
    order -> _code_stripes' tuple, the first view standing for the tensor."""
    n = code.stripeSize() + code.paritySize()
    if len(row_views) != n or any(v is None for v in row_views):
        raise ValueError(f"need {n} row views")
    return (*_rows(row_views), row_views[0])


def _stream(t):
    return _lib.torch.cuda.current_stream(t.device).cuda_stream


# A device batch without bytes (L == 0 or S == 0) is answered here, not by the
# library: torch gives a tensor without elements a null data_ptr(), which the
# scrub, heal and decode entry points refuse as a NULL row. Such a call has
# nothing to do, so the bodies below skip it (`if L and S`); _dev_crcs has
# filled its CRCs and _dev_reports its reports.


def _dev_crcs(shape, ref, L, S, crc_in, crc_out=None):
    """(crc_in pointer or None, the int32 result tensor) of a device call over
    S stripes of L-byte cells on ref's device; _host_crcs' counterpart."""
    torch = _lib.torch
    for name, t in (("crc_in", crc_in), ("crc_out", crc_out)):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.int32
                              or not t.is_contiguous() or t.device != ref.device):
            raise ValueError(f"{name} must be a contiguous int32 tensor [S, {shape[1]}] on the stripes' device")
    crc = crc_out if crc_out is not None else torch.empty(shape, dtype=torch.int32, device=ref.device)
    if (L == 0 or S == 0) and crc is not crc_in:  # the call touches nothing: every CRC continues over no bytes
        crc.zero_() if crc_in is None else crc.copy_(crc_in)
    return (None if crc_in is None else crc_in.data_ptr()), crc


def _decode_erased(erased, S):
    """The decode family's erasure lists as a contiguous host int32 [S, E] array."""
    e = np.ascontiguousarray(np.asarray(erased, dtype=np.int32))
    if e.ndim != 2 or e.shape[0] != S:
        raise ValueError("erased must be [S, E]")
    return e


# ---- host arguments

def _host_crcs(shape, L, crc_in, crc_out):
    """(crc_in pointer or None, the uint32 result array) of a host batch of L-byte cells."""
    for name, a in (("crc_in", crc_in), ("crc_out", crc_out)):
        if a is not None and (not isinstance(a, np.ndarray) or a.dtype != np.uint32 or a.shape != shape
                              or not a.flags["C_CONTIGUOUS"]):
            raise ValueError(f"{name} must be a C-contiguous uint32 array {list(shape)}")
    if crc_out is not None and not crc_out.flags["WRITEABLE"]:
        raise ValueError("crc_out must be writable")
    crc = crc_out if crc_out is not None else np.empty(shape, dtype=np.uint32)
    if L == 0 and crc is not crc_in:  # the call touches nothing: every CRC continues over no bytes
        crc[...] = 0 if crc_in is None else crc_in
    return (None if crc_in is None else crc_in.ctypes.data), crc


def _host_ptr(a, name, writable=False):
    """Base address of a host batch (numpy array or CPU tensor, pinned or not)."""
    torch = _lib.torch
    if torch is not None and isinstance(a, torch.Tensor):
        if a.is_cuda or a.dtype != torch.uint8:
            raise ValueError(f"{name} must be a host uint8 tensor")
        return a.data_ptr(), tuple(a.shape), tuple(a.stride())
    a = np.asarray(a)
    if a.dtype != np.uint8 or (writable and not a.flags["WRITEABLE"]):
        raise ValueError(f"{name} must be a {'writable ' if writable else ''}uint8 array")
    return a.ctypes.data, a.shape, tuple(x // a.itemsize for x in a.strides)


def _host_batch(code, stripes, writable=False):
    """A host batch stripes[S, n, L] of this code -> (pointer, row stride,
    stripe stride, L, S), the order the library's host-batch calls take them in."""
    n = code.stripeSize() + code.paritySize()
    sp, sshape, sstr = _host_ptr(stripes, "stripes", writable)
    if len(sshape) != 3 or sshape[1] != n or sstr[2] != 1:
        raise ValueError(f"stripes must be [S, {n}, L] with unit byte stride")
    return sp, sstr[1], sstr[0], sshape[2], sshape[0]


def _host_out(out, S, E, L):
    """The decode family's host out[S, E, L] -> (pointer, row stride, stripe stride)."""
    op, oshape, ostr = _host_ptr(out, "out", writable=True)
    if len(oshape) != 3 or tuple(oshape) != (S, E, L) or ostr[2] != 1:
        raise ValueError("out must be [S, E, L]")
    return op, ostr[1], ostr[0]


def _codec_array(codes):
    codes = list(codes)
    if not codes:
        raise ValueError("a device set needs at least one codec")
    return codes, ptr_array([c._handle().value for c in codes])


# ---- encode and decode on the device

def _encode_stripes(code, stripes, crcs=None):
    k, p = code.stripeSize(), code.paritySize()
    ins, s_in, L, S = _stripe_rows(stripes, range(p, p + k), k + p)
    outs, s_out, _, _ = _stripe_rows(stripes, range(p))
    args = (code._handle(), ins, s_in, outs, s_out, L, S)
    if crcs is None:
        code._check(_lib.lib().hrs_encode_dev(*args, _stream(stripes)))
        return None
    cin, crc = _dev_crcs((S, k + p), stripes, L, S, *crcs)
    code._check(_lib.lib().hrs_encode_crc_dev(*args, cin, crc.data_ptr(), _stream(stripes)))
    return crc


def encode_stripes(code, stripes):
    """Parity rows of every stripe from its data rows (encodeBulk over S stripes)."""
    _encode_stripes(code, stripes)


def encode_stripes_crc(code, stripes, crc_in=None):
    """Encode every stripe and return the CRC-32 (java.util.zip.CRC32) of its
    cells in one pass, as Encoder.encodeStripe keeps them with
    computeBlockChecksum (Encoder.java:408-450): an int32 tensor [S, k + p],
    columns [source 0..k-1, parity 0..p-1] holding the uint32 CRC bits.
    crc_in ([S, k + p] int32, same layout) continues running CRCs across
    successive cells (CRC32.update chaining)."""
    return _encode_stripes(code, stripes, (crc_in,))


def encode_rows(code, data_rows, parity_rows):
    """encodeBulk with explicit [S, L] row views (k data, p parity)."""
    ins, s_in, L, S = _rows(data_rows)
    outs, s_out, L2, S2 = _rows(parity_rows)
    if (L, S) != (L2, S2):
        raise ValueError("data and parity views differ in shape")
    code._check(_lib.lib().hrs_encode_dev(code._handle(), ins, s_in, outs, s_out, L, S, _stream(data_rows[0])))


def _ragged_valid(code, valid, S, cells=None):
    """The ragged calls' valid lengths as a C-contiguous host uint32 [S, cells]
    array (cells: k, the encodes' data cells, unless given)."""
    cells = code.stripeSize() if cells is None else cells
    torch = _lib.torch
    if torch is not None and isinstance(valid, torch.Tensor):
        valid = valid.cpu().numpy()
    v = np.ascontiguousarray(np.asarray(valid), dtype=np.uint32)
    if v.shape != (S, cells):
        raise ValueError(f"valid must be [S, {cells}]")
    return v


def encode_stripes_ragged(code, stripes, valid):
    """encode_stripes over data cells of which only the leading valid[s, j]
    bytes hold data (hrs_encode_ragged_dev): cell j of stripe s (location
    p + j) counts as those bytes followed by zeros, the buffer
    RaidUtils.readTillEnd hands encodeBulk, and whatever lies behind them is
    never used; windows wholly behind them are not read. valid: anything
    convertible to a uint32 [S, k] array (ReadResult.numRead per stripe); it
    may be reused as soon as the call returns."""
    k, p = code.stripeSize(), code.paritySize()
    ins, s_in, L, S = _stripe_rows(stripes, range(p, p + k), k + p)
    outs, s_out, _, _ = _stripe_rows(stripes, range(p))
    v = _ragged_valid(code, valid, S)
    if L and S:
        code._check(_lib.lib().hrs_encode_ragged_dev(code._handle(), ins, s_in, outs, s_out, L, S, v.ctypes.data,
                                                     _stream(stripes)))


def encode_stripes_ragged_crc(code, stripes, valid, crc_in=None):
    """encode_stripes_ragged plus the CRC-32 of every cell from the same pass
    (hrs_encode_ragged_crc_dev), as Encoder.encodeStripe keeps them with
    computeBlockChecksum: an int32 tensor [S, k + p], columns [source 0..k-1,
    parity 0..p-1]. A source's CRC covers its valid bytes followed by
    L - valid zeros, the zero-filled buffer updateChecksums sees; nothing at or
    beyond valid is read. crc_in ([S, k + p] int32) continues running CRCs."""
    k, p = code.stripeSize(), code.paritySize()
    ins, s_in, L, S = _stripe_rows(stripes, range(p, p + k), k + p)
    outs, s_out, _, _ = _stripe_rows(stripes, range(p))
    v = _ragged_valid(code, valid, S)
    cin, crc = _dev_crcs((S, k + p), stripes, L, S, crc_in)
    if L and S:
        code._check(_lib.lib().hrs_encode_ragged_crc_dev(code._handle(), ins, s_in, outs, s_out, L, S, v.ctypes.data,
                                                         cin, crc.data_ptr(), _stream(stripes)))
    return crc


def _decode_stripes(code, stripes, erased, not_to_read, out, crcs=None):
    n = code.stripeSize() + code.paritySize()
    ntr = set(not_to_read)
    rows, s_in, L, S = _stripe_rows(stripes, [None if loc in ntr else loc for loc in range(n)], n)
    outs, s_out, L2, S2 = _stripe_rows(out, range(len(erased)))
    if (L, S) != (L2, S2):
        raise ValueError("out must be [S, e, L]")
    args = (code._handle(), rows, s_in, outs, s_out, int_array(erased), len(erased), int_array(not_to_read),
            len(not_to_read), L, S)
    if crcs is None:
        if L and S:
            code._check(_lib.lib().hrs_decode_dev(*args, _stream(stripes)))
        return None
    cin, crc = _dev_crcs((S, len(erased)), stripes, L, S, *crcs)
    if L and S:
        code._check(_lib.lib().hrs_decode_crc_dev(*args, cin, crc.data_ptr(), _stream(stripes)))
    return crc


def decode_stripes(code, stripes, erased, not_to_read, out):
    """decodeBulk 5-arg over S stripes: out[S, e, L] <- the erased locations.
    Rows of `stripes` at not_to_read locations are never read."""
    _decode_stripes(code, stripes, erased, not_to_read, out)


def decode_stripes_crc(code, stripes, erased, not_to_read, out, crc_in=None):
    """decode_stripes plus the CRC-32 (java.util.zip.CRC32) of every repaired
    cell in one pass, as the Decoder checks a repaired block against the
    NameNode's checksum (Decoder.java:222-229, :645-655): returns an int32
    tensor [S, e] of the uint32 CRC bits; crc_in (same layout) continues
    running CRCs across successive cells."""
    return _decode_stripes(code, stripes, erased, not_to_read, out, (crc_in,))


def _decode_batch(code, stripes, erased, out, crcs=None, valid=None):
    n = code.stripeSize() + code.paritySize()
    _, _, L, S = _stripe_rows(stripes, None, n)
    e = _decode_erased(erased, S)
    if (out.dim() != 3 or tuple(out.shape) != (S, e.shape[1], L) or out.stride(2) != 1
            or out.dtype != _lib.torch.uint8 or out.device != stripes.device):
        raise ValueError("out must be [S, E, L] on the stripes' device")
    args = (code._handle(), stripes.data_ptr(), stripes.stride(1), stripes.stride(0), e.ctypes.data, e.shape[1],
            out.data_ptr(), out.stride(1), out.stride(0), L, S)
    if valid is not None:
        v = _ragged_valid(code, valid, S, n)
        if crcs is None:
            if L and S:
                code._check(_lib.lib().hrs_decode_batch_ragged_dev(*args, v.ctypes.data, _stream(stripes)))
            return None
        cin, crc = _dev_crcs((S, e.shape[1]), stripes, L, S, *crcs)
        if L and S:
            code._check(_lib.lib().hrs_decode_batch_ragged_crc_dev(*args, v.ctypes.data, cin, crc.data_ptr(),
                                                                   _stream(stripes)))
        return crc
    if crcs is None:
        if L and S:
            code._check(_lib.lib().hrs_decode_batch_dev(*args, _stream(stripes)))
        return None
    cin, crc = _dev_crcs((S, e.shape[1]), stripes, L, S, *crcs)
    if L and S:
        code._check(_lib.lib().hrs_decode_batch_crc_dev(*args, cin, crc.data_ptr(), _stream(stripes)))
    return crc


def decode_batch(code, stripes, erased, out):
    """Repair every stripe of stripes[S, n, L] from its own erasure list, in one
    launch (hrs_decode_batch_dev): erased is an int array [S, E] of hops
    locations (ascending per stripe, -1 padded; a row of -1 = nothing lost);
    out[S, E, L] receives stripe s's repaired rows in that order. Survivors are
    the ones locationsToReadForDecode picks, as Decoder.fixErasedBlockImpl does."""
    _decode_batch(code, stripes, erased, out)


def decode_batch_crc(code, stripes, erased, out, crc_in=None, crc_out=None):
    """decode_batch plus the CRC-32 (java.util.zip.CRC32) of every repaired cell
    in one pass (hrs_decode_batch_crc_dev): returns an int32 tensor [S, E] of
    the uint32 CRC bits, entry [s, t] for output t of stripe s. crc_in (same
    layout) continues running CRCs across successive cells; an entry past its
    stripe's losses continues over no bytes and keeps its crc_in value (0
    without crc_in). crc_out: the tensor to fill and return (it may be crc_in
    itself) instead of a new one."""
    return _decode_batch(code, stripes, erased, out, (crc_in, crc_out))


def decode_batch_ragged(code, stripes, erased, out, valid):
    """decode_batch over cells of which only the leading valid[s, l] bytes hold
    data (hrs_decode_batch_ragged_dev): a survivor counts as those bytes
    followed by zeros, the buffer RaidUtils.readTillEnd hands decodeBulk, and
    nothing behind them is read; output t of stripe s receives exactly the
    first valid[s, erased[s, t]] bytes of the rebuilt cell and keeps the rest
    of out[s, t] as it was. valid: anything convertible to a uint32 [S, n]
    array in hops order; it may be reused as soon as the call returns."""
    _decode_batch(code, stripes, erased, out, valid=valid)


def decode_batch_ragged_crc(code, stripes, erased, out, valid, crc_in=None, crc_out=None):
    """decode_batch_ragged plus the CRC-32 of every rebuilt cell from the same
    pass (hrs_decode_batch_ragged_crc_dev), as Decoder.fixErasedBlockImpl takes
    it: entry [s, t] of the returned int32 tensor [S, E] is the CRC of exactly
    the first valid[s, erased[s, t]] bytes of output t of stripe s, with no
    zeros behind them, continued from crc_in[s, t]. An entry of length 0 or
    past its stripe's losses keeps its crc_in value (0 without crc_in).
    crc_out: the tensor to fill and return (it may be crc_in itself)."""
    return _decode_batch(code, stripes, erased, out, (crc_in, crc_out), valid=valid)


# ---- encode and decode over host batches

def _decode_batch_host(code, head, call, stripes, erased, out, crcs=None, valid=None):
    """The library's `call` over a host batch; `head` is its leading handle
    argument, or a device set's handle array and count with `code` its first
    codec. valid: the ragged call's lengths, its last argument."""
    sp, row_stride, stripe_stride, L, S = _host_batch(code, stripes)
    e = _decode_erased(erased, S)
    args = (*head, sp, row_stride, stripe_stride, e.ctypes.data, e.shape[1], *_host_out(out, S, e.shape[1], L), L, S)
    if valid is not None:
        v = _ragged_valid(code, valid, S, code.stripeSize() + code.paritySize())
        if crcs is None:
            code._check(call(*args, v.ctypes.data))
            return None
        cin, crc = _host_crcs((S, e.shape[1]), L, *crcs)
        code._check(call(*args, v.ctypes.data, cin, crc.ctypes.data))
        return crc
    if crcs is None:
        code._check(call(*args))
        return None
    cin, crc = _host_crcs((S, e.shape[1]), L, *crcs)
    code._check(call(*args, cin, crc.ctypes.data))
    return crc


def _encode_batch_host(code, head, call, stripes, crcs=None):
    """As _decode_batch_host; the stripes are written in place."""
    sp, row_stride, stripe_stride, L, S = _host_batch(code, stripes, writable=True)
    args = (*head, sp, row_stride, stripe_stride, L, S)
    if crcs is None:
        code._check(call(*args))
        return None
    cin, crc = _host_crcs((S, code.stripeSize() + code.paritySize()), L, *crcs)
    code._check(call(*args, cin, crc.ctypes.data))
    return crc


def decode_batch_host(code, stripes, erased, out):
    """hrs_decode_batch_host: decode_batch for stripes[S, n, L] and out[S, E, L]
    in HOST memory (numpy arrays or CPU tensors; pinned ones are DMA'd
    directly). Only each stripe's survivors go over PCIe, only the repaired
    cells come back; chunks of stripes pipeline through the device."""
    _decode_batch_host(code, (code._handle(),), _lib.lib().hrs_decode_batch_host, stripes, erased, out)


def decode_batch_host_ragged(code, stripes, erased, out, valid):
    """hrs_decode_batch_ragged_host: decode_batch_host with decode_batch_ragged's
    valid lengths ([S, n], hops order). Pinned batches are repaired in place and
    dead windows never cross the host link; of any other memory only the valid
    bytes of each survivor are copied in and only the valid bytes of each
    repaired cell are copied back."""
    _decode_batch_host(code, (code._handle(),), _lib.lib().hrs_decode_batch_ragged_host, stripes, erased, out,
                       valid=valid)


def decode_batch_host_ragged_crc(code, stripes, erased, out, valid, crc_in=None, crc_out=None):
    """hrs_decode_batch_ragged_host_crc: decode_batch_host_ragged plus
    decode_batch_ragged_crc's CRCs, as a uint32 numpy array [S, E] (crc_in and
    crc_out: such arrays; crc_out may be crc_in itself)."""
    return _decode_batch_host(code, (code._handle(),), _lib.lib().hrs_decode_batch_ragged_host_crc, stripes, erased,
                              out, (crc_in, crc_out), valid=valid)


def encode_batch_host(code, stripes):
    """hrs_encode_batch_host: parity rows of every stripe of a HOST batch
    stripes[S, n, L] (hops order) from its data rows, in place."""
    _encode_batch_host(code, (code._handle(),), _lib.lib().hrs_encode_batch_host, stripes)


def encode_batch_host_ragged(code, stripes, valid):
    """hrs_encode_ragged_batch_host: encode_batch_host with encode_stripes_ragged's
    valid lengths. Pinned stripes are encoded in place and dead windows never
    cross the host link; of any other memory only the valid bytes of each data
    cell are copied in."""
    sp, row_stride, stripe_stride, L, S = _host_batch(code, stripes, writable=True)
    v = _ragged_valid(code, valid, S)
    code._check(_lib.lib().hrs_encode_ragged_batch_host(code._handle(), sp, row_stride, stripe_stride, L, S,
                                                        v.ctypes.data))


def encode_batch_host_ragged_crc(code, stripes, valid, crc_in=None, crc_out=None):
    """hrs_encode_ragged_batch_host_crc: encode_batch_host_ragged plus the
    CRC-32 of every cell, computed on the GPU in the same pass: returns a numpy
    uint32 array [S, k + p] laid out as encode_stripes_ragged_crc's. crc_in
    continues running CRCs; crc_out: the array to fill and return (it may be
    crc_in itself) instead of a new one."""
    sp, row_stride, stripe_stride, L, S = _host_batch(code, stripes, writable=True)
    v = _ragged_valid(code, valid, S)
    cin, crc = _host_crcs((S, code.stripeSize() + code.paritySize()), L, crc_in, crc_out)
    code._check(_lib.lib().hrs_encode_ragged_batch_host_crc(code._handle(), sp, row_stride, stripe_stride, L, S,
                                                            v.ctypes.data, cin, crc.ctypes.data))
    return crc


def decode_batch_host_crc(code, stripes, erased, out, crc_in=None, crc_out=None):
    """hrs_decode_batch_host_crc: decode_batch_host plus the CRC-32 of every
    repaired cell, computed on the GPU in the same pass: returns a numpy uint32
    array [S, E] (entry [s, t] for output t of stripe s; entries past a
    stripe's losses keep their crc_in value, 0 without crc_in). crc_in (uint32
    [S, E]) continues running CRCs; crc_out: the array to fill and return (it
    may be crc_in itself) instead of a new one."""
    return _decode_batch_host(code, (code._handle(),), _lib.lib().hrs_decode_batch_host_crc, stripes, erased, out,
                              (crc_in, crc_out))


def encode_batch_host_crc(code, stripes, crc_in=None, crc_out=None):
    """hrs_encode_batch_host_crc: encode_batch_host plus the CRC-32 of every
    cell, as Encoder.encodeStripe keeps them with computeBlockChecksum: returns
    a numpy uint32 array [S, k + p], columns [source 0..k-1, parity 0..p-1]
    (encode_stripes_crc's order). crc_in (same layout) continues running CRCs;
    crc_out: the array to fill and return (it may be crc_in itself)."""
    return _encode_batch_host(code, (code._handle(),), _lib.lib().hrs_encode_batch_host_crc, stripes,
                              (crc_in, crc_out))


def decode_batch_host_multi(codes, stripes, erased, out):
    """hrs_decode_batch_host_multi: decode_batch_host over a device set. `codes`
    are distinct codecs of one code, each on the device it should use; the
    stripes split into len(codes) contiguous ranges, one per codec, run on
    their own host threads (one host link per device)."""
    codes, arr = _codec_array(codes)
    _decode_batch_host(codes[0], (arr, len(codes)), _lib.lib().hrs_decode_batch_host_multi, stripes, erased, out)


def encode_batch_host_multi(codes, stripes):
    """hrs_encode_batch_host_multi: encode_batch_host over a device set
    (contiguous stripe ranges, one per codec, each on its own host thread)."""
    codes, arr = _codec_array(codes)
    _encode_batch_host(codes[0], (arr, len(codes)), _lib.lib().hrs_encode_batch_host_multi, stripes)


def apply_rows(code, matrix, in_rows, out_rows):
    """out_o = XOR_i matrix[o, i] * in_i over S stripes (matrix: host uint8 [nout, nin]).
    Used with coding matrices broadcast over RCCL (bench.py --gpus N). An input
    whose matrix column is all zero is never read and may be passed as None."""
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.uint8))
    ins, s_in, L, S = _rows(in_rows)
    outs, s_out, L2, S2 = _rows(out_rows)
    if m.shape != (len(out_rows), len(in_rows)) or (L, S) != (L2, S2):
        raise ValueError("shape mismatch")
    ref = next(v for v in in_rows if v is not None)
    code._check(_lib.lib().hrs_apply_dev(code._handle(), m.ctypes.data, m.shape[0], m.shape[1], ins, s_in, outs,
                                         s_out, L, S, _stream(ref)))


def crc32_rows(code, row_views, crc_in=None):
    """CRC-32 (java.util.zip.CRC32) of every [S, L] row view, per stripe:
    returns an int32 tensor [S, nrows] holding the uint32 CRC bits
    (`& 0xFFFFFFFF` for the Java long value). crc_in, if given, is an int32
    tensor [S, nrows] of running CRCs to continue (CRC32.update chaining)."""
    rows, stride, L, S = _rows(row_views)
    ref = next(v for v in row_views if v is not None)
    cin, out = _dev_crcs((S, len(row_views)), ref, L, S, crc_in)
    code._check(_lib.lib().hrs_crc32_dev(code._handle(), rows, len(row_views), stride, L, S, cin, out.data_ptr(),
                                         _stream(ref)))
    return out


# ---- scrub, heal and heal with known erasures

SCRUB_BAD, SCRUB_UNRESOLVED, SCRUB_FIRST_BAD, SCRUB_HEAD = 0, 1, 2, 4  # report words (include/hrs.h)
SCRUB_PATCHED = 3  # heal only: bytes written back
SCRUB_NONE = 0xFFFFFFFF


def _dev_reports(code, L, S, ref):
    """The int32 report tensor [S, 4 + n] of a device call, for the library to
    fill; of a batch without bytes, filled here: every stripe is clean."""
    n = code.stripeSize() + code.paritySize()
    reports = _lib.torch.empty((S, SCRUB_HEAD + n), dtype=_lib.torch.int32, device=ref.device)
    if L == 0 or S == 0:
        reports.zero_()
        reports[:, SCRUB_FIRST_BAD] = -1
    return reports


def _erased_array(erased, S, what="erased"):
    """The host int32 [S, max_erased] erasure array of hrs_heal_erased_dev from
    a [S, m] array or a list of per-stripe location lists (-1 padded)."""
    torch = _lib.torch
    if torch is not None and isinstance(erased, torch.Tensor):
        erased = erased.cpu().numpy()
    if isinstance(erased, np.ndarray):
        arr = np.ascontiguousarray(erased.astype(np.int32))
        if arr.ndim != 2 or arr.shape[0] != S:
            raise ValueError(f"{what} must be [S, max_erased]")
        return arr
    lists = [list(e) for e in erased]
    if len(lists) != S:
        raise ValueError(f"{what} must list the erased locations of each of the {S} stripes")
    arr = np.full((S, max(1, max(len(e) for e in lists))), -1, dtype=np.int32)
    for s, e in enumerate(lists):
        arr[s, : len(e)] = e
    return arr


def _scrub(code, batch, op, erased=None, crcs=None, valid=None):
    """hrs_<op>_dev or hrs_<op>_crc_dev over _code_stripes' or _code_rows'
    tuple; op is "scrub", "heal" or, with `erased`, "heal_erased"; with `valid`
    (the cells' lengths, [S, n]) "scrub_ragged" or "heal_ragged". Returns the
    reports, with CRCs (reports, crcs)."""
    rows, stride, L, S, ref = batch
    args = [code._handle(), rows, stride, L, S]
    if valid is not None:
        v = _ragged_valid(code, valid, S, code.stripeSize() + code.paritySize())
        args.append(v.ctypes.data)
    if erased is not None:
        arr = _erased_array(erased, S)
        args += [arr.ctypes.data, arr.shape[1]]
    reports = _dev_reports(code, L, S, ref)
    args += [reports.data_ptr(), reports.shape[1]]
    if crcs is None:
        if L and S:
            code._check(getattr(_lib.lib(), f"hrs_{op}_dev")(*args, _stream(ref)))
        return reports
    cin, crc = _dev_crcs((S, reports.shape[1] - SCRUB_HEAD), ref, L, S, *crcs)
    if L and S:
        code._check(getattr(_lib.lib(), f"hrs_{op}_crc_dev")(*args, cin, crc.data_ptr(), _stream(ref)))
    return reports, crc


def _scrub_batch_host(code, stripes, op, erased=None, crcs=None, valid=None):
    """hrs_<op>_batch_host or hrs_<op>_batch_host_crc; op, valid and the result as for _scrub."""
    sp, row_stride, stripe_stride, L, S = _host_batch(code, stripes, writable=not op.startswith("scrub"))
    args = [code._handle(), sp, row_stride, stripe_stride, L, S]
    if valid is not None:
        v = _ragged_valid(code, valid, S, code.stripeSize() + code.paritySize())
        args.append(v.ctypes.data)
    if erased is not None:
        arr = _erased_array(erased, S)
        args += [arr.ctypes.data, arr.shape[1]]
    reports = np.zeros((S, SCRUB_HEAD + code.stripeSize() + code.paritySize()), dtype=np.uint32)
    args += [reports.ctypes.data, reports.shape[1]]
    if crcs is None:
        code._check(getattr(_lib.lib(), f"hrs_{op}_batch_host")(*args))
        return reports
    cin, crc = _host_crcs((S, reports.shape[1] - SCRUB_HEAD), L, *crcs)
    code._check(getattr(_lib.lib(), f"hrs_{op}_batch_host_crc")(*args, cin, crc.ctypes.data))
    return reports, crc


def scrub_stripes(code, stripes):
    """computeErrorLocations over every byte column of every stripe of
    stripes[S, n, L] (hrs_scrub_dev): an int32 tensor [S, 4 + n] holding the
    uint32 report words of each stripe — bad columns, unresolved columns,
    first bad column (SCRUB_NONE if clean), 0, then per location the columns
    that resolved and blamed it."""
    return _scrub(code, _code_stripes(code, stripes), "scrub")


def scrub_rows(code, row_views):
    """scrub_stripes with explicit [S, L] row views, one per location in hops order."""
    return _scrub(code, _code_rows(code, row_views), "scrub")


def scrub_batch_host(code, stripes):
    """hrs_scrub_batch_host: scrub_stripes for stripes[S, n, L] in HOST memory
    (numpy array or CPU tensor; pinned ones are read in place): a numpy uint32
    array [S, 4 + n]."""
    return _scrub_batch_host(code, stripes, "scrub")


def heal_stripes(code, stripes):
    """scrub_stripes plus the write-back (hrs_heal_dev): every column that
    computeErrorLocations resolves is rewritten in place to the method's
    post-call data, unresolved columns are left as they are. Returns the
    reports of the stripes as they were; word SCRUB_PATCHED counts the bytes
    stored."""
    return _scrub(code, _code_stripes(code, stripes), "heal")


def heal_rows(code, row_views):
    """heal_stripes with explicit [S, L] row views, one per location in hops order."""
    return _scrub(code, _code_rows(code, row_views), "heal")


def heal_batch_host(code, stripes):
    """hrs_heal_batch_host: heal_stripes for stripes[S, n, L] in HOST memory
    (numpy array or CPU tensor, healed in place; of staged memory only the
    cells that held a resolved error are written): a numpy uint32 array
    [S, 4 + n]."""
    return _scrub_batch_host(code, stripes, "heal")


def heal_host(code, rows):
    """hrs_heal_host: one stripe of n HOST rows (contiguous writable uint8
    numpy arrays of one length, hops order) healed in place on the CPU; works
    on host-only handles. Returns the report, a numpy uint32 array [4 + n]."""
    n = code.stripeSize() + code.paritySize()
    L = _host_stripe_rows(rows, n)
    report = np.zeros(SCRUB_HEAD + n, dtype=np.uint32)
    report[SCRUB_FIRST_BAD] = SCRUB_NONE
    code._check(_lib.lib().hrs_heal_host(code._handle(), _lib.ptr_array([r.ctypes.data for r in rows]), L,
                                         report.ctypes.data))
    return report


def scrub_stripes_ragged(code, stripes, valid):
    """scrub_stripes over cells of which only the leading valid[s, l] bytes
    hold data (hrs_scrub_ragged_dev): cell l of stripe s counts as those bytes
    followed by zeros, which are never read. valid: anything convertible to a
    uint32 [S, n] array in hops order, free for reuse on return. A column that
    only a patch of such a zero would resolve counts as unresolved."""
    return _scrub(code, _code_stripes(code, stripes), "scrub_ragged", valid=valid)


def heal_stripes_ragged(code, stripes, valid):
    """heal_stripes under scrub_stripes_ragged's lengths (hrs_heal_ragged_dev):
    nothing at or beyond a cell's valid is read or written."""
    return _scrub(code, _code_stripes(code, stripes), "heal_ragged", valid=valid)


def scrub_batch_host_ragged(code, stripes, valid):
    """hrs_scrub_ragged_batch_host: scrub_stripes_ragged for stripes[S, n, L]
    in HOST memory; staged memory sends only each cell's valid bytes."""
    return _scrub_batch_host(code, stripes, "scrub_ragged", valid=valid)


def heal_batch_host_ragged(code, stripes, valid):
    """hrs_heal_ragged_batch_host: heal_stripes_ragged for stripes[S, n, L] in
    HOST memory, healed in place; of staged memory only the valid bytes of the
    cells that held a resolved error are written."""
    return _scrub_batch_host(code, stripes, "heal_ragged", valid=valid)


def heal_host_ragged(code, rows, valid):
    """hrs_heal_ragged_host: heal_host with the stripe's n cell lengths; works
    on host-only handles. Returns the report, a numpy uint32 array [4 + n]."""
    n = code.stripeSize() + code.paritySize()
    L = _host_stripe_rows(rows, n)
    v = _ragged_valid(code, np.asarray(valid).reshape(1, -1), 1, n)
    report = np.zeros(SCRUB_HEAD + n, dtype=np.uint32)
    report[SCRUB_FIRST_BAD] = SCRUB_NONE
    code._check(_lib.lib().hrs_heal_ragged_host(code._handle(), _lib.ptr_array([r.ctypes.data for r in rows]), L,
                                                v.ctypes.data, report.ctypes.data))
    return report


def _host_stripe_rows(rows, n):
    if len(rows) != n:
        raise ValueError(f"need {n} rows")
    for r in rows:
        if not (isinstance(r, np.ndarray) and r.dtype == np.uint8 and r.ndim == 1 and r.flags.c_contiguous
                and r.flags.writeable and len(r) == len(rows[0])):
            raise ValueError("rows must be contiguous writable uint8 numpy arrays of one length")
    return len(rows[0])


def heal_erased_stripes(code, stripes, erased):
    """Heal with known erasures (hrs_heal_erased_dev) over stripes[S, n, L]:
    per stripe the lost cells erased[s] (an int [S, m] array, -1 padded, e.g.
    from checksums_to_erased, or a list of location lists; a stripe may have
    none) are rebuilt in place from the survivors, and silent errors in the
    survivors are located and fixed in the same pass wherever
    erasures + 2 * errors <= p per column. Returns the reports [S, 4 + n] in the
    heal's layout: columns whose survivors disagree, unresolved columns, first
    bad column, survivor bytes stored, then per survivor the resolved columns
    that blamed it."""
    return _scrub(code, _code_stripes(code, stripes), "heal_erased", erased)


def heal_erased_rows(code, row_views, erased):
    """heal_erased_stripes with explicit [S, L] row views, one per location in hops order."""
    return _scrub(code, _code_rows(code, row_views), "heal_erased", erased)


def heal_erased_host(code, rows, erased):
    """hrs_heal_erased_host: heal_erased_stripes for one stripe of n HOST rows
    (as for heal_host) on the CPU, the kernels' byte-exact reference; works on
    host-only handles. Returns the report, a numpy uint32 array [4 + n]."""
    n = code.stripeSize() + code.paritySize()
    L = _host_stripe_rows(rows, n)
    erased = [int(e) for e in erased]
    report = np.zeros(SCRUB_HEAD + n, dtype=np.uint32)
    report[SCRUB_FIRST_BAD] = SCRUB_NONE
    code._check(_lib.lib().hrs_heal_erased_host(code._handle(), _lib.ptr_array([r.ctypes.data for r in rows]), L,
                                                _lib.int_array(erased), len(erased), report.ctypes.data))
    return report


def heal_erased_stripes_crc(code, stripes, erased, crc_in=None):
    """heal_erased_stripes plus the CRC-32 of every cell AS THE CALL LEAVES IT
    (hrs_heal_erased_crc_dev): rebuilt cells, patched survivors, unresolved
    columns as they were. Returns (reports, crcs), crcs an int32 tensor [S, n]
    of the uint32 CRC bits in HOPS order as heal_stripes_crc returns them;
    crc_in ([S, n] int32) continues running CRCs. A stripe whose CRCs equal its
    stored checksums was restored."""
    return _scrub(code, _code_stripes(code, stripes), "heal_erased", erased, (crc_in,))


def heal_erased_rows_crc(code, row_views, erased, crc_in=None):
    """heal_erased_stripes_crc with explicit [S, L] row views, one per location in hops order."""
    return _scrub(code, _code_rows(code, row_views), "heal_erased", erased, (crc_in,))


def heal_erased_batch_host(code, stripes, erased):
    """hrs_heal_erased_batch_host: heal_erased_stripes for stripes[S, n, L] in
    HOST memory (numpy array or CPU tensor, healed in place; of staged memory
    only the survivors are copied in, and only the erased cells and the cells
    that held a resolved error are written): a numpy uint32 array [S, 4 + n].
    erased as for heal_erased_stripes."""
    return _scrub_batch_host(code, stripes, "heal_erased", erased)


def heal_erased_batch_host_crc(code, stripes, erased, crc_in=None, crc_out=None):
    """hrs_heal_erased_batch_host_crc: heal_erased_batch_host plus the CRC-32
    of every cell as the call leaves it: (reports, crcs), crcs a numpy uint32
    array [S, n] in HOPS order; crc_in and crc_out as for heal_batch_host_crc."""
    return _scrub_batch_host(code, stripes, "heal_erased", erased, (crc_in, crc_out))


def scrub_to_erased(reports, p):
    """The int32 [S, p] erasure array decode_batch takes from scrub reports
    [S, 4 + n]: per stripe the locations with a nonzero count, ascending, -1
    padded. ValueError for a stripe with unresolved columns or more than p
    blamed locations (not repairable from the report alone)."""
    torch = _lib.torch
    if torch is not None and isinstance(reports, torch.Tensor):
        reports = reports.cpu().numpy()
    r = np.asarray(reports)
    if r.ndim != 2 or r.shape[1] <= SCRUB_HEAD:
        raise ValueError("reports must be [S, 4 + n]")
    r = r.astype(np.int64) & 0xFFFFFFFF
    erased = np.full((r.shape[0], int(p)), -1, dtype=np.int32)
    for s in range(r.shape[0]):
        if r[s, SCRUB_UNRESOLVED]:
            raise ValueError(f"stripe {s}: {int(r[s, SCRUB_UNRESOLVED])} unresolved columns")
        locs = np.flatnonzero(r[s, SCRUB_HEAD:])
        if len(locs) > p:
            raise ValueError(f"stripe {s}: {len(locs)} blamed locations, the code repairs {int(p)}")
        erased[s, : len(locs)] = locs
    return erased


def scrub_stripes_crc(code, stripes, crc_in=None):
    """scrub_stripes plus the CRC-32 (java.util.zip.CRC32) of every cell from
    the same read (hrs_scrub_crc_dev): returns (reports, crcs), crcs an int32
    tensor [S, n] of the uint32 CRC bits in HOPS order (column l = location l,
    parity first; not encode_stripes_crc's data-first order), as crc32_rows
    returns it over the n rows. crc_in ([S, n] int32) continues running CRCs."""
    return _scrub(code, _code_stripes(code, stripes), "scrub", None, (crc_in,))


def scrub_rows_crc(code, row_views, crc_in=None):
    """scrub_stripes_crc with explicit [S, L] row views, one per location in hops order."""
    return _scrub(code, _code_rows(code, row_views), "scrub", None, (crc_in,))


def heal_stripes_crc(code, stripes, crc_in=None):
    """heal_stripes plus the CRC-32 of every cell AS IT IS AFTER the write-back
    (hrs_heal_crc_dev): (reports, crcs) as for scrub_stripes_crc. A cell whose
    CRC equals its stored checksum was restored."""
    return _scrub(code, _code_stripes(code, stripes), "heal", None, (crc_in,))


def heal_rows_crc(code, row_views, crc_in=None):
    """heal_stripes_crc with explicit [S, L] row views, one per location in hops order."""
    return _scrub(code, _code_rows(code, row_views), "heal", None, (crc_in,))


def scrub_batch_host_crc(code, stripes, crc_in=None, crc_out=None):
    """hrs_scrub_batch_host_crc: scrub_batch_host plus the CRC-32 of every cell
    from the same read: (reports, crcs), crcs a numpy uint32 array [S, n] in
    HOPS order. crc_in (same layout) continues running CRCs; crc_out: the array
    to fill and return (it may be crc_in itself)."""
    return _scrub_batch_host(code, stripes, "scrub", None, (crc_in, crc_out))


def heal_batch_host_crc(code, stripes, crc_in=None, crc_out=None):
    """hrs_heal_batch_host_crc: heal_batch_host plus the CRC-32 of every cell as
    it is after the write-back; arguments and result as scrub_batch_host_crc."""
    return _scrub_batch_host(code, stripes, "heal", None, (crc_in, crc_out))


def checksums_to_erased(crcs, stored, p, reports=None):
    """The int32 [S, p] erasure array decode_batch / decode_batch_crc and the
    heal-with-erasures calls (heal_erased_stripes[_crc], heal_erased_rows[_crc],
    heal_erased_batch_host[_crc]) take, from
    the cell CRCs of a scrub ([S, n], hops order) and the stored checksums:
    per stripe the locations whose CRC differs from `stored`, joined, when
    `reports` ([S, 4 + n]) is given, by the locations with a nonzero count in
    word 4 + l (a stale parity cell whose checksum was rewritten with it shows
    only there); ascending, -1 padded. A checksum names up to p bad cells where
    the syndromes stop at p / 2, so unresolved columns are no error here as
    long as some checksum of the stripe differs. ValueError for a stripe with
    more than p such locations, and for one with unresolved columns while no
    checksum differs (the data and the checksums disagree in a way neither
    names). scrub_to_erased is the rule for reports alone."""
    torch = _lib.torch

    def host(a):
        if a is not None and torch is not None and isinstance(a, torch.Tensor):
            a = a.cpu().numpy()
        return None if a is None else np.asarray(a)

    c, st, r = host(crcs), host(stored), host(reports)
    if c.ndim != 2 or st.shape != c.shape:
        raise ValueError("crcs and stored must both be [S, n]")
    S, n = c.shape
    differ = (c.astype(np.int64) & 0xFFFFFFFF) != (st.astype(np.int64) & 0xFFFFFFFF)
    if r is not None:
        if r.ndim != 2 or r.shape != (S, SCRUB_HEAD + n):
            raise ValueError("reports must be [S, 4 + n]")
        r = r.astype(np.int64) & 0xFFFFFFFF
    erased = np.full((S, int(p)), -1, dtype=np.int32)
    for s in range(S):
        bad = differ[s].copy()
        if r is not None:
            if r[s, SCRUB_UNRESOLVED] and not differ[s].any():
                raise ValueError(f"stripe {s}: {int(r[s, SCRUB_UNRESOLVED])} unresolved columns and no checksum differs")
            bad |= r[s, SCRUB_HEAD:] != 0
        locs = np.flatnonzero(bad)
        if len(locs) > p:
            raise ValueError(f"stripe {s}: {len(locs)} bad locations, the code repairs {int(p)}")
        erased[s, : len(locs)] = locs
    return erased


# hrs_repair_checked_dev / hrs_repair_checked_host: verdicts and the flag
REPAIR_CLEAN, REPAIR_REPAIRED, REPAIR_RESTAMP, REPAIR_FAILED, REPAIR_TOOMANY, REPAIR_AMBIGUOUS = range(6)
REPAIR_JOIN_SYNDROMES = 1


def _repair_checked(code, batch, stored, join_syndromes):
    rows, stride, L, S, ref = batch
    torch = _lib.torch
    n, p = code.stripeSize() + code.paritySize(), code.paritySize()
    if (not isinstance(stored, torch.Tensor) or stored.shape != (S, n) or stored.dtype != torch.int32
            or not stored.is_contiguous() or stored.device != ref.device):
        raise ValueError(f"stored must be a contiguous int32 device tensor [S, {n}]")
    verdicts = torch.empty((S,), dtype=torch.int32, device=ref.device)
    erased = torch.empty((S, p), dtype=torch.int32, device=ref.device)
    reports = _dev_reports(code, L, S, ref)
    crcs = torch.empty((S, n), dtype=torch.int32, device=ref.device)
    if L == 0 or S == 0:  # the call touches nothing: every stripe is clean, every CRC is over no bytes
        verdicts.zero_()
        erased.fill_(-1)
        crcs.zero_()
        return verdicts, erased, reports, crcs
    code._check(_lib.lib().hrs_repair_checked_dev(
        code._handle(), rows, stride, L, S, stored.data_ptr(), REPAIR_JOIN_SYNDROMES if join_syndromes else 0,
        verdicts.data_ptr(), erased.data_ptr(), reports.data_ptr(), SCRUB_HEAD + n, crcs.data_ptr(), _stream(ref)))
    return verdicts, erased, reports, crcs


def repair_checked_stripes(code, stripes, stored, join_syndromes=False):
    """Checked repair (hrs_repair_checked_dev) over stripes[S, n, L], all on the
    device and on the current stream: the cells' CRC-32s are compared with the
    checksums `stored` ([S, n] int32, hops order); a stripe whose checksums all
    match and whose syndromes are clean is REPAIR_CLEAN; one with more than p
    doubted cells is REPAIR_TOOMANY, one with unresolved columns and no
    differing checksum REPAIR_AMBIGUOUS, and neither is written; every other
    stripe is healed in place with the doubted cells as erasures
    (heal_erased_stripes' bytes and report) and called REPAIR_REPAIRED when
    every CRC then equals the stored one, REPAIR_RESTAMP when the stripe is a
    codeword and only checksums that matched before now differ (stale cells
    stamped with their own checksum: take the new values from crcs), else
    REPAIR_FAILED. join_syndromes adds the cells pass 1's syndromes blamed to
    the doubted ones (checksums_to_erased with reports): for few-column damage;
    whole-cell garbage makes the locator blame sound cells. Returns device
    tensors (verdicts [S], erased [S, p] ascending and -1 padded, reports
    [S, 4 + n], crcs [S, n]), all int32."""
    return _repair_checked(code, _code_stripes(code, stripes), stored, join_syndromes)


def repair_checked_rows(code, row_views, stored, join_syndromes=False):
    """repair_checked_stripes with explicit [S, L] row views, one per location in hops order."""
    return _repair_checked(code, _code_rows(code, row_views), stored, join_syndromes)


def repair_checked_host(code, rows, stored, join_syndromes=False):
    """hrs_repair_checked_host: repair_checked_stripes for one stripe of n HOST
    rows (as for heal_host) on the CPU, the device call's byte-exact reference;
    works on host-only handles. stored: n uint32 checksums. Returns (verdict,
    erased int32 [p], report uint32 [4 + n], crcs uint32 [n])."""
    n, p = code.stripeSize() + code.paritySize(), code.paritySize()
    L = _host_stripe_rows(rows, n)
    st = np.ascontiguousarray(np.asarray(stored).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    if st.shape != (n,):
        raise ValueError(f"stored must hold {n} checksums")
    verdict = np.zeros(1, dtype=np.uint32)
    erased = np.full(p, -1, dtype=np.int32)
    report = np.zeros(SCRUB_HEAD + n, dtype=np.uint32)
    report[SCRUB_FIRST_BAD] = SCRUB_NONE
    crcs = np.zeros(n, dtype=np.uint32)
    code._check(_lib.lib().hrs_repair_checked_host(
        code._handle(), _lib.ptr_array([r.ctypes.data for r in rows]), L, st.ctypes.data,
        REPAIR_JOIN_SYNDROMES if join_syndromes else 0, verdict.ctypes.data, erased.ctypes.data, report.ctypes.data,
        crcs.ctypes.data))
    return int(verdict[0]), erased, report, crcs


PROBE_COPY, PROBE_READ, PROBE_WRITE = 0, 1, 2
WAVE_TASKS, GRID_STRIDE, BLOCK_RANGE = 0, 1, 2  # hrs_probe_stream schedules


def _nbytes(t):
    return t.numel() * t.element_size()


def _probe_check(status):
    if status != _lib.HRS_OK:
        raise _lib.HrsError(status, "hrs_probe call rejected its arguments")


def _probe_stream(op, src, dst, schedule, depth, nontemporal, block_threads, blocks_per_cu, nbytes, stream):
    _probe_check(_lib.probe_lib().hrs_probe_stream(op, src, dst, nbytes, int(schedule), int(depth),
                                                   int(bool(nontemporal)), int(block_threads), int(blocks_per_cu),
                                                   stream))


def probe_copy(src, dst, schedule=BLOCK_RANGE, depth=8, nontemporal=True, block_threads=1024, blocks_per_cu=1):
    """HBM ceiling probe (libhrs_probe.so, hrs_probe_stream COPY): dst <- src,
    both contiguous device tensors of the same byte size, on the current
    stream. Diagnostic: bench.py's copy_peak. Default = the fastest copy
    schedule of tools/copy_lab.hip (block ranges, 8 in flight, nontemporal,
    one 1024-thread block per CU)."""
    if (not src.is_cuda or not dst.is_cuda or not src.is_contiguous() or not dst.is_contiguous()
            or _nbytes(dst) != _nbytes(src)):
        raise ValueError("probe_copy needs two contiguous device tensors of equal size")
    _probe_stream(PROBE_COPY, src.data_ptr(), dst.data_ptr(), schedule, depth, nontemporal, block_threads,
                  blocks_per_cu, _nbytes(src), _stream(src))


def probe_read(src, sink, schedule=BLOCK_RANGE, depth=8, nontemporal=True, block_threads=1024, blocks_per_cu=1):
    """HBM read-only probe (hrs_probe_stream READ): reads the contiguous
    device tensor `src` once; `sink` is a device tensor of >= 4 KiB (never
    written in practice)."""
    if not src.is_cuda or not src.is_contiguous() or not sink.is_cuda or _nbytes(sink) < 4096:
        raise ValueError("probe_read needs a contiguous device tensor and a 4 KiB device sink")
    _probe_stream(PROBE_READ, src.data_ptr(), sink.data_ptr(), schedule, depth, nontemporal, block_threads,
                  blocks_per_cu, _nbytes(src), _stream(src))


def probe_write(dst, schedule=BLOCK_RANGE, depth=8, nontemporal=True, block_threads=1024, blocks_per_cu=1):
    """HBM write-only probe (hrs_probe_stream WRITE): writes the contiguous
    device tensor `dst` once."""
    if not dst.is_cuda or not dst.is_contiguous():
        raise ValueError("probe_write needs a contiguous device tensor")
    _probe_stream(PROBE_WRITE, None, dst.data_ptr(), schedule, depth, nontemporal, block_threads, blocks_per_cu,
                  _nbytes(dst), _stream(dst))


def probe_rows(stripes, nread, nwrite, blocks_per_cu=2, schedule=0):
    """The coding kernels' access pattern without the math (hrs_probe_rows):
    `stripes` is a contiguous uint8 device tensor [S, nrows, L]; per 2 KiB
    column window rows [nrows - nread, nrows) are read and rows [0, nwrite)
    overwritten with their XOR (+ the row index); `schedule` 0-3 spaces the
    loads (include/hrs_probe.h)."""
    if (not stripes.is_cuda or stripes.dtype != _lib.torch.uint8 or stripes.dim() != 3
            or not stripes.is_contiguous()):
        raise ValueError("probe_rows needs a contiguous uint8 device tensor [S, nrows, L]")
    S, n, L = stripes.shape
    _probe_check(_lib.probe_lib().hrs_probe_rows(stripes.data_ptr(), S, n, L, int(nread), int(nwrite),
                                                 int(schedule), int(blocks_per_cu), _stream(stripes)))
