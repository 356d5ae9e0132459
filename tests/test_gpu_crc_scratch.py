"""The handle's shared raw-CRC scratch under two streams, across the entry
families that lease it, with the buffer growing in between: crc32_rows,
scrub / heal / heal-erased with CRCs (kernel modes 0 and 3), decode_batch_crc,
repair_checked_stripes (an outer lease around pass 1's own) and
encode_stripes_crc on one rs(10,4) handle, alternating between two non-default
streams with no host synchronisation between the calls. L = 4096 is two whole
2 KiB windows (the one-pass routes), L = 4096 + 13 adds a row tail (the
two-pass routes), S = 2; one S = 48 scrub at L = 32768 + 13 in the middle asks
for more scratch than any call before it, so the buffer is freed and
reallocated while earlier folds may still be queued. The sequence runs twice.

After one final synchronise every CRC must equal zlib.crc32 of the host copy
of the cell as the call left it, and every report, verdict, erased list and
cell must equal what the same call returns alone on the default stream of a
handle of its own. This cannot prove ordering; it catches a lease that skips
the wait, records on the wrong stream, or frees the buffer under a queued
fold. Codeword stripes come from the CPU oracle (tests/heal_erased_inputs.py)."""
import zlib

import numpy as np
import pytest

import heal_erased_inputs as H
from lambdafs_amd import HipReedSolomonCode, device

pytestmark = pytest.mark.gpu

K, P = 10, 4
N = K + P
SMALL, TAIL, LARGE = 2 * H.WINDOW, 2 * H.WINDOW + 13, 16 * H.WINDOW + 13
CALLS = ["crc32_rows", "scrub", "heal", "heal_erased_0", "heal_erased_3", "decode_batch", "repair_checked"]
# (call, L, S) in queue order; the large scrub goes to stream B, the rest alternate A, B
SEQUENCE = ([(c, SMALL, 2) for c in CALLS] + [("encode", SMALL, 2), ("scrub", LARGE, 48)] +
            [(c, TAIL, 2) for c in CALLS])
ERASED = [[P + 1], [0, 7]]  # heal with erasures: one data cell; parity 0 and a data cell
LOST = np.array([[5, -1], [0, 9]], dtype=np.int32)  # decode_batch: per stripe, -1 padded


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _place(torch, host):
    """host[S, m, L] on the device as a view whose row pitch is a multiple of
    16, so that a row tail leaves the whole windows to the vector kernels."""
    s, m, length = host.shape
    big = torch.full((s, m, (length + 15) // 16 * 16), 0xC3, dtype=torch.uint8, device="cuda:0")
    view = big[:, :, :length]
    view.copy_(torch.from_numpy(np.ascontiguousarray(host)).to("cuda:0"))
    return view


def _inputs(torch, call, L, S):
    """The device inputs of one call, built and copied up before the sequence starts."""
    clean = H.clean_stripes(K, P, S, L, 7)
    st = np.array(clean)
    x = {}
    if call == "heal":
        st[S - 1, 5, 100] ^= 0x5A  # one corrupted byte
    elif call.startswith("heal_erased"):
        for s, e in enumerate(ERASED):
            st[s, e, :] = H.FILL
        st[0, 9, L - 1] ^= 0x11  # and a survivor error within capacity
    elif call == "decode_batch":
        for s in range(S):
            st[s, LOST[s][LOST[s] >= 0], :] = H.FILL  # lost cells are never read
        x["out"] = torch.full((S, LOST.shape[1], L), 0x3C, dtype=torch.uint8, device="cuda:0")
    elif call == "repair_checked":
        x["stored"] = torch.from_numpy(_crcs(clean).view(np.int32)).to("cuda:0")
        st[0, 3, :] = H.FILL  # a cell of garbage: its checksum differs, the heal rebuilds it
    elif call == "encode":
        st[:, :P] = 0
    x["st"] = _place(torch, st)
    return x


def _crcs(cells):
    return np.array([[zlib.crc32(c.tobytes()) for c in stripe] for stripe in cells], dtype=np.uint32)


def _run(code, call, x):
    """One call on the current stream. Returns device tensors only: the CRCs,
    the cells they cover (read back after the final synchronise) and what must
    equal the call made alone."""
    st = x["st"]
    if call == "crc32_rows":
        return {"crc": device.crc32_rows(code, [st[:, l] for l in range(N)]), "cells": st, "same": []}
    if call in ("scrub", "heal"):
        fn = device.heal_stripes_crc if call == "heal" else device.scrub_stripes_crc
        rep, crc = fn(code, st)
        L = st.shape[2]
        want = f"{call}_crc_kernel<{P}>" if L % H.WINDOW == 0 else f"{call}_kernel<{P}>"
        assert code.lastKernel() == want, (call, L, code.lastKernel())
        return {"crc": crc, "cells": st, "same": [rep]}
    if call.startswith("heal_erased"):
        code.setKernelMode(int(call[-1]))
        try:
            rep, crc = device.heal_erased_stripes_crc(code, st, ERASED)
        finally:
            code.setKernelMode(0)
        return {"crc": crc, "cells": st, "same": [rep]}
    if call == "decode_batch":
        return {"crc": device.decode_batch_crc(code, st, LOST, x["out"]), "cells": x["out"], "same": []}
    if call == "repair_checked":
        verdicts, erased, rep, crc = device.repair_checked_stripes(code, st, x["stored"])
        return {"crc": crc, "cells": st, "same": [verdicts, erased, rep]}
    assert call == "encode"
    crc = device.encode_stripes_crc(code, st)
    assert code.lastKernel().startswith("encode_crc"), code.lastKernel()
    return {"crc": crc, "cells": st, "same": []}


def _want_crcs(call, cells):
    """zlib over the host copy of the cells, in the order the call returns its CRCs."""
    z = _crcs(cells)
    if call == "encode":  # sources first, then parities
        return np.concatenate([z[:, P:], z[:, :P]], axis=1)
    if call == "decode_batch":  # an entry past its stripe's losses continues over no bytes
        return np.where(LOST >= 0, z, 0).astype(np.uint32)
    return z


def _host(outs):
    return {"crc": _u32(outs["crc"]), "cells": outs["cells"].cpu().numpy(),
            "same": [t.cpu().numpy() for t in outs["same"]]}


def test_shared_scratch_across_two_streams_with_growth(cuda):
    torch = cuda
    # every call alone on the default stream, on a handle of its own
    alone_code = HipReedSolomonCode(K, P, device=0)
    alone = {}
    for step in dict.fromkeys(SEQUENCE):
        outs = _run(alone_code, step[0], _inputs(torch, *step))
        torch.cuda.synchronize()
        alone[step] = _host(outs)
    # the sequence, twice, on two streams of one fresh handle
    code = HipReedSolomonCode(K, P, device=0)
    rounds = [[_inputs(torch, *step) for step in SEQUENCE] for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()  # the inputs are in place; from here on the host waits for nothing
    queued = []
    for xs in rounds:
        for i, (step, x) in enumerate(zip(SEQUENCE, xs)):
            with torch.cuda.stream(streams[1 if step[1] == LARGE else i % 2]):
                queued.append((step, _run(code, step[0], x)))
    torch.cuda.synchronize()
    for i, (step, outs) in enumerate(queued):
        got, ref = _host(outs), alone[step]
        where = (i, *step)
        assert got["crc"].tolist() == _want_crcs(step[0], got["cells"]).tolist(), where
        assert (got["cells"] == ref["cells"]).all(), where
        assert len(got["same"]) == len(ref["same"])
        for a, b in zip(got["same"], ref["same"]):
            assert a.tolist() == b.tolist(), where
