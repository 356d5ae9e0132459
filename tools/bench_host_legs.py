"""Every host-batch and repair-batch call of one build (the tree's libhrs.so, or HRS_LIB), timed end to end in
one process: one JSON line of raw milliseconds per leg. For A/B runs of host-side changes: alternate two
builds process by process and compare with tools/bench_host_legs_report.py (profiles/batch_fold/).
Shapes follow tools/bench_hbatch.py and bench.py's config 5 (RS(12,4), 256 KiB cells, 512 stripes, seeded
lost pair per stripe; pinned and pageable memory, the copy-engine knobs, 8-stripe batches for the fixed cost)
and the host legs of tools/bench_heal.py, bench_scrub_crc.py, bench_heal_erased_crc.py and bench_batch_crc.py
(RS(10,4), 256 KiB cells, 256 stripes). Every leg's output is checked.

Run: python tools/bench_host_legs.py   (AB_REPS: timed calls per leg, default 7)
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402
from lambdafs_amd import HipReedSolomonCode, _lib, device  # noqa: E402

REPS = int(os.environ.get("AB_REPS", "7"))
KNOBS = ("HRS_ZEROCOPY", "HRS_HBATCH_DUPLEX", "HRS_ZC_BLOCKS", "HRS_HBATCH_BYTES", "HRS_HBATCH_MERGE")


def timed(fn, reps=REPS, env=None, before=None):
    for key in KNOBS:
        os.environ.pop(key, None)
    os.environ.update(env or {})
    ms = []
    for r in range(reps + 1):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            ms.append(round(dt, 4))
    for key in KNOBS:
        os.environ.pop(key, None)
    return ms


def pinned(shape, dtype=torch.uint8):
    return torch.empty(shape, dtype=dtype, pin_memory=True)


def main():
    res = {"lib": _lib.LIB_PATH}
    L = 256 << 10
    # ---- config 5: decode / encode host batches, plain and CRC
    k, p, S = 12, 4, 512
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    st_dev = torch.zeros((S, n, L), dtype=torch.uint8, device="cuda")
    synth.fill_data_rows(torch, st_dev, 5, 0, k, p)
    device.encode_stripes(code, st_dev)
    torch.cuda.synchronize()
    ref = st_dev.cpu().numpy()
    st = pinned((S, n, L))
    st.copy_(torch.from_numpy(ref))
    stn = st.numpy()
    er = np.array([np.sort(np.random.default_rng([0x5EED0005, s]).choice(n, 2, replace=False)) for s in range(S)],
                  dtype=np.int32)
    outn = pinned((S, 2, L)).numpy()
    pg = np.array(stn)
    pout = np.zeros((S, 2, L), np.uint8)
    idx = np.arange(S)[:, None]
    want = ref[idx, er]
    crc_d = np.zeros((S, 2), np.uint32)
    crc_e = np.zeros((S, n), np.uint32)

    def zero_par(a):
        return lambda: a[:, :p].fill(0)

    R = {}
    R["decode_pinned"] = timed(lambda: device.decode_batch_host(code, stn, er, outn))
    assert np.array_equal(outn, want)
    R["decode_pageable"] = timed(lambda: device.decode_batch_host(code, pg, er, pout))
    assert np.array_equal(pout, want)
    R["encode_pinned"] = timed(lambda: device.encode_batch_host(code, stn), before=zero_par(stn))
    assert np.array_equal(stn, ref)
    R["encode_pageable"] = timed(lambda: device.encode_batch_host(code, pg), before=zero_par(pg))
    assert np.array_equal(pg, ref)
    outn.fill(0)
    pout.fill(0)
    R["decode_crc_pinned"] = timed(lambda: device.decode_batch_host_crc(code, stn, er, outn, crc_out=crc_d))
    c1 = crc_d.copy()
    assert np.array_equal(outn, want)
    R["decode_crc_pageable"] = timed(lambda: device.decode_batch_host_crc(code, pg, er, pout, crc_out=crc_d))
    assert np.array_equal(pout, want) and np.array_equal(c1, crc_d)
    R["encode_crc_pinned"] = timed(lambda: device.encode_batch_host_crc(code, stn, crc_out=crc_e), before=zero_par(stn))
    c2 = crc_e.copy()
    assert np.array_equal(stn, ref)
    R["encode_crc_pageable"] = timed(lambda: device.encode_batch_host_crc(code, pg, crc_out=crc_e),
                                     before=zero_par(pg))
    assert np.array_equal(pg, ref) and np.array_equal(c2, crc_e)
    # the copy-engine pipelines (A/B knobs)
    ring = {"HRS_ZEROCOPY": "0"}
    duplex = {"HRS_ZEROCOPY": "0", "HRS_HBATCH_DUPLEX": "1"}
    outn.fill(0)
    pout.fill(0)
    R["ring_decode_pinned"] = timed(lambda: device.decode_batch_host(code, stn, er, outn), env=ring)
    assert np.array_equal(outn, want)
    R["ring_decode_pageable"] = timed(lambda: device.decode_batch_host(code, pg, er, pout), env=ring)
    assert np.array_equal(pout, want)
    R["ring_encode_pageable"] = timed(lambda: device.encode_batch_host(code, pg), env=ring, before=zero_par(pg))
    assert np.array_equal(pg, ref)
    outn.fill(0)
    R["duplex_decode_pinned"] = timed(lambda: device.decode_batch_host(code, stn, er, outn), env=duplex)
    assert np.array_equal(outn, want)
    R["nomerge_decode_pageable"] = timed(lambda: device.decode_batch_host(code, pg, er, pout),
                                         env={"HRS_HBATCH_MERGE": "0"})
    # small batches: the call's fixed cost (8 stripes of 64 KiB cells)
    s8 = pinned((8, n, 64 << 10)).numpy()
    s8[:] = ref[:8, :, :64 << 10]
    o8 = pinned((8, 2, 64 << 10)).numpy()
    p8 = np.array(s8)
    po8 = np.zeros((8, 2, 64 << 10), np.uint8)
    R["small_decode_pinned"] = timed(lambda: device.decode_batch_host(code, s8, er[:8], o8), reps=60)
    R["small_decode_pageable"] = timed(lambda: device.decode_batch_host(code, p8, er[:8], po8), reps=60)
    R["small_encode_pageable"] = timed(lambda: device.encode_batch_host(code, p8), reps=60)
    # device-resident repair batches (the call returns once queued: timed to the sync)
    od = torch.empty((S, 2, L), dtype=torch.uint8, device="cuda")

    def dev_plain():
        device.decode_batch(code, st_dev, er, od)
        torch.cuda.synchronize()

    def dev_crc():
        device.decode_batch_crc(code, st_dev, er, od)
        torch.cuda.synchronize()

    R["dev_decode"] = timed(dev_plain, reps=20)
    R["dev_decode_crc"] = timed(dev_crc, reps=20)
    assert np.array_equal(od.cpu().numpy(), want)
    del st_dev, od, st, stn, pg, pout, outn, want, ref
    torch.cuda.empty_cache()
    # ---- scrub / heal / heal-erased host batches, plain and CRC
    k, p, S = 10, 4, 256
    n = k + p
    code = HipReedSolomonCode(k, p, device=0)
    sd = torch.zeros((S, n, L), dtype=torch.uint8, device="cuda")
    synth.fill_data_rows(torch, sd, 7, 0, k, p)
    device.encode_stripes(code, sd)
    torch.cuda.synchronize()
    ref = sd.cpu().numpy()
    hp = pinned((S, n, L)).numpy()
    hp[:] = ref
    hg = np.array(ref)
    er = np.array([np.sort(np.random.default_rng([0x5EED0007, s]).choice(n, 2, replace=False)) for s in range(S)],
                  dtype=np.int32)
    for name, a in (("pinned", hp), ("pageable", hg)):
        R[f"scrub_{name}"] = timed(lambda: device.scrub_batch_host(code, a))
        R[f"heal_{name}"] = timed(lambda: device.heal_batch_host(code, a))
        R[f"scrub_crc_{name}"] = timed(lambda: device.scrub_batch_host_crc(code, a))
        R[f"heal_crc_{name}"] = timed(lambda: device.heal_batch_host_crc(code, a))
        R[f"heal_erased_{name}"] = timed(lambda: device.heal_erased_batch_host(code, a, er))
        R[f"heal_erased_crc_{name}"] = timed(lambda: device.heal_erased_batch_host_crc(code, a, er))
        assert np.array_equal(a, ref), name
    res["legs_ms"] = R
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
