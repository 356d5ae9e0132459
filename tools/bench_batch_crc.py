"""Batch repair / host batch timing with block checksums
(hrs_decode_batch_crc_dev, hrs_decode_batch_host_crc, hrs_encode_batch_host_crc)
beside the routes a caller had before them, one JSON line.

  (1) device: 1 MiB cells, 1,024 stripes, a seeded random set of `ne` lost
      locations per stripe, for ne = 1, 2, 3 on RS(10,4) and ne = 4 on RS(8,4)
      (4 losses of RS(10,4) read 10 survivors, beyond the fused kernel). Legs,
      alternating in this process:
        fused     decode_batch_crc
        two_pass  decode_batch, then crc32_rows over out  (the yardstick: the
                  route without the new call; its code is not changed by it)
        plain     decode_batch alone
        uniform   decode_stripes_crc, one pattern for every stripe (for scale)
      fused_wins = the fused median lies below the two-pass median by more than
      the two-pass leg's own max - min.
  (2) host: RS(12,4), 256 KiB cells, 512 stripes, pinned then pageable:
      decode_batch_host_crc against decode_batch_host, encode_batch_host_crc
      against encode_batch_host (host clock; the calls are synchronous), and
      zlib.crc32 over the same cells on one thread, once, for the host
      alternative.

Warm-up, then HIP events around each repetition of the device legs, median of
--reps (>= 20) with [min, max]. Run it on an idle card.

  python tools/bench_batch_crc.py [--stripes 1024] [--reps 20] [--out profiles/batch_crc/bench_batch_crc.json]
"""
import argparse
import json
import os
import random
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lambdafs_amd import HipReedSolomonCode, device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--stripes", type=int, default=1024)
ap.add_argument("--cell", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--host-stripes", type=int, default=512)
ap.add_argument("--host-cell", type=int, default=256 << 10)
ap.add_argument("--skip-host", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_crc", "bench_batch_crc.json"))
args = ap.parse_args()
if args.reps < 20:
    ap.error("--reps must be at least 20")


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def interleaved(fns, host_clock=False):
    samples = {name: [] for name in fns}
    for r in range(args.warmup + args.reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            if host_clock:
                t0 = time.perf_counter()
                fn()
                ms = (time.perf_counter() - t0) * 1e3
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms = a.elapsed_time(b)
            if r >= args.warmup:
                samples[name].append(ms)
    return {name: stats(ms) for name, ms in samples.items()}


def patterns(S, n, ne, seed):
    rnd = random.Random(seed)
    return np.array([sorted(rnd.sample(range(n), ne)) for _ in range(S)], dtype=np.int32)


def zlib_words(cells):
    return np.array([zlib.crc32(c.tobytes()) for c in cells], dtype=np.uint32)


torch.manual_seed(31)
res = {"bench": "batch_crc", "gpu": torch.cuda.get_device_name(0), "reps": args.reps, "device": [], "host": []}

# (1) device
S, L = args.stripes, args.cell
for k, p, ne in ((10, 4, 1), (10, 4, 2), (10, 4, 3), (8, 4, 4)):
    n = k + p
    code = HipReedSolomonCode(k, p)
    st = torch.randint(0, 256, (S, n, L), dtype=torch.uint8, device="cuda")
    out = torch.empty((S, ne, L), dtype=torch.uint8, device="cuda")
    er = patterns(S, n, ne, seed=ne)
    uni = [int(x) for x in er[0]]
    to_read = sorted(code.locationsToReadForDecode(uni))
    ntr = [x for x in range(n) if x not in to_read]
    kernels = {}

    def fused():
        return device.decode_batch_crc(code, st, er, out)

    def two_pass():
        device.decode_batch(code, st, er, out)
        return device.crc32_rows(code, [out[:, t] for t in range(ne)])

    got = fused()
    kernels["fused"] = code.lastKernel()  # batch_decode_crc_kernel<...>, unless the count is routed to two passes
    ref_out = out.clone()
    want = two_pass()
    kernels["plain"] = code.lastKernel()
    assert torch.equal(got, want) and torch.equal(out, ref_out), "fused and two-pass routes disagree"
    sample = list(range(0, S, max(1, S // 8)))
    assert np.array_equal(got[sample].cpu().numpy().view(np.uint32).reshape(-1),
                          zlib_words([out[s, t].cpu().numpy() for s in sample for t in range(ne)]))
    device.decode_stripes_crc(code, st, uni, ntr, out)
    kernels["uniform"] = code.lastKernel()
    t = interleaved({
        "fused": fused,
        "two_pass": two_pass,
        "plain": lambda: device.decode_batch(code, st, er, out),
        "uniform": lambda: device.decode_stripes_crc(code, st, uni, ntr, out),
    })
    spread = t["two_pass"]["max_ms"] - t["two_pass"]["min_ms"]
    moved = (k + ne) * L * S  # survivors read + repaired cells written, once
    res["device"].append({
        "k": k, "p": p, "losses": ne, "cell": L, "stripes": S, "kernels": kernels, **t,
        "fused_wins": bool(t["two_pass"]["median_ms"] - t["fused"]["median_ms"] > spread),
        "fused_over_two_pass": round(t["fused"]["median_ms"] / t["two_pass"]["median_ms"], 4),
        "fused_GBps": round(moved / (t["fused"]["median_ms"] * 1e-3) / 1e9, 1),
        "two_pass_GBps": round(moved / (t["two_pass"]["median_ms"] * 1e-3) / 1e9, 1),
    })
    del st, out, ref_out
    torch.cuda.empty_cache()

# (2) host batches
if not args.skip_host:
    k, p, S, L = 12, 4, args.host_stripes, args.host_cell
    n = k + p
    code = HipReedSolomonCode(k, p)
    dev = torch.randint(0, 256, (S, n, L), dtype=torch.uint8, device="cuda")
    base = dev.cpu().numpy()
    del dev
    er = np.full((S, 4), -1, dtype=np.int32)
    er[:, :2] = patterns(S, n, 2, seed=5)
    t0 = time.perf_counter()
    zl = zlib_words([base[s, p + r] if r < k else base[s, r - k] for s in range(S) for r in range(n)])
    res["zlib_one_thread"] = {"cells": S * n, "bytes": S * n * L, "ms": round((time.perf_counter() - t0) * 1e3, 1)}
    for pinned in (True, False):
        st = torch.empty((S, n, L), dtype=torch.uint8, pin_memory=True).numpy() if pinned else np.empty_like(base)
        st[:] = base
        out = (torch.empty((S, 4, L), dtype=torch.uint8, pin_memory=True).numpy() if pinned
               else np.empty((S, 4, L), np.uint8))
        crc = device.decode_batch_host_crc(code, st, er, out)
        path, kern = code.lastHostPath(), code.lastKernel()
        sample = list(range(0, S, max(1, S // 8)))
        assert np.array_equal(crc[sample, :2].reshape(-1), zlib_words([out[s, t] for s in sample for t in range(2)]))
        t = interleaved({
            "decode_crc": lambda: device.decode_batch_host_crc(code, st, er, out),
            "decode": lambda: device.decode_batch_host(code, st, er, out),
            "encode_crc": lambda: device.encode_batch_host_crc(code, st),
            "encode": lambda: device.encode_batch_host(code, st),
        }, host_clock=True)
        device.encode_batch_host_crc(code, st)
        ekern = code.lastKernel()
        dmoved, emoved = (k + 2) * L * S, n * L * S
        res["host"].append({
            "k": k, "p": p, "cell": L, "stripes": S, "memory": "pinned" if pinned else "pageable", "path": path,
            "decode_kernel": kern, "encode_kernel": ekern, **t,
            "decode_crc_over_decode": round(t["decode_crc"]["median_ms"] / t["decode"]["median_ms"], 4),
            "encode_crc_over_encode": round(t["encode_crc"]["median_ms"] / t["encode"]["median_ms"], 4),
            "decode_crc_GiBps": round(dmoved / (t["decode_crc"]["median_ms"] * 1e-3) / 2 ** 30, 2),
            "decode_GiBps": round(dmoved / (t["decode"]["median_ms"] * 1e-3) / 2 ** 30, 2),
            "encode_crc_GiBps": round(emoved / (t["encode_crc"]["median_ms"] * 1e-3) / 2 ** 30, 2),
            "encode_GiBps": round(emoved / (t["encode"]["median_ms"] * 1e-3) / 2 ** 30, 2),
        })

line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
