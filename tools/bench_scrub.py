"""Stripe-scrub timing (hrs_scrub_dev / hrs_scrub_batch_host), one JSON line.

  (a) clean stripes, device resident: RS(10,4), 1 MiB cells, 1,024 stripes
      (14 GiB read per pass), GB/s of bytes read — beside the read-only
      ceiling device.probe_read measures over the same tensor in the same
      process (the probe is the yardstick);
  (b) the same stripes with one whole corrupted cell each: every column takes
      the slow path (un-slice, locator, LDS histogram, atomics); time only;
  (c) hrs_scrub_batch_host from pinned memory: RS(12,4), 256 KiB cells,
      GiB/s of bytes moved.

Warm-up, then HIP events around each repetition, median of --reps (>= 20);
(c) is synchronous and timed with the host clock. Run it on an idle card.

  python tools/bench_scrub.py [--stripes 1024] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

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
ap.add_argument("--host-stripes", type=int, default=256)
ap.add_argument("--host-cell", type=int, default=256 << 10)
ap.add_argument("--out", default=None, help="also write the JSON line here")
args = ap.parse_args()
if args.reps < 20:
    ap.error("--reps must be at least 20")


def timed(fn):
    """Median and minimum milliseconds of fn() on the current stream."""
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0]


torch.manual_seed(23)
k, p, L, S = 10, 4, args.cell, args.stripes
n = k + p
code = HipReedSolomonCode(k, p)
st = torch.randint(0, 256, (S, n, L), dtype=torch.uint8, device="cuda")
device.encode_stripes(code, st)
nbytes = n * L * S
sink = torch.zeros(4096, dtype=torch.uint8, device="cuda")

reports = device.scrub_stripes(code, st)
torch.cuda.synchronize()
assert int((reports[:, 0] != 0).sum()) == 0, "encoded stripes must scrub clean"
clean_med, clean_min = timed(lambda: device.scrub_stripes(code, st))
kernel = code.lastKernel()
probe_med, probe_min = timed(lambda: device.probe_read(st, sink))

# (b) one whole corrupted cell per stripe
for s in range(S):
    st[s, s % n].bitwise_not_()
reports = device.scrub_stripes(code, st)
torch.cuda.synchronize()
r = reports.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
assert (r[:, 0] == L).all() and (r[:, 1] == 0).all(), "every column of every stripe has one error"
assert all(r[s, 4 + s % n] == L for s in range(S))
bad_med, bad_min = timed(lambda: device.scrub_stripes(code, st))
del st, reports
torch.cuda.empty_cache()

# (c) host batch from pinned memory
hk, hp, hL, hS = 12, 4, args.host_cell, args.host_stripes
hn = hk + hp
hcode = HipReedSolomonCode(hk, hp)
dev = torch.randint(0, 256, (hS, hn, hL), dtype=torch.uint8, device="cuda")
device.encode_stripes(hcode, dev)
pinned = dev.cpu().pin_memory()
del dev
hbytes = hn * hL * hS
got = device.scrub_batch_host(hcode, pinned)
assert not got[:, 0].any(), "encoded host stripes must scrub clean"
for _ in range(args.warmup):
    device.scrub_batch_host(hcode, pinned)
hms = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    device.scrub_batch_host(hcode, pinned)
    hms.append((time.perf_counter() - t0) * 1e3)
hms.sort()
host_med = hms[len(hms) // 2]

line = json.dumps({
    "bench": "scrub", "k": k, "p": p, "cell": L, "stripes": S, "bytes_read": nbytes, "reps": args.reps,
    "kernel": kernel,
    "clean_median_ms": round(clean_med, 4), "clean_min_ms": round(clean_min, 4),
    "clean_GBps": round(nbytes / (clean_med * 1e-3) / 1e9, 1),
    "probe_read_median_ms": round(probe_med, 4), "probe_read_min_ms": round(probe_min, 4),
    "probe_read_GBps": round(nbytes / (probe_med * 1e-3) / 1e9, 1),
    "clean_over_probe": round(probe_med / clean_med, 4),
    "all_bad_median_ms": round(bad_med, 3), "all_bad_min_ms": round(bad_min, 3),
    "host": {"k": hk, "p": hp, "cell": hL, "stripes": hS, "bytes_moved": hbytes, "path": hcode.lastHostPath(),
             "median_ms": round(host_med, 3), "min_ms": round(hms[0], 3),
             "GiBps": round(hbytes / (host_med * 1e-3) / 2 ** 30, 2)},
})
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
