"""Window map sweep (HRS_WINDOW_SPLIT, lambdafs_amd/csrc/hrs_window_map.hpp: the
half distance H in bytes between a wave task's two 1 KiB pieces; 1024 = the
contiguous 2 KiB window) in one process: the variants alternate per round (the
variable is read per launch), HIP-event times on the launch stream, the median
and the minimum over the rounds of each variant, and the spread of the 1 KiB
runs (max / min over its rounds) that a gain has to beat.

Stage "probe": the no-math access pattern (hrs_probe_rows) for 10 reads / 4
writes and 10 / 1 at the bench shape, load schedules 0 and 1, 1 and 2 blocks
per CU. Stage "product": RS(10,4) 1 MiB x 1,024 encode and 1- to 4-loss
repairs, RS(12,4) 256 KiB x 512 and RS(6,3) 64 KiB x 4,096 encode and repair,
and a small job (RS(10,4) 1 MiB x 128); every product launch's output under
every H is compared with the 1 KiB map's.
Run: python tools/bench_split.py [--stage probe|product|all] [--rounds 10] [--iters 5]
(one JSON line per workload)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lambdafs_amd import HipReedSolomonCode, device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--stage", default="all", choices=["probe", "product", "all"])
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--splits", default="1024,4096,16384,32768,65536,131072,262144")
ap.add_argument("--stripes", type=int, default=1024, help="stripes of the bench shape (smaller for a rehearsal)")
args = ap.parse_args()
SPLITS = [int(x) for x in args.splits.split(",")]
assert SPLITS[0] == 1024 and args.rounds >= 1, "the first variant is the contiguous map every other is compared with"


def timed(fn):
    ms = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def set_split(h):
    os.environ["HRS_WINDOW_SPLIT"] = str(h)


def sweep(name, fn, nbytes, extra):
    times = {h: [] for h in SPLITS}
    for _ in range(args.rounds):
        for h in SPLITS:
            set_split(h)
            fn()
            torch.cuda.synchronize()
            times[h].append(timed(fn))
    med = {h: float(np.median(times[h])) for h in SPLITS}
    mn = {h: float(np.min(times[h])) for h in SPLITS}
    base = times[SPLITS[0]]
    best = min(SPLITS, key=lambda h: med[h])
    row = {"workload": name, **extra,
           "median_ms": {str(h): round(med[h], 4) for h in SPLITS},
           "min_ms": {str(h): round(mn[h], 4) for h in SPLITS},
           "median_GBps": {str(h): round(nbytes / 1e9 / (med[h] * 1e-3), 1) for h in SPLITS},
           "spread_1k": round(max(base) / min(base), 4),
           "best_split": best, "best_vs_1k": round(med[SPLITS[0]] / med[best], 4),
           "rounds": args.rounds, "iters": args.iters}
    print(json.dumps(row), flush=True)
    return row


def probe_stage():
    S, n, L = args.stripes, 14, 1 << 20
    st = torch.randint(0, 256, (S, n, L), dtype=torch.uint8, device="cuda")
    for nr, nw in ((10, 4), (10, 1)):
        for sched in (0, 1):
            for bpc in (1, 2):
                sweep(f"probe {nr}r/{nw}w sched{sched} {bpc}/CU 1024 KiB x {S}",
                      lambda: device.probe_rows(st, nr, nw, bpc, sched), (nr + nw) * L * S, {})
    del st


def product_workloads():
    out = []
    shapes = ((10, 4, 1 << 20, args.stripes, ([4], [0, 5], [1, 6, 11], [0, 4, 9, 13])),
              (12, 4, 256 << 10, max(1, args.stripes // 2), ([0, 5],)),
              (6, 3, 64 << 10, args.stripes * 4, ([2],)),
              (10, 4, 1 << 20, max(1, args.stripes // 8), ([4],)))
    for k, p, L, S, losses in shapes:
        n = k + p
        code = HipReedSolomonCode(k, p)
        st = torch.randint(0, 256, (S, n, L), dtype=torch.uint8, device="cuda")
        device.encode_stripes(code, st)
        shape = f"RS({k},{p}) {L >> 10} KiB x {S}"
        par = st[:, :p]
        out.append((f"{shape} encode", code, lambda code=code, st=st: device.encode_stripes(code, st), par,
                    (k + p) * L * S))
        for er in losses:
            to_read = sorted(code.locationsToReadForDecode(er))
            ntr = [x for x in range(n) if x not in to_read]
            o = torch.empty((S, len(er), L), dtype=torch.uint8, device="cuda")
            out.append((f"{shape} decode {er}", code,
                        lambda code=code, st=st, er=er, ntr=ntr, o=o: device.decode_stripes(code, st, er, ntr, o), o,
                        (k + len(er)) * L * S))
    return out


def product_stage():
    bad = []
    for name, code, fn, target, nbytes in product_workloads():
        outs, kern = {}, {}
        for h in SPLITS:
            set_split(h)
            target.fill_(0xA5)  # a piece the map skips would leave this behind
            fn()
            torch.cuda.synchronize()
            outs[h] = target.clone()
            kern[h] = code.lastKernel()
        ident = all(bool(torch.equal(outs[h], outs[SPLITS[0]])) for h in SPLITS)
        del outs
        sweep(name, fn, nbytes, {"kernel": kern[SPLITS[0]], "identical": ident,
                                 "same_kernel": len(set(kern.values())) == 1})
        if not ident:
            bad.append(name)
    assert not bad, f"a window map changed an output: {bad}"


def main():
    try:
        if args.stage in ("probe", "all"):
            probe_stage()
        if args.stage in ("product", "all"):
            product_stage()
    finally:
        os.environ.pop("HRS_WINDOW_SPLIT", None)


if __name__ == "__main__":
    main()
