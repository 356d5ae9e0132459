"""The ragged scrub and heal (hrs_scrub_ragged_dev, hrs_heal_ragged_dev,
hrs_scrub_ragged_batch_host) against today's route, hrs_scrub_dev /
hrs_scrub_batch_host over zero-filled stripes. The figures of DESIGN.md §14
(profiles/ragged_scrub/bench_ragged_scrub.json, pmc_fetch.json).

The stripes are clean codewords of a file tail: the parity cells and the first
m data cells of every stripe are full, the other data cells empty.

  bench  device-resident: RS(10,4), 1 MiB cells, 1,024 stripes, m in 10, 7, 5,
         3, 1. Leg a: hrs_scrub_dev over the zero-filled stripes (the
         yardstick). Leg b: the ragged scrub over stripes whose empty cells hold
         0xEE bytes (kernel mode 3 at m = 10, where mode 0 would run leg a's
         kernel). At m = 5 also leg c, the ragged heal. Device events.
         host batches: RS(10,4), 256 KiB cells, 512 stripes, pinned and
         pageable, m in 10, 5, 1: hrs_scrub_batch_host over zero-filled stripes
         against the ragged call (host clock; the calls are synchronous). Rates
         in bytes that cross the link: 14 L against (4 + m) L per stripe.
         The legs alternate call by call in one process; each figure is the
         median of --reps calls after warm-up, with [min, max]. Every report of
         every leg must be the clean report, and the empty cells must still
         hold their 0xEE.
  pmc-run / pmc-parse  HBM read bytes of scrub_ragged_kernel<4> at m = 5 from a
         rocprofv3 counter pass of its own (no tracing beside it), against the
         sum of the lengths rounded up to 2 KiB; FETCH_SIZE in KiB, doubled, as
         tools/pmc_traffic.py does.

  python3 tools/bench_ragged_scrub.py bench [--reps 20] [--out FILE]
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d <dir> -o run -- python3 tools/bench_ragged_scrub.py pmc-run
  python3 tools/bench_ragged_scrub.py pmc-parse <dir> <out.json>
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, P = 10, 4
N = K + P
GiB = float(1 << 30)
TAIL = 0xEE  # what the empty cells of the ragged legs hold
NONE = 0xFFFFFFFF


def stats(ms, nbytes):
    med = float(np.median(ms))
    return {"ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4),
            "GiBps": round(nbytes / GiB / (med * 1e-3), 2)}


def valid_for(m, S, L):
    """[S, n] in hops order: the parity cells and the first m data cells full, the rest empty."""
    return np.array([[L] * P + [L] * m + [0] * (K - m)] * S, np.uint32)


def all_clean(rep):
    rep = np.asarray(rep).astype(np.int64) & 0xFFFFFFFF
    want = np.zeros_like(rep)
    want[:, 2] = NONE
    return bool((rep == want).all())


def device_legs(torch, reps, L=1 << 20, S=1024):
    from lambdafs_amd import HipReedSolomonCode, device
    plain, ragged, ragged3 = (HipReedSolomonCode(K, P, device=0) for _ in range(3))
    ragged3.setKernelMode(3)
    torch.manual_seed(11)
    a = torch.randint(1, 256, (S, N, L), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    out = {"workload": f"RS({K},{P}) {L >> 10} KiB cells x {S} stripes, clean, device-resident", "legs": {}}
    for m in (10, 7, 5, 3, 1):
        a[:, P + m:] = 0     # today's route: the zero fill is stored and read
        device.encode_stripes(plain, a)
        b.copy_(a)
        b[:, P + m:] = TAIL  # the ragged route must not look at it
        valid = valid_for(m, S, L)
        code_b = ragged3 if m == K else ragged
        fns = [lambda: device.scrub_stripes(plain, a), lambda: device.scrub_stripes_ragged(code_b, b, valid)]
        if m == 5:
            fns.append(lambda: device.heal_stripes_ragged(code_b, b, valid))
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in fns]
        ms = [[] for _ in fns]
        kernels = [None] * len(fns)
        for r in range(reps + 3):
            reports = []
            for leg, fn in enumerate(fns):
                ev[leg][0].record()
                reports.append(fn())
                ev[leg][1].record()
                kernels[leg] = (plain if leg == 0 else code_b).lastKernel()
            torch.cuda.synchronize()
            if r >= 3:
                for leg in range(len(fns)):
                    ms[leg].append(ev[leg][0].elapsed_time(ev[leg][1]))
        for leg, rep in enumerate(reports):
            if not all_clean(rep.cpu().numpy()):
                raise RuntimeError(f"device m={m} leg {leg}: a report is not the clean report")
        if not bool((b[:, P + m:] == TAIL).all()):
            raise RuntimeError(f"device m={m}: a ragged call wrote an empty cell")
        ra, rb = stats(ms[0], N * L * S), stats(ms[1], (P + m) * L * S)
        res = {
            "plain": dict(ra, kernel=kernels[0], bytes=N * L * S),
            "ragged": dict(rb, kernel=kernels[1], bytes=(P + m) * L * S),
            "bytes_ratio": round((P + m) / N, 4),
            "ragged_over_plain_ms": round(rb["ms"] / ra["ms"], 4),
            "ragged_range_below_plain_min": rb["max_ms"] < ra["min_ms"],
        }
        if m == 5:
            res["ragged_heal"] = dict(stats(ms[2], (P + m) * L * S), kernel=kernels[2])
        out["legs"][f"m{m}"] = res
        print(f"device m={m}", json.dumps(res), flush=True)
    return out


def host_legs(torch, reps, L=256 << 10, S=512):
    from lambdafs_amd import HipReedSolomonCode, device
    plain, ragged, ragged3 = (HipReedSolomonCode(K, P, device=0) for _ in range(3))
    ragged3.setKernelMode(3)
    torch.manual_seed(12)
    dev = torch.randint(1, 256, (S, N, L), dtype=torch.uint8, device="cuda")
    pin_a = torch.empty((S, N, L), dtype=torch.uint8, pin_memory=True)
    pin_b = torch.empty((S, N, L), dtype=torch.uint8, pin_memory=True)
    out = {"workload": f"RS({K},{P}) {L >> 10} KiB cells x {S} stripes, clean, host batches", "legs": {}}
    for m in (10, 5, 1):
        dev[:, P + m:] = 0
        device.encode_stripes(plain, dev)
        base = dev.cpu().numpy()
        valid = valid_for(m, S, L)
        code_b = ragged3 if m == K else ragged
        for memory in ("pinned", "pageable"):
            if memory == "pinned":
                pin_a.copy_(torch.from_numpy(base))
                pin_b.copy_(torch.from_numpy(base))
                pin_b[:, P + m:] = TAIL
                arg_a, arg_b, b = pin_a, pin_b, pin_b.numpy()
            else:
                arg_a, b = base.copy(), base.copy()
                b[:, P + m:] = TAIL
                arg_b = b
            ms = ([], [])
            for r in range(reps + 2):
                reports = []
                for leg, fn in enumerate((lambda: device.scrub_batch_host(plain, arg_a),
                                          lambda: device.scrub_batch_host_ragged(code_b, arg_b, valid))):
                    t0 = time.perf_counter()
                    reports.append(fn())
                    dt = (time.perf_counter() - t0) * 1e3
                    if r >= 2:
                        ms[leg].append(dt)
            if not all(all_clean(rep) for rep in reports):
                raise RuntimeError(f"host {memory} m={m}: a report is not the clean report")
            if not bool((b[:, P + m:] == TAIL).all()):
                raise RuntimeError(f"host {memory} m={m}: the ragged call wrote an empty cell")
            ra, rb = stats(ms[0], N * L * S), stats(ms[1], (P + m) * L * S)
            key = f"{memory}_m{m}"
            out["legs"][key] = {
                "plain": dict(ra, path=plain.lastHostPath(), kernel=plain.lastKernel(), link_bytes=N * L * S),
                "ragged": dict(rb, path=code_b.lastHostPath(), kernel=code_b.lastKernel(),
                               link_bytes=(P + m) * L * S),
                "ragged_over_plain_ms": round(rb["ms"] / ra["ms"], 4),
            }
            print(f"host {key}", json.dumps(out["legs"][key]), flush=True)
    return out


PMC_M, PMC_L, PMC_S = 5, 1 << 20, 1024


def pmc_run():
    import torch
    from lambdafs_amd import HipReedSolomonCode, device
    code = HipReedSolomonCode(K, P, device=0)
    torch.manual_seed(11)
    st = torch.randint(1, 256, (PMC_S, N, PMC_L), dtype=torch.uint8, device="cuda")
    st[:, P + PMC_M:] = 0
    device.encode_stripes(code, st)
    st[:, P + PMC_M:] = TAIL
    valid = valid_for(PMC_M, PMC_S, PMC_L)
    for _ in range(3):
        rep = device.scrub_stripes_ragged(code, st, valid)
    torch.cuda.synchronize()
    if not all_clean(rep.cpu().numpy()):
        raise RuntimeError("a report is not the clean report")
    print("kernel", code.lastKernel())


def pmc_parse(path, out):
    vals = []
    for f in glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if row["Counter_Name"] == "FETCH_SIZE" and "scrub_ragged_kernel" in row["Kernel_Name"]:
                    vals.append(float(row["Counter_Value"]))
    if not vals:
        sys.exit(f"no scrub_ragged_kernel dispatch with FETCH_SIZE under {path}")
    want = (P + PMC_M) * PMC_L * PMC_S  # every length is 0 or L: already whole 2 KiB windows
    res = {"kernel": "scrub_ragged_kernel<4>", "m": PMC_M, "dispatches": len(vals), "FETCH_SIZE_KiB": vals,
           "read_bytes_x2": [2 * v * 1024 for v in vals], "valid_window_bytes": want,
           "plain_read_bytes": N * PMC_L * PMC_S, "ratio": [2 * v * 1024 / want for v in vals]}
    line = json.dumps(res)
    print(line)
    with open(out, "w") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["bench", "pmc-run", "pmc-parse"])
    ap.add_argument("rest", nargs="*")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (its figures mean nothing)")
    ap.add_argument("--device-only", action="store_true", help="skip the host batches")
    args = ap.parse_args()
    if args.what == "pmc-run":
        return pmc_run()
    if args.what == "pmc-parse":
        if len(args.rest) != 2:
            sys.exit(__doc__)
        return pmc_parse(*args.rest)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ragged_scrub.py measures on a HIP device and there is none")
    small = dict(L=8192, S=8) if args.small else {}
    res = {"tool": "tools/bench_ragged_scrub.py", "reps": args.reps, "device": device_legs(torch, args.reps, **small)}
    if not args.device_only:
        res["host"] = host_legs(torch, args.reps, **small)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
