"""The ragged repair (hrs_decode_batch_ragged_dev, hrs_decode_batch_ragged_host)
against today's route, the plain repair batch over zero-filled stripes. The
figures of DESIGN.md §13 (profiles/ragged_repair/bench_ragged_repair.json,
pmc_fetch.json).

Every stripe lost data cell 0 (hops location p), so locationsToReadForDecode
reads locations 13..5 and 3: nine data cells and one parity cell. The first m
data cells of every stripe are full and the rest empty (a file tail), so m of
the ten survivors hold bytes (the parity cell and data cells 1..m-1) and the
lost cell is full.

  bench  device-resident: RS(10,4), 1 MiB cells, 1,024 stripes, m in 10, 7, 5,
         3, 1. Leg a: hrs_decode_batch_dev over the zero-filled stripes. Leg b:
         the ragged call over stripes whose empty cells hold 0xEE bytes (kernel
         mode 3 at m = 10, where mode 0 would run leg a's kernel). Device
         events.
         host batches: RS(10,4), 256 KiB cells, 512 stripes, pinned and
         pageable, m in 10, 5, 1: hrs_decode_batch_host over zero-filled
         stripes against the ragged call (host clock; the calls are
         synchronous). Rates in bytes that cross the link: 11 L against
         (m + 1) L per stripe.
         The legs alternate call by call in one process; each figure is the
         median of --reps calls after warm-up, with [min, max]. After timing,
         the ragged leg's outputs are compared with the plain leg's bytes and
         its empty cells must still hold their 0xEE.
  pmc-run / pmc-parse  HBM read bytes of batch_ragged_kernel<1, 12> at m = 5
         from a rocprofv3 counter pass of its own (no tracing beside it), against
         the sum over the read survivors of their length rounded up to 2 KiB;
         FETCH_SIZE in KiB, doubled, as tools/pmc_traffic.py does.

  python3 tools/bench_ragged_repair.py bench [--reps 20] [--out FILE]
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d <dir> -o run -- python3 tools/bench_ragged_repair.py pmc-run
  python3 tools/bench_ragged_repair.py pmc-parse <dir> <out.json>
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
TAIL = 0xEE  # what the empty cells of the ragged leg hold
READ = 10    # survivors the plain leg reads per stripe


def stats(ms, nbytes):
    med = float(np.median(ms))
    return {"ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4),
            "GiBps": round(nbytes / GiB / (med * 1e-3), 2)}


def valid_for(m, S, L):
    """[S, n] in hops order: the parity cells and the first m data cells full, the rest empty."""
    return np.array([[L] * P + [L] * m + [0] * (K - m)] * S, np.uint32)


def erased_for(S):
    return np.full((S, 1), P, np.int32)  # data cell 0


def device_legs(torch, reps, L=1 << 20, S=1024):
    from lambdafs_amd import HipReedSolomonCode, device
    plain, ragged, ragged3 = (HipReedSolomonCode(K, P, device=0) for _ in range(3))
    ragged3.setKernelMode(3)
    torch.manual_seed(11)
    a = torch.randint(1, 256, (S, N, L), dtype=torch.uint8, device="cuda")
    b = a.clone()
    out_a = torch.empty((S, 1, L), dtype=torch.uint8, device="cuda")
    out_b = torch.empty((S, 1, L), dtype=torch.uint8, device="cuda")
    erased = erased_for(S)
    out = {"workload": f"RS({K},{P}) {L >> 20} MiB cells x {S} stripes, data cell 0 lost, device-resident", "legs": {}}
    for m in (10, 7, 5, 3, 1):
        a[:, P + m:] = 0     # today's route: the zero fill is stored and read
        b[:, P + m:] = TAIL  # the ragged route must not look at it
        valid = valid_for(m, S, L)
        code_b = ragged3 if m == K else ragged
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(2)]
        ms = ([], [])
        for r in range(reps + 3):
            for leg, fn in enumerate((lambda: device.decode_batch(plain, a, erased, out_a),
                                      lambda: device.decode_batch_ragged(code_b, b, erased, out_b, valid))):
                ev[leg][0].record()
                fn()
                ev[leg][1].record()
            torch.cuda.synchronize()
            if r >= 3:
                for leg in range(2):
                    ms[leg].append(ev[leg][0].elapsed_time(ev[leg][1]))
        if not torch.equal(out_a, out_b):
            raise RuntimeError(f"device m={m}: the ragged outputs differ from the plain leg's")
        if not bool((b[:, P + m:] == TAIL).all()):
            raise RuntimeError(f"device m={m}: the ragged call wrote a survivor")
        ra, rb = stats(ms[0], (READ + 1) * L * S), stats(ms[1], (m + 1) * L * S)
        out["legs"][f"m{m}"] = {
            "plain": dict(ra, kernel=plain.lastKernel(), bytes=(READ + 1) * L * S),
            "ragged": dict(rb, kernel=code_b.lastKernel(), bytes=(m + 1) * L * S),
            "ragged_over_plain_ms": round(rb["ms"] / ra["ms"], 4),
            "ragged_range_below_plain_range": rb["max_ms"] < ra["min_ms"],
        }
        print(f"device m={m}", json.dumps(out["legs"][f"m{m}"]), flush=True)
    return out


def host_legs(torch, reps, L=256 << 10, S=512):
    from lambdafs_amd import HipReedSolomonCode, device
    plain, ragged, ragged3 = (HipReedSolomonCode(K, P, device=0) for _ in range(3))
    ragged3.setKernelMode(3)
    base = np.random.default_rng(12).integers(1, 256, (S, N, L), dtype=np.uint8)
    pin_a = torch.empty((S, N, L), dtype=torch.uint8, pin_memory=True)
    pin_b = torch.empty((S, N, L), dtype=torch.uint8, pin_memory=True)
    pin_oa = torch.empty((S, 1, L), dtype=torch.uint8, pin_memory=True)
    pin_ob = torch.empty((S, 1, L), dtype=torch.uint8, pin_memory=True)
    erased = erased_for(S)
    out = {"workload": f"RS({K},{P}) {L >> 10} KiB cells x {S} stripes, data cell 0 lost, host batches", "legs": {}}
    for memory in ("pinned", "pageable"):
        if memory == "pinned":
            pin_a.copy_(torch.from_numpy(base))
            pin_b.copy_(torch.from_numpy(base))
            a, b, oa, ob = pin_a.numpy(), pin_b.numpy(), pin_oa.numpy(), pin_ob.numpy()
            args_a, args_b = (pin_a, erased, pin_oa), (pin_b, erased, pin_ob)
        else:
            a, b = base.copy(), base.copy()
            oa, ob = np.empty((S, 1, L), np.uint8), np.empty((S, 1, L), np.uint8)
            args_a, args_b = (a, erased, oa), (b, erased, ob)
        for m in (10, 5, 1):
            a[:, P + m:] = 0
            b[:, P + m:] = TAIL
            oa[...] = 0
            ob[...] = 1
            valid = valid_for(m, S, L)
            code_b = ragged3 if m == K else ragged
            ms = ([], [])
            for r in range(reps + 2):
                for leg, fn in enumerate((lambda: device.decode_batch_host(plain, *args_a),
                                          lambda: device.decode_batch_host_ragged(code_b, *args_b, valid))):
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if r >= 2:
                        ms[leg].append(dt)
            if not np.array_equal(oa, ob):
                raise RuntimeError(f"host {memory} m={m}: the ragged outputs differ from the plain leg's")
            if not bool((b[:, P + m:] == TAIL).all()):
                raise RuntimeError(f"host {memory} m={m}: the ragged call wrote a survivor")
            ra, rb = stats(ms[0], (READ + 1) * L * S), stats(ms[1], (m + 1) * L * S)
            key = f"{memory}_m{m}"
            out["legs"][key] = {
                "plain": dict(ra, path=plain.lastHostPath(), kernel=plain.lastKernel(), link_bytes=(READ + 1) * L * S),
                "ragged": dict(rb, path=code_b.lastHostPath(), kernel=code_b.lastKernel(),
                               link_bytes=(m + 1) * L * S),
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
    out = torch.empty((PMC_S, 1, PMC_L), dtype=torch.uint8, device="cuda")
    valid = valid_for(PMC_M, PMC_S, PMC_L)
    for _ in range(3):
        device.decode_batch_ragged(code, st, erased_for(PMC_S), out, valid)
    torch.cuda.synchronize()
    print("kernel", code.lastKernel())


def pmc_parse(path, out):
    vals = []
    for f in glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if row["Counter_Name"] == "FETCH_SIZE" and "batch_ragged_kernel" in row["Kernel_Name"]:
                    vals.append(float(row["Counter_Value"]))
    if not vals:
        sys.exit(f"no batch_ragged_kernel dispatch with FETCH_SIZE under {path}")
    want = PMC_M * PMC_L * PMC_S  # every length is 0 or L: already whole 2 KiB windows
    res = {"kernel": "batch_ragged_kernel<1, 12>", "m": PMC_M, "dispatches": len(vals), "FETCH_SIZE_KiB": vals,
           "read_bytes_x2": [2 * v * 1024 for v in vals], "valid_window_bytes": want,
           "plain_read_bytes": READ * PMC_L * PMC_S, "ratio": [2 * v * 1024 / want for v in vals]}
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
    args = ap.parse_args()
    if args.what == "pmc-run":
        return pmc_run()
    if args.what == "pmc-parse":
        if len(args.rest) != 2:
            sys.exit(__doc__)
        return pmc_parse(*args.rest)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ragged_repair.py measures on a HIP device and there is none")
    small = dict(L=8192, S=8) if args.small else {}
    res = {"tool": "tools/bench_ragged_repair.py", "reps": args.reps, "device": device_legs(torch, args.reps, **small),
           "host": host_legs(torch, args.reps, **small)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
