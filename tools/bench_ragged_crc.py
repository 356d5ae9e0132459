"""The ragged encode with block CRC-32s (hrs_encode_ragged_crc_dev,
hrs_encode_ragged_batch_host_crc) against the only route there was, the plain
encode + CRC over zero-filled stripes. The figures of DESIGN.md §12.1
(profiles/ragged_crc/bench_ragged_crc.json, pmc_fetch.json).

  bench  device-resident: RS(10,4), 1 MiB cells, 1,024 stripes, the first m
         cells of every stripe full and the rest empty, m in 10, 7, 5, 3, 1.
         Leg a: hrs_encode_crc_dev over the zero-filled stripes. Leg b: the
         new call over stripes whose empty cells hold 0xEE bytes (kernel mode
         3 at m = 10, where mode 0 would run leg a's kernel). Leg c: the new
         call's two-pass route (kernel mode 1). Device events.
         host batches: RS(10,4), 256 KiB cells, 512 stripes, pinned and
         pageable, m in 10, 5, 1: hrs_encode_batch_host_crc over zero-filled
         stripes against the new call (host clock; the calls are synchronous).
         Rates over the bytes that cross the link: 14 L against (m + 4) L per
         stripe.
         The legs alternate call by call in one process; each figure is the
         median of --reps calls after warm-up, with [min, max]. After timing,
         the ragged legs' parity and CRCs are compared with leg a's.
  pmc-run / pmc-parse  HBM read bytes of encode_ragged_crc_kernel at m = 5 from
         a rocprofv3 counter pass of its own (no tracing beside it), against
         the sum over cells of `valid` rounded up to 2 KiB; FETCH_SIZE in KiB,
         doubled, as tools/pmc_traffic.py does.

  python3 tools/bench_ragged_crc.py bench [--reps 20] [--out FILE]
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d <dir> -o run -- python3 tools/bench_ragged_crc.py pmc-run
  python3 tools/bench_ragged_crc.py pmc-parse <dir> <out.json>
  (a trailing `plain` on both: the plain fused kernel over the same shape, all k rows read)
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
TAIL = 0xEE  # what the unused cells of the ragged legs hold
DEFAULT_OUT = os.path.join(ROOT, "profiles", "ragged_crc", "bench_ragged_crc.json")


def stats(ms, nbytes):
    med = float(np.median(ms))
    return {"ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4),
            "GiBps": round(nbytes / GiB / (med * 1e-3), 2)}


def valid_for(m, S, L):
    return np.array([[L] * m + [0] * (K - m)] * S, np.uint32)


def device_legs(torch, reps, L=1 << 20, S=1024):
    from lambdafs_amd import HipReedSolomonCode, device
    plain, ragged, ragged3, two_pass = (HipReedSolomonCode(K, P, device=0) for _ in range(4))
    ragged3.setKernelMode(3)
    two_pass.setKernelMode(1)
    torch.manual_seed(11)
    a = torch.randint(1, 256, (S, N, L), dtype=torch.uint8, device="cuda")
    b = a.clone()
    c = a.clone()
    out = {"workload": f"RS({K},{P}) {L >> 20} MiB cells x {S} stripes, device-resident", "legs": {}}
    for m in (10, 7, 5, 3, 1):
        a[:, P + m:] = 0     # the parent's route: the zero fill is stored, read and checksummed
        b[:, P + m:] = TAIL  # the ragged routes must not look at it
        c[:, P + m:] = TAIL
        valid = valid_for(m, S, L)
        code_b = ragged3 if m == K else ragged
        calls = (lambda: device.encode_stripes_crc(plain, a),
                 lambda: device.encode_stripes_ragged_crc(code_b, b, valid),
                 lambda: device.encode_stripes_ragged_crc(two_pass, c, valid))
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in calls]
        ms = tuple([] for _ in calls)
        crcs = [None] * len(calls)
        for r in range(reps + 3):
            for leg, fn in enumerate(calls):
                ev[leg][0].record()
                crcs[leg] = fn()
                ev[leg][1].record()
            torch.cuda.synchronize()
            if r >= 3:
                for leg in range(len(calls)):
                    ms[leg].append(ev[leg][0].elapsed_time(ev[leg][1]))
        for name, t, crc in (("fused", b, crcs[1]), ("two-pass", c, crcs[2])):
            if not torch.equal(a[:, :P], t[:, :P]):
                raise RuntimeError(f"device m={m}: the {name} leg's parity differs from the plain leg's")
            if not torch.equal(crcs[0], crc):
                raise RuntimeError(f"device m={m}: the {name} leg's CRCs differ from the plain leg's")
            if not bool((t[:, P + m:] == TAIL).all()):
                raise RuntimeError(f"device m={m}: the {name} leg wrote a data cell")
        ra = stats(ms[0], N * L * S)
        rb, rc = stats(ms[1], (m + P) * L * S), stats(ms[2], (m + P) * L * S)
        out["legs"][f"m{m}"] = {
            "plain": dict(ra, kernel=plain.lastKernel(), bytes=N * L * S),
            "ragged": dict(rb, kernel=code_b.lastKernel(), bytes=(m + P) * L * S),
            "two_pass": dict(rc, kernel=two_pass.lastKernel(), bytes=(m + P) * L * S),
            "ragged_over_plain_ms": round(rb["ms"] / ra["ms"], 4),
            "two_pass_over_plain_ms": round(rc["ms"] / ra["ms"], 4),
            "ragged_range_below_plain_range": rb["max_ms"] < ra["min_ms"],
            "two_pass_beats_ragged": rc["ms"] < rb["ms"],
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
    crc_a, crc_b = np.zeros((S, N), np.uint32), np.zeros((S, N), np.uint32)
    out = {"workload": f"RS({K},{P}) {L >> 10} KiB cells x {S} stripes, host batches", "legs": {}}
    for memory in ("pinned", "pageable"):
        if memory == "pinned":
            pin_a.copy_(torch.from_numpy(base))
            pin_b.copy_(torch.from_numpy(base))
            a, b = pin_a.numpy(), pin_b.numpy()
            arg_a, arg_b = pin_a, pin_b
        else:
            a, b = base.copy(), base.copy()
            arg_a, arg_b = a, b
        for m in (10, 5, 1):
            a[:, P + m:] = 0
            b[:, P + m:] = TAIL
            valid = valid_for(m, S, L)
            code_b = ragged3 if m == K else ragged
            ms = ([], [])
            for r in range(reps + 2):
                for leg, fn in enumerate((lambda: device.encode_batch_host_crc(plain, arg_a, crc_out=crc_a),
                                          lambda: device.encode_batch_host_ragged_crc(code_b, arg_b, valid,
                                                                                      crc_out=crc_b))):
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if r >= 2:
                        ms[leg].append(dt)
            if not np.array_equal(a[:, :P], b[:, :P]):
                raise RuntimeError(f"host {memory} m={m}: the ragged parity differs from the plain leg's")
            if not np.array_equal(crc_a, crc_b):
                raise RuntimeError(f"host {memory} m={m}: the ragged CRCs differ from the plain leg's")
            if not bool((b[:, P + m:] == TAIL).all()):
                raise RuntimeError(f"host {memory} m={m}: the ragged call wrote a data cell")
            ra, rb = stats(ms[0], N * L * S), stats(ms[1], (m + P) * L * S)
            key = f"{memory}_m{m}"
            out["legs"][key] = {
                "plain": dict(ra, path=plain.lastHostPath(), kernel=plain.lastKernel(), link_bytes=N * L * S),
                "ragged": dict(rb, path=code_b.lastHostPath(), kernel=code_b.lastKernel(), link_bytes=(m + P) * L * S),
                "ragged_over_plain_ms": round(rb["ms"] / ra["ms"], 4),
            }
            print(f"host {key}", json.dumps(out["legs"][key]), flush=True)
    return out


PMC_M, PMC_L, PMC_S = 5, 1 << 20, 1024
PMC_KERNEL = "encode_ragged_crc_kernel"


PMC_PLAIN = "encode_crc_grouped_kernel"


def pmc_run(plain):
    """Three dispatches of the ragged fused kernel at m = 5, or (plain) of the
    plain fused kernel over the same shape, which reads all k rows."""
    import torch
    from lambdafs_amd import HipReedSolomonCode, device
    code = HipReedSolomonCode(K, P, device=0)
    torch.manual_seed(11)
    st = torch.randint(1, 256, (PMC_S, N, PMC_L), dtype=torch.uint8, device="cuda")
    valid = valid_for(PMC_M, PMC_S, PMC_L)
    for _ in range(3):
        if plain:
            device.encode_stripes_crc(code, st)
        else:
            device.encode_stripes_ragged_crc(code, st, valid)
    torch.cuda.synchronize()
    print("kernel", code.lastKernel())


def pmc_parse(path, out, plain):
    kernel = PMC_PLAIN if plain else PMC_KERNEL
    vals = []
    for f in glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if row["Counter_Name"] == "FETCH_SIZE" and kernel in row["Kernel_Name"]:
                    vals.append(float(row["Counter_Value"]))
    if not vals:
        sys.exit(f"no {kernel} dispatch with FETCH_SIZE under {path}")
    # every valid is 0 or L: already whole 2 KiB windows; the plain kernel reads all k rows
    want = (K if plain else PMC_M) * PMC_L * PMC_S
    res = {"kernel": kernel, "m": PMC_M, "dispatches": len(vals), "FETCH_SIZE_KiB": vals,
           "read_bytes_x2": [2 * v * 1024 for v in vals], "valid_window_bytes": want,
           "plain_read_bytes": K * PMC_L * PMC_S, "ratio": [2 * v * 1024 / want for v in vals]}
    line = json.dumps(res)
    print(line)
    with open(out, "w") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["bench", "pmc-run", "pmc-parse"])
    ap.add_argument("rest", nargs="*")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (its figures mean nothing)")
    args = ap.parse_args()
    plain = args.rest[-1:] == ["plain"]
    if args.what == "pmc-run":
        return pmc_run(plain)
    if args.what == "pmc-parse":
        if len(args.rest) != 2 + plain:
            sys.exit(__doc__)
        return pmc_parse(args.rest[0], args.rest[1], plain)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ragged_crc.py measures on a HIP device and there is none")
    small = dict(L=8192, S=8) if args.small else {}
    res = {"tool": "tools/bench_ragged_crc.py", "reps": args.reps, "device": device_legs(torch, args.reps, **small),
           "host": host_legs(torch, args.reps, **small)}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
