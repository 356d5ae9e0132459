"""The ragged repair + CRC-32 (hrs_decode_batch_ragged_crc_dev,
hrs_decode_batch_ragged_host_crc): its fused and two-pass routes against the
ragged repair alone (the floor) and against what a caller could run before,
the plain repair + CRC batch over zero-filled stripes. The figures of
DESIGN.md §13.1 (profiles/ragged_repair_crc/bench_ragged_repair_crc.json).

Every stripe lost data cell 0 (hops location p); the first m data cells of
every stripe are full and the rest empty (a file tail), as in
tools/bench_ragged_repair.py.

  device-resident: RS(10,4), 1 MiB cells, 1,024 stripes, m in 10, 5, 1. Legs,
    alternating call by call in one process, HIP events, the median of --reps
    calls after warm-up with [min, max]:
      a  hrs_decode_batch_ragged_dev alone (kernel mode 3 so that m = 10 stays
         on the ragged kernel): the floor
      b  the new call, fused (kernel mode 3)
      c  the new call, two passes (kernel mode 1; at m = 10 a cell of stripe 0
         that is neither read nor lost is one byte short, so the batch is not
         all-full and stays on the ragged route)
      d  hrs_decode_batch_crc_dev over the zero-filled stripes: a yardstick for
         time only, its CRCs cover len bytes
    and one more leg pair at m = 10 with the lost cell of half length (b_half,
    c_half).
  host batches: RS(10,4), 256 KiB cells, 512 stripes, pinned and pageable,
    m in 10, 5, 1: hrs_decode_batch_host_crc over zero-filled stripes against
    the new call (host clock; the calls are synchronous).
  After timing, every leg's bytes are compared with leg a's and its CRCs with
  zlib over a sample of cells (every leg's first, middle and last stripe).

  python3 tools/bench_ragged_repair_crc.py [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, P = 10, 4
N = K + P
GiB = float(1 << 30)
TAIL = 0xEE  # what the empty cells of the ragged legs hold


def stats(ms):
    return {"ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4)}


def valid_for(m, S, L, out_len=None):
    """[S, n] in hops order: the parity cells and the first m data cells full, the rest empty."""
    v = np.array([[L] * P + [L] * m + [0] * (K - m)] * S, np.uint32)
    if out_len is not None:
        v[:, P] = out_len  # the lost cell
    return v


def erased_for(S):
    return np.full((S, 1), P, np.int32)  # data cell 0


def check_crcs(what, out, crc, lens, sample):
    """zlib over the sampled stripes' rebuilt cells, exactly lens[s] bytes each."""
    for s in sample:
        want = zlib.crc32(bytes(out[s, 0, :int(lens[s])].cpu().numpy() if hasattr(out, "cpu") else out[s, 0, :int(lens[s])]))
        got = int(crc[s, 0]) & 0xFFFFFFFF
        if got != want:
            raise RuntimeError(f"{what}: stripe {s} CRC {got:#010x}, zlib {want:#010x}")


def device_legs(torch, reps, L=1 << 20, S=1024):
    from lambdafs_amd import HipReedSolomonCode, device
    floor, fused, two, plain = (HipReedSolomonCode(K, P, device=0) for _ in range(4))
    floor.setKernelMode(3)
    fused.setKernelMode(3)
    two.setKernelMode(1)
    torch.manual_seed(11)
    z = torch.randint(1, 256, (S, N, L), dtype=torch.uint8, device="cuda")  # leg d: zero-filled
    r = z.clone()                                                          # the ragged legs: TAIL behind the lengths
    outs = {k: torch.zeros((S, 1, L), dtype=torch.uint8, device="cuda") for k in "abcd"}
    erased = erased_for(S)
    sample = sorted({0, S // 2, S - 1})
    res = {"workload": f"RS({K},{P}) {L >> 10} KiB cells x {S} stripes, data cell 0 lost, device-resident",
           "legs": {}}
    for m, out_len in ((10, None), (5, None), (1, None), (10, L // 2)):
        z[:, P + m:] = 0
        r[:, P + m:] = TAIL
        valid = valid_for(m, S, L, out_len)
        valid_c = valid.copy()
        valid_c[0, 0] -= 1  # location 0 (a parity cell the plan does not read): keeps mode 1 on the ragged route
        crcs = {}
        legs = {
            "a": lambda: device.decode_batch_ragged(floor, r, erased, outs["a"], valid),
            "b": lambda: crcs.__setitem__("b", device.decode_batch_ragged_crc(fused, r, erased, outs["b"], valid)),
            "c": lambda: crcs.__setitem__("c", device.decode_batch_ragged_crc(two, r, erased, outs["c"], valid_c)),
            "d": lambda: crcs.__setitem__("d", device.decode_batch_crc(plain, z, erased, outs["d"])),
        }
        if out_len is not None:
            del legs["d"]  # no plain form of a short output
        codes = {"a": floor, "b": fused, "c": two, "d": plain}
        kernels = {}
        ev = {k: [torch.cuda.Event(enable_timing=True) for _ in range(2)] for k in legs}
        ms = {k: [] for k in legs}
        for o in outs.values():
            o.zero_()
        for rep in range(reps + 3):
            for k, fn in legs.items():
                ev[k][0].record()
                fn()
                ev[k][1].record()
                kernels[k] = codes[k].lastKernel()
            torch.cuda.synchronize()
            if rep >= 3:
                for k in legs:
                    ms[k].append(ev[k][0].elapsed_time(ev[k][1]))
        lens = valid[:, P]
        for k in legs:
            if k != "a" and not torch.equal(outs[k], outs["a"]):
                raise RuntimeError(f"device m={m}: leg {k}'s outputs differ from leg a's")
            if k in "bc":
                check_crcs(f"device m={m} leg {k}", outs[k], crcs[k].cpu().numpy(), lens, sample)
        if "d" in legs:
            check_crcs(f"device m={m} leg d", outs["d"], crcs["d"].cpu().numpy(), np.full(S, L), sample)
        if not bool((r[:, P + m:] == TAIL).all()):
            raise RuntimeError(f"device m={m}: a ragged call wrote a survivor")
        st = {k: dict(stats(ms[k]), kernel=kernels[k]) for k in legs}
        key = f"m{m}" + ("" if out_len is None else "_half_output")
        leg = {"legs": st, "b_over_c": round(st["b"]["ms"] / st["c"]["ms"], 4),
               "b_over_a": round(st["b"]["ms"] / st["a"]["ms"], 4),
               "b_range_above_c_range": st["b"]["min_ms"] > st["c"]["max_ms"]}
        if "d" in st:
            leg["b_over_d"] = round(st["b"]["ms"] / st["d"]["ms"], 4)
        res["legs"][key] = leg
        print(f"device {key}", json.dumps(leg), flush=True)
    return res


def host_legs(torch, reps, L=256 << 10, S=512):
    from lambdafs_amd import HipReedSolomonCode, device
    plain, ragged = (HipReedSolomonCode(K, P, device=0) for _ in range(2))
    ragged.setKernelMode(3)
    base = np.random.default_rng(12).integers(1, 256, (S, N, L), dtype=np.uint8)
    pins = [torch.empty((S, N, L), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    pouts = [torch.empty((S, 1, L), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    erased = erased_for(S)
    sample = sorted({0, S // 2, S - 1})
    res = {"workload": f"RS({K},{P}) {L >> 10} KiB cells x {S} stripes, data cell 0 lost, host batches", "legs": {}}
    for memory in ("pinned", "pageable"):
        if memory == "pinned":
            for p in pins:
                p.copy_(torch.from_numpy(base))
            a, b, oa, ob = pins[0].numpy(), pins[1].numpy(), pouts[0].numpy(), pouts[1].numpy()
            args_a, args_b = (pins[0], erased, pouts[0]), (pins[1], erased, pouts[1])
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
            crcs = {}
            ms = ([], [])
            for rep in range(reps + 2):
                for leg, fn in enumerate((
                        lambda: crcs.__setitem__(0, device.decode_batch_host_crc(plain, *args_a)),
                        lambda: crcs.__setitem__(1, device.decode_batch_host_ragged_crc(ragged, *args_b, valid)))):
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep >= 2:
                        ms[leg].append(dt)
            if not np.array_equal(oa, ob):
                raise RuntimeError(f"host {memory} m={m}: the ragged outputs differ from the plain leg's")
            if not bool((b[:, P + m:] == TAIL).all()):
                raise RuntimeError(f"host {memory} m={m}: the ragged call wrote a survivor")
            for leg, o in ((0, oa), (1, ob)):
                check_crcs(f"host {memory} m={m} leg {leg}", o, crcs[leg], np.full(S, L), sample)
            ra, rb = stats(ms[0]), stats(ms[1])
            key = f"{memory}_m{m}"
            res["legs"][key] = {
                "plain_crc": dict(ra, path=plain.lastHostPath(), kernel=plain.lastKernel()),
                "ragged_crc": dict(rb, path=ragged.lastHostPath(), kernel=ragged.lastKernel()),
                "ragged_over_plain_ms": round(rb["ms"] / ra["ms"], 4),
            }
            print(f"host {key}", json.dumps(res["legs"][key]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (its figures mean nothing)")
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ragged_repair_crc.py measures on a HIP device and there is none")
    small = dict(L=8192, S=8) if args.small else {}
    res = {"tool": "tools/bench_ragged_repair_crc.py", "reps": args.reps, "device": device_legs(torch, args.reps, **small)}
    if not args.skip_host:
        res["host"] = host_legs(torch, args.reps, **small)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
