"""Checked repair timing (hrs_repair_checked_dev) against the scrub it starts
with and against the route through the existing entry points that it
replaces, one JSON line (DESIGN.md §10.5,
profiles/repair_checked/bench_repair_checked.json).

RS(10,4), 1 MiB cells, 1,024 stripes, device-resident; one lost cell (filled
with 0xA5) in each of d stripes spread over the batch, d in {0, 8, 1024},
planted again, untimed, before every repetition of every leg. Per d, in one
process, the legs alternate repetition by repetition; per leg the median of
--reps (>= 20) after warm-up with [min, max].

  (a) hrs_scrub_crc_dev alone: the floor. HIP events.
  (b) today's route: scrub_stripes_crc, checksums_to_erased (its copies to the
      host and its host loop; the stored checksums wait on the host),
      heal_erased_stripes_crc over all stripes, the compare of the CRCs with
      the stored ones on the device, its result read back. Host clock, from a
      synchronised device to the result on the host.
  (c) hrs_repair_checked_dev, checksums alone. HIP events ("c_repair_checked"),
      and the same call on the host clock from a synchronised device to a
      synchronised device ("c_host_clock"), the figure to hold against (b).

After the timing the results of every leg are checked on a sample of stripes:
(a)'s CRCs against zlib, (b)'s bytes against the clean stripes, (c)'s bytes,
verdicts, erased sets, reports and CRCs against hrs_repair_checked_host.

  python tools/bench_repair_checked.py [--stripes 1024] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, P = 10, 4
N = K + P


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def apart(fast, slow):
    """fast's whole [min, max] lies below slow's."""
    return fast["max_ms"] < slow["min_ms"]


def bench(args):
    import numpy as np
    import torch
    from lambdafs_amd import HipReedSolomonCode, device

    L, S = args.cell, args.stripes
    code = HipReedSolomonCode(K, P)
    hcode = HipReedSolomonCode(K, P, device=-2)  # host-only: the reference
    torch.manual_seed(31)
    st = torch.randint(0, 256, (S, N, L), dtype=torch.uint8, device="cuda")
    device.encode_stripes(code, st)
    stored = device.crc32_rows(code, [st[:, l, :] for l in range(N)])
    stored_host = stored.cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()
    results = {}
    for d in args.damaged:
        d = min(d, S)
        hit_host = (np.arange(d) * S // max(d, 1)).astype(np.int64)  # spread over the batch
        lost_host = np.random.default_rng(7 + d).integers(0, N, d)
        hit, lost = torch.from_numpy(hit_host).to("cuda"), torch.from_numpy(lost_host).to("cuda")
        keep = st[hit, lost].clone()  # the lost cells, to check against and to clear the damage

        def plant():
            if d:
                st[hit, lost] = 0xA5

        def leg_a():
            return device.scrub_stripes_crc(code, st)

        def leg_b():
            r1, c1 = device.scrub_stripes_crc(code, st)
            erased = device.checksums_to_erased(c1, stored_host, P)
            r2, c2 = device.heal_erased_stripes_crc(code, st, erased)
            return bool((c2 == stored).all().item())

        def leg_c():
            return device.repair_checked_stripes(code, st, stored)

        def host_clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def events(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            return a, b

        for _ in range(args.warmup):
            for fn in (leg_a, leg_b, leg_c):
                plant()
                fn()
        torch.cuda.synchronize()
        ev = {"a_scrub_crc": [], "c_repair_checked": []}
        ms = {"b_todays_route": [], "c_host_clock": []}
        for _ in range(args.reps):
            plant()
            ev["a_scrub_crc"].append(events(leg_a))
            plant()
            ms["b_todays_route"].append(host_clock(leg_b))
            plant()
            ev["c_repair_checked"].append(events(leg_c))
            plant()
            ms["c_host_clock"].append(host_clock(leg_c))
        torch.cuda.synchronize()
        legs = {name: stats([a.elapsed_time(b) for a, b in v]) for name, v in ev.items()}
        legs.update({name: stats(v) for name, v in ms.items()})

        # ---- every leg's results on a sample of stripes
        sample = sorted(set(hit_host[:3].tolist() + hit_host[-1:].tolist() + [1, S - 1]))
        plant()
        rep, crc = leg_a()
        crc = crc.cpu().numpy().view(np.uint32)
        for s in sample:
            for l in (0, N - 1) + tuple(lost_host[hit_host == s].tolist()):
                assert crc[s, l] == zlib.crc32(st[s, l].cpu().numpy().tobytes()), "scrub CRC differs from zlib"
        before = {s: st[s].cpu().numpy() for s in sample}
        assert leg_b(), "today's route did not restore the stored checksums"
        if d:
            assert torch.equal(st[hit, lost], keep), "today's route did not rebuild the lost cells"
        plant()
        verdicts, erased, reports, crcs = leg_c()
        kernel = code.lastKernel()
        torch.cuda.synchronize()
        v = verdicts.cpu().numpy()
        assert int((v == device.REPAIR_REPAIRED).sum()) == d and int((v == device.REPAIR_CLEAN).sum()) == S - d
        if d:
            assert torch.equal(st[hit, lost], keep), "checked repair did not rebuild the lost cells"
        for s in sample:
            rows = [np.ascontiguousarray(before[s][l]) for l in range(N)]
            hv, he, hr, hc = device.repair_checked_host(hcode, rows, stored_host[s])
            assert hv == v[s] and he.tolist() == erased[s].cpu().numpy().tolist()
            assert (hr == reports[s].cpu().numpy().view(np.uint32)).all()
            assert (hc == crcs[s].cpu().numpy().view(np.uint32)).all()
            assert (np.stack(rows) == st[s].cpu().numpy()).all(), "bytes differ from hrs_repair_checked_host"
        a, b, c, ch = (legs[x] for x in ("a_scrub_crc", "b_todays_route", "c_repair_checked", "c_host_clock"))
        results[str(d)] = {
            "legs": legs,
            "c_below_b_ranges_apart": apart(ch, b),
            "c_host_clock_over_b": round(ch["median_ms"] / b["median_ms"], 4),
            "c_over_a": round(c["median_ms"] / a["median_ms"], 4),
            "sample_checked": sample,
        }
    line = json.dumps({"bench": "repair_checked", "k": K, "p": P, "cell": L, "stripes": S, "bytes": N * L * S,
                       "reps": args.reps, "date": time.strftime("%Y-%m-%d"), "pass_1_kernel": kernel,
                       "damaged_stripes": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=1024)
    ap.add_argument("--cell", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--damaged", type=int, nargs="+", default=[0, 8, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_checked", "bench_repair_checked.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    bench(a)
