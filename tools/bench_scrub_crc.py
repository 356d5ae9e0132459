"""Scrub / heal + CRC-32 timing (hrs_scrub_crc_dev, hrs_heal_crc_dev,
hrs_scrub_batch_host_crc) against what the calls without CRCs already do, one
JSON line (profiles/scrub/bench_scrub_crc.json).

Every comparison runs in one process with its legs alternating repetition by
repetition; per leg the median of --reps (>= 20) after warm-up with [min, max].
Device legs are timed with HIP events, the synchronous host calls with the
host clock.

  device, RS(10,4), 1 MiB cells, 1,024 clean stripes (14 GiB per pass):
    (a) hrs_scrub_dev
    (b) hrs_scrub_dev, then hrs_crc32_dev over the 14 rows: the two-pass baseline
    (c) hrs_scrub_crc_dev, with the 1,024-thread blocks and (c512) the 512-thread ones
  heal: hrs_heal_crc_dev over clean stripes beside the same stripes with one
    single-byte error each (planted again before every repetition, untimed)
  host, pinned, RS(12,4), 256 KiB cells, 256 clean stripes:
    hrs_scrub_batch_host, hrs_scrub_batch_host_crc, and the plain scrub plus a
    second zero-copy read of the same bytes (hrs_crc32_dev over the pinned
    stripes' device addresses where the runtime maps them, else a second
    hrs_scrub_batch_host; "second_read" says which)

  python tools/bench_scrub_crc.py [--stripes 1024] [--reps 20] [--out FILE]

Profiler runs, each in a run of its own (profiles/run_rocprof.sh):

  rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -o run -- python3 tools/bench_scrub_crc.py pmc-run
  python3 tools/bench_scrub_crc.py pmc-parse DIR profiles/scrub/pmc_fetch_scrub_crc.json
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/bench_scrub_crc.py trace-run
  python3 tools/bench_scrub_crc.py trace-parse DIR profiles/scrub/heal_crc_trace.json
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, P = 10, 4
N = K + P
PROFILE_STRIPES = 256  # 3.5 GiB: past the Infinity Cache


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def apart(fast, slow):
    """fast's whole [min, max] lies below slow's."""
    return fast["max_ms"] < slow["min_ms"]


def clean_stripes(torch, device, code, k, p, cell, stripes, seed):
    torch.manual_seed(seed)
    st = torch.randint(0, 256, (stripes, k + p, cell), dtype=torch.uint8, device="cuda")
    device.encode_stripes(code, st)
    return st


def plant(torch, st):
    """One single-byte error per stripe, each in another location and window."""
    s = torch.arange(st.shape[0], device=st.device)
    st[s, s % st.shape[1], (s * 2053 + 17) % st.shape[2]] ^= 0x5A


def bench(args):
    import numpy as np
    import torch
    from lambdafs_amd import HipReedSolomonCode, _lib, device

    def alternate(legs, before=None):
        """{name: stats} of the device legs, run in turn within each repetition."""
        for _ in range(args.warmup):
            for name, fn in legs.items():
                if before and name in before:
                    before[name]()
                fn()
        torch.cuda.synchronize()
        ev = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():
                if before and name in before:
                    before[name]()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        return {name: stats([a.elapsed_time(b) for a, b in v]) for name, v in ev.items()}

    L, S = args.cell, args.stripes
    code = HipReedSolomonCode(K, P)
    st = clean_stripes(torch, device, code, K, P, L, S, 23)
    rows = [st[:, l, :] for l in range(N)]
    rep, crc = device.scrub_stripes_crc(code, st)
    fused_kernel = code.lastKernel()
    assert int((rep[:, 0] != 0).sum()) == 0, "encoded stripes must scrub clean"
    assert torch.equal(crc, device.crc32_rows(code, rows)), "fused CRCs differ from hrs_crc32_dev"

    def fused(threads):
        def run():
            os.environ["HRS_SCRUB_CRC_THREADS"] = threads
            device.scrub_stripes_crc(code, st)
        return run

    dev = alternate({
        "a_scrub": lambda: device.scrub_stripes(code, st),
        "b_scrub_then_crc32": lambda: (device.scrub_stripes(code, st), device.crc32_rows(code, rows)),
        "c_scrub_crc": fused("1024"),
        "c512_scrub_crc": fused("512"),
    })
    os.environ["HRS_SCRUB_CRC_THREADS"] = "1024"
    heal = alternate({
        "heal_crc_clean": lambda: device.heal_stripes_crc(code, st),
        "heal_crc_one_error_per_stripe": lambda: device.heal_stripes_crc(code, st),
        "heal_clean": lambda: device.heal_stripes(code, st),
    }, before={"heal_crc_one_error_per_stripe": lambda: plant(torch, st)})
    plant(torch, st)
    rep, _ = device.heal_stripes_crc(code, st)
    heal_kernel = code.lastKernel()
    r = rep.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert (r[:, 0] == 1).all() and (r[:, 3] == 1).all(), "one error per stripe, each healed"
    del st, rows
    torch.cuda.empty_cache()

    # host batch from pinned memory
    hk, hp, hL, hS = 12, 4, args.host_cell, args.host_stripes
    hn = hk + hp
    hcode = HipReedSolomonCode(hk, hp)
    pinned = clean_stripes(torch, device, hcode, hk, hp, hL, hS, 29).cpu().pin_memory()
    torch.cuda.empty_cache()
    got = device.scrub_batch_host(hcode, pinned)
    mapped = hcode.lastHostPath() == "pinned"
    assert not got[:, 0].any(), "encoded host stripes must scrub clean"
    got, hcrc = device.scrub_batch_host_crc(hcode, pinned)
    host_kernel = hcode.lastKernel()
    assert not got[:, 0].any()
    ptrs = _lib.ptr_array([pinned.data_ptr() + l * pinned.stride(1) for l in range(hn)])
    dcrc = torch.empty((hS, hn), dtype=torch.int32, device="cuda")

    def second_read():
        if not mapped:
            device.scrub_batch_host(hcode, pinned)
            return
        hcode._check(_lib.lib().hrs_crc32_dev(hcode._handle(), ptrs, hn, pinned.stride(0), hL, hS, None,
                                              dcrc.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()

    def both():
        device.scrub_batch_host(hcode, pinned)
        second_read()

    hlegs = {"scrub_batch_host": lambda: device.scrub_batch_host(hcode, pinned),
             "scrub_batch_host_crc": lambda: device.scrub_batch_host_crc(hcode, pinned),
             "scrub_batch_host_then_second_read": both}
    for _ in range(args.warmup):
        for fn in hlegs.values():
            fn()
    if mapped:
        assert (dcrc.cpu().numpy().view(np.uint32) == hcrc).all(), "host CRCs differ from hrs_crc32_dev"
    hms = {name: [] for name in hlegs}
    for _ in range(args.reps):
        for name, fn in hlegs.items():
            t0 = time.perf_counter()
            fn()
            hms[name].append((time.perf_counter() - t0) * 1e3)
    host = {name: stats(v) for name, v in hms.items()}
    hbytes = hn * hL * hS
    plain, fusedh, twice = (host[x] for x in hlegs)

    nbytes = N * L * S
    a, b, c = dev["a_scrub"], dev["b_scrub_then_crc32"], dev["c_scrub_crc"]
    line = json.dumps({
        "bench": "scrub_crc", "k": K, "p": P, "cell": L, "stripes": S, "bytes_read": nbytes, "reps": args.reps,
        "kernel": fused_kernel, "heal_kernel": heal_kernel,
        "device": dev,
        "c_faster_than_b_ranges_apart": apart(c, b),
        "c_over_b": round(c["median_ms"] / b["median_ms"], 4),
        "c_over_a": round(c["median_ms"] / a["median_ms"], 4),
        "c_GBps": round(nbytes / (c["median_ms"] * 1e-3) / 1e9, 1),
        "heal": heal,
        "host": {"k": hk, "p": hp, "cell": hL, "stripes": hS, "bytes_moved": hbytes, "path": hcode.lastHostPath(),
                 "kernel": host_kernel, "second_read": "hrs_crc32_dev" if mapped else "hrs_scrub_batch_host",
                 "legs": host,
                 "crc_GiBps": round(hbytes / (fusedh["median_ms"] * 1e-3) / 2 ** 30, 2),
                 "plain_GiBps": round(hbytes / (plain["median_ms"] * 1e-3) / 2 ** 30, 2),
                 "crc_median_within_plain_max": fusedh["median_ms"] <= plain["max_ms"],
                 "crc_over_plain": round(fusedh["median_ms"] / plain["median_ms"], 4),
                 "crc_over_two_reads": round(fusedh["median_ms"] / twice["median_ms"], 4)},
    })
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def profile_run(heal):
    """The profiled program: three fused clean scrubs (counters), or three
    heals of stripes with one single-byte error each (kernel trace)."""
    import torch
    from lambdafs_amd import HipReedSolomonCode, device
    code = HipReedSolomonCode(K, P)
    st = clean_stripes(torch, device, code, K, P, 1 << 20, PROFILE_STRIPES, 3)
    for _ in range(3):
        if heal:
            plant(torch, st)
            rep, _ = device.heal_stripes_crc(code, st)
        else:
            rep, _ = device.scrub_stripes_crc(code, st)
    torch.cuda.synchronize()
    assert int((rep[:, 0] != 0).sum()) == (PROFILE_STRIPES if heal else 0)
    print("kernel", code.lastKernel(), "algorithmic_read_bytes", N * (1 << 20) * PROFILE_STRIPES)


def rows_of(path, pattern):
    for f in glob.glob(os.path.join(path, "**", pattern), recursive=True):
        with open(f) as fh:
            yield from csv.DictReader(fh)


def pmc_parse(path, out):
    """FETCH_SIZE (KiB; doubled, as tools/pmc_traffic.py does for the 16-B-per-
    lane streaming reads on gfx950) of every fused dispatch against n * L * S."""
    algorithmic = N * (1 << 20) * PROFILE_STRIPES
    vals = [float(r["Counter_Value"]) for r in rows_of(path, "*counter_collection.csv")
            if r["Counter_Name"] == "FETCH_SIZE" and "scrub_crc_kernel" in r["Kernel_Name"]]
    if not vals:
        sys.exit(f"no scrub_crc_kernel dispatch with FETCH_SIZE under {path}")
    write(out, {"kernel": f"scrub_crc_kernel<{P}>", "dispatches": len(vals), "FETCH_SIZE_KiB": vals,
                "algorithmic_read_bytes": algorithmic, "ratio": [2 * v * 1024 / algorithmic for v in vals]})


def trace_parse(path, out):
    """Per kernel family of the heal + CRC call: dispatches and mean microseconds."""
    fam = {}
    for r in rows_of(path, "*kernel_trace.csv"):
        for key in ("scrub_crc_kernel", "scrub_crc_redo_kernel", "crc_fold_kernel", "scrub_init_kernel"):
            if key + "<" in r["Kernel_Name"] or key + "(" in r["Kernel_Name"] or r["Kernel_Name"].endswith(key):
                fam.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if "scrub_crc_redo_kernel" not in fam:
        sys.exit(f"no scrub_crc_redo_kernel dispatch under {path}")
    res = {k: {"dispatches": len(v), "mean_us": round(sum(v) / len(v), 2)} for k, v in fam.items()}
    total = sum(x["mean_us"] for x in res.values())
    res["redo_share"] = round(res["scrub_crc_redo_kernel"]["mean_us"] / total, 5)
    write(out, res)


def write(out, res):
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] in ("pmc-run", "trace-run"):
        profile_run(sys.argv[1] == "trace-run")
    elif len(sys.argv) == 4 and sys.argv[1] == "pmc-parse":
        pmc_parse(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "trace-parse":
        trace_parse(sys.argv[2], sys.argv[3])
    else:
        ap = argparse.ArgumentParser()
        ap.add_argument("--stripes", type=int, default=1024)
        ap.add_argument("--cell", type=int, default=1 << 20)
        ap.add_argument("--reps", type=int, default=20)
        ap.add_argument("--warmup", type=int, default=3)
        ap.add_argument("--host-stripes", type=int, default=256)
        ap.add_argument("--host-cell", type=int, default=256 << 10)
        ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub", "bench_scrub_crc.json"))
        a = ap.parse_args()
        if a.reps < 20:
            ap.error("--reps must be at least 20")
        bench(a)
