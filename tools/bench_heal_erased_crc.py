"""Heal with known erasures + CRC-32 timing (hrs_heal_erased_crc_dev,
hrs_heal_erased_batch_host, hrs_heal_erased_batch_host_crc) against the two
passes they replace, one JSON line (DESIGN.md §10.4,
profiles/heal_erased/bench_heal_erased_crc.json).

Every comparison runs in one process with its legs alternating repetition by
repetition; per leg the median of --reps (>= 20) after warm-up with [min, max].
Device legs are timed with HIP events, the synchronous host calls with the
host clock.

  device, RS(10,4), 1 MiB cells, 1,024 stripes, one random lost cell per stripe
  (the workload of tools/bench_heal_erased.py):
    (a) hrs_heal_erased_dev
    (b) (a), then hrs_crc32_dev over the 14 rows: the two-pass route, the baseline
    (c) hrs_heal_erased_crc_dev in kernel mode 3 (the fused kernel), once per
        block width that is built for the parity size (P = 4: 512 threads)
    (d) (c) with one single-byte survivor error per stripe (planted again
        before every repetition, untimed)
    (m0) hrs_heal_erased_crc_dev in kernel mode 0: the route the library picks
  host, pinned, RS(12,4), 256 KiB cells, 256 stripes, one lost cell per stripe:
    hrs_heal_erased_batch_host, hrs_heal_erased_batch_host_crc in kernel mode 3,
    the plain call plus a second zero-copy CRC read of the stripes
    (hrs_crc32_dev over the pinned stripes' device addresses where the runtime
    maps them, else hrs_scrub_batch_host; "second_read" says which), and
    hrs_heal_erased_batch_host_crc in kernel mode 0

  python tools/bench_heal_erased_crc.py [--stripes 1024] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

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


def clean_stripes(torch, device, code, k, p, cell, stripes, seed):
    torch.manual_seed(seed)
    st = torch.randint(0, 256, (stripes, k + p, cell), dtype=torch.uint8, device="cuda")
    device.encode_stripes(code, st)
    return st


def plant(torch, st, lost):
    """One single-byte error per stripe in the survivor after its lost cell, each in another window."""
    s = torch.arange(st.shape[0], device=st.device)
    st[s, (lost + 1) % st.shape[1], (s * 2053 + 17) % st.shape[2]] ^= 0x5A


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
    code = HipReedSolomonCode(K, P)    # kernel mode 0
    fcode = HipReedSolomonCode(K, P)   # kernel mode 3: the fused kernel
    fcode.setKernelMode(3)
    st = clean_stripes(torch, device, code, K, P, L, S, 23)
    rows = [st[:, l, :] for l in range(N)]
    want_crc = device.crc32_rows(code, rows)
    lost_host = np.random.default_rng(7).integers(0, N, S)
    lost = torch.from_numpy(lost_host).to("cuda")
    erased = lost_host.reshape(S, 1).astype(np.int32)
    st[torch.arange(S, device="cuda"), lost] = 0xA5
    rep, crc = device.heal_erased_stripes_crc(fcode, st, erased)
    fused_kernel = fcode.lastKernel()
    assert int((rep[:, 0] != 0).sum()) == 0, "encoded survivors must be consistent"
    assert torch.equal(crc, want_crc), "fused CRCs differ from hrs_crc32_dev over the encoded stripes"
    device.heal_erased_stripes_crc(code, st, erased)
    mode0_kernel = code.lastKernel()

    def fused(threads):
        def run():
            os.environ["HRS_HEAL_ERASED_CRC_THREADS"] = threads
            device.heal_erased_stripes_crc(fcode, st, erased)
        return run

    widths = ["512"] if P == 4 else ["1024", "512"]  # the instantiations hrs_heal_erased_crc.hip builds
    legs = {
        "a_heal_erased": lambda: device.heal_erased_stripes(code, st, erased),
        "b_heal_erased_then_crc32": lambda: (device.heal_erased_stripes(code, st, erased),
                                             device.crc32_rows(code, rows)),
    }
    for w in widths:
        legs[f"c{w}_heal_erased_crc"] = fused(w)
    legs[f"d{widths[0]}_one_error_per_stripe"] = fused(widths[0])
    legs["m0_heal_erased_crc_mode_0"] = lambda: device.heal_erased_stripes_crc(code, st, erased)
    dev = alternate(legs, before={f"d{widths[0]}_one_error_per_stripe": lambda: plant(torch, st, lost)})
    plant(torch, st, lost)
    rep, crc = device.heal_erased_stripes_crc(fcode, st, erased)
    r = rep.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert (r[:, 0] == 1).all() and (r[:, 3] == 1).all(), "one error per stripe, each healed"
    assert torch.equal(crc, want_crc), "CRCs after the heal differ from the encoded stripes'"
    del st, rows
    torch.cuda.empty_cache()

    # host batch from pinned memory
    hk, hp, hL, hS = 12, 4, args.host_cell, args.host_stripes
    hn = hk + hp
    hcode = HipReedSolomonCode(hk, hp)
    hfcode = HipReedSolomonCode(hk, hp)
    hfcode.setKernelMode(3)
    pinned = clean_stripes(torch, device, hcode, hk, hp, hL, hS, 29).cpu().pin_memory()
    torch.cuda.empty_cache()
    herased = np.random.default_rng(11).integers(0, hn, (hS, 1)).astype(np.int32)
    got = device.heal_erased_batch_host(hcode, pinned, herased)
    mapped = hcode.lastHostPath() == "pinned"
    assert not got[:, 0].any(), "encoded host survivors must be consistent"
    got, hcrc = device.heal_erased_batch_host_crc(hfcode, pinned, herased)
    host_kernel = hfcode.lastKernel()
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
        device.heal_erased_batch_host(hcode, pinned, herased)
        second_read()

    hlegs = {"heal_erased_batch_host": lambda: device.heal_erased_batch_host(hcode, pinned, herased),
             "heal_erased_batch_host_crc": lambda: device.heal_erased_batch_host_crc(hfcode, pinned, herased),
             "heal_erased_batch_host_then_second_read": both,
             "heal_erased_batch_host_crc_mode_0": lambda: device.heal_erased_batch_host_crc(hcode, pinned, herased)}
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
    plain, fusedh, twice = (host[x] for x in list(hlegs)[:3])
    device.heal_erased_batch_host_crc(hcode, pinned, herased)

    nbytes = N * L * S
    a, b = dev["a_heal_erased"], dev["b_heal_erased_then_crc32"]
    c = min((dev[f"c{w}_heal_erased_crc"] for w in widths), key=lambda x: x["median_ms"])
    line = json.dumps({
        "bench": "heal_erased_crc", "k": K, "p": P, "cell": L, "stripes": S, "bytes": nbytes, "reps": args.reps,
        "date": time.strftime("%Y-%m-%d"), "kernel": fused_kernel, "mode_0_kernel": mode0_kernel,
        "device": dev,
        "c_faster_than_b_ranges_apart": apart(c, b),
        "c_over_b": round(c["median_ms"] / b["median_ms"], 4),
        "c_over_a": round(c["median_ms"] / a["median_ms"], 4),
        "host": {"k": hk, "p": hp, "cell": hL, "stripes": hS, "bytes": hbytes, "path": hcode.lastHostPath(),
                 "kernel": host_kernel, "mode_0_kernel": hcode.lastKernel(), "second_read": "hrs_crc32_dev" if mapped else "hrs_scrub_batch_host",
                 "legs": host,
                 "crc_faster_than_two_reads_ranges_apart": apart(fusedh, twice),
                 "crc_over_plain": round(fusedh["median_ms"] / plain["median_ms"], 4),
                 "crc_over_two_reads": round(fusedh["median_ms"] / twice["median_ms"], 4)},
    })
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
    ap.add_argument("--host-stripes", type=int, default=256)
    ap.add_argument("--host-cell", type=int, default=256 << 10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heal_erased", "bench_heal_erased_crc.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    bench(a)
