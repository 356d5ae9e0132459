"""Heal-with-known-erasures timing (hrs_heal_erased_dev) beside the calls it
replaces, one JSON line. One device, RS(10,4), 1 MiB cells, 1,024 stripes, one
random lost cell per stripe unless told otherwise. Legs, alternating in this
process:

  (a) decode_batch      hrs_decode_batch_dev: moves k + e rows;
  (b) scrub             hrs_scrub_dev over the same tensor (n rows; with a lost
                        cell every column is dirty, so it runs over the
                        REPAIRED stripes, the best case of the second pass);
  (c) decode_then_scrub (a) then (b): today's only way to repair and learn
                        that the survivors disagree: the yardstick;
  (d) heal_erased       hrs_heal_erased_dev, clean survivors: n rows;
  (e) heal_erased_byte  (d) with one single-byte survivor error per stripe,
                        planted again before every repetition, untimed;
  (f) heal              hrs_heal_dev, clean stripes;
  (g) heal_erased_none  nothing erased, through the new call.

HIP events around each repetition, warm-up, median of --reps (>= 20) with
[min, max]. Run it on an idle card.

  python tools/bench_heal_erased.py [--stripes 1024] [--reps 20] [--out FILE]
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
ap.add_argument("--stripes", type=int, default=1024)
ap.add_argument("--cell", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--heal-json", default=os.path.join(ROOT, "profiles", "heal", "bench_heal.json"),
                help="recorded scrub / heal ranges to compare legs (b) and (f) with")
ap.add_argument("--out", default=None, help="also write the JSON line here")
args = ap.parse_args()
if args.reps < 20:
    ap.error("--reps must be at least 20")


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def interleaved(fns, before=None):
    before = before or {}
    samples = {name: [] for name in fns}
    for r in range(args.warmup + args.reps):
        for name, fn in fns.items():
            if name in before:
                before[name]()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                samples[name].append(a.elapsed_time(b))
    return {name: stats(ms) for name, ms in samples.items()}


def u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


torch.manual_seed(31)
k, p, L, S = 10, 4, args.cell, args.stripes
n = k + p
code = HipReedSolomonCode(k, p)
st = torch.randint(0, 256, (S, n, L), dtype=torch.uint8, device="cuda")
device.encode_stripes(code, st)
lost = np.random.default_rng(31).integers(0, n, S).astype(np.int32)
erased = lost.reshape(S, 1)
none = np.full((S, 1), -1, dtype=np.int32)
out = torch.empty((S, 1, L), dtype=torch.uint8, device="cuda")
idx_s = torch.arange(S, device="cuda")
idx_lost = torch.from_numpy(lost.astype(np.int64)).to("cuda")
idx_l = (idx_lost + 1 + idx_s % (n - 1)) % n  # a survivor of each stripe
idx_c = (idx_s * 7919) % L


def flip_bytes():
    st[idx_s, idx_l, idx_c] ^= 0x5A


# what every leg computes, checked once
device.decode_batch(code, st, erased, out)
assert torch.equal(out[:, 0], st[idx_s, idx_lost]), "decode_batch must rebuild the lost cells"
clean = st.clone()
st[idx_s, idx_lost] = 0xA5
r = u32(device.heal_erased_stripes(code, st, erased))
kernel = code.lastKernel()
assert torch.equal(st, clean) and not r[:, [0, 1, 3]].any(), "clean survivors: cells rebuilt, empty reports"
st[idx_s, idx_lost] = 0xA5
flip_bytes()
r = u32(device.heal_erased_stripes(code, st, erased))
assert torch.equal(st, clean) and (r[:, [0, 1, 3]] == [1, 0, 1]).all(), "one survivor byte fixed per stripe"
del clean


def decode_then_scrub():
    device.decode_batch(code, st, erased, out)
    device.scrub_stripes(code, st)


t = interleaved({
    "decode_batch": lambda: device.decode_batch(code, st, erased, out),
    "scrub": lambda: device.scrub_stripes(code, st),
    "decode_then_scrub": decode_then_scrub,
    "heal_erased": lambda: device.heal_erased_stripes(code, st, erased),
    "heal_erased_byte": lambda: device.heal_erased_stripes(code, st, erased),
    "heal": lambda: device.heal_stripes(code, st),
    "heal_erased_none": lambda: device.heal_erased_stripes(code, st, none),
}, before={"heal_erased_byte": flip_bytes})
assert not u32(device.scrub_stripes(code, st))[:, 0].any(), "the stripes must end clean"

c, d = t["decode_then_scrub"], t["heal_erased"]
res = {"bench": "heal_erased", "k": k, "p": p, "cell": L, "stripes": S, "lost_cells_per_stripe": 1, "reps": args.reps,
       "kernel": kernel, "legs": t,
       "bytes": {"decode_batch": (k + 1) * L * S, "scrub": n * L * S, "decode_then_scrub": (k + 1 + n) * L * S,
                 "heal_erased": n * L * S},
       "heal_erased_below_decode_then_scrub_by_more_than_its_spread":
           bool(c["median_ms"] - d["median_ms"] > c["max_ms"] - c["min_ms"]),
       "heal_erased_over_decode_batch": round(d["median_ms"] / t["decode_batch"]["median_ms"], 3),
       "heal_erased_over_scrub": round(d["median_ms"] / t["scrub"]["median_ms"], 3),
       "heal_erased_over_decode_then_scrub": round(d["median_ms"] / c["median_ms"], 3)}
if os.path.exists(args.heal_json) and (L, S) == (1 << 20, 1024):
    rec = json.load(open(args.heal_json))["clean"]
    res["recorded"] = {"file": os.path.relpath(args.heal_json, ROOT), "scrub": rec["scrub"], "heal": rec["heal"],
                       "scrub_median_inside_recorded_range":
                           bool(rec["scrub"]["min_ms"] <= t["scrub"]["median_ms"] <= rec["scrub"]["max_ms"]),
                       "heal_median_inside_recorded_range":
                           bool(rec["heal"]["min_ms"] <= t["heal"]["median_ms"] <= rec["heal"]["max_ms"])}

line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
