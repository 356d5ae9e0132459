"""Stripe-heal timing (hrs_heal_dev / hrs_heal_batch_host) beside the scrub,
one JSON line. RS(10,4), 1 MiB cells, 1,024 stripes unless told otherwise.

  (1) clean stripes: heal against scrub, alternating in this process. The
      clean path is the same loads and math, so heal's median should lie
      inside the min-max range of the scrub's own samples;
  (2) clean scrub of this build against another build of libhrs.so
      (--parent-lib, e.g. the parent commit's), alternating, same criterion;
  (3) one whole corrupted cell per stripe: heal, the scrub of the same input,
      and the two-pass route scrub -> scrub_to_erased -> decode_batch;
  (4) one single-byte error per stripe: heal against clean heal;
  (5) hrs_heal_batch_host against hrs_scrub_batch_host on one pinned buffer:
      RS(12,4), 256 KiB cells, 256 stripes, clean.

Warm-up, then HIP events around each repetition, median of --reps (>= 20);
the legs that end in a host synchronise ((3)'s two-pass route, (5)) use the
host clock. Heal repairs what it finds, so the corruption of (3) and (4) is
put back before every repetition, outside the timed region. Run it on an idle
card.

  python tools/bench_heal.py [--stripes 1024] [--reps 20] [--parent-lib SO] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lambdafs_amd import HipReedSolomonCode, _lib, device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--stripes", type=int, default=1024)
ap.add_argument("--cell", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--host-stripes", type=int, default=256)
ap.add_argument("--host-cell", type=int, default=256 << 10)
ap.add_argument("--parent-lib", default=None, help="another libhrs.so for leg (2)")
ap.add_argument("--out", default=None, help="also write the JSON line here")
args = ap.parse_args()
if args.reps < 20:
    ap.error("--reps must be at least 20")


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def interleaved(fns, before=None, host_clock=False):
    """Times the callables of `fns` (name -> fn) in turn, --reps rounds after
    --warmup rounds; before[name]() runs untimed ahead of each call."""
    before = before or {}
    samples = {name: [] for name in fns}
    for r in range(args.warmup + args.reps):
        for name, fn in fns.items():
            if name in before:
                before[name]()
            torch.cuda.synchronize()
            if host_clock:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms = a.elapsed_time(b)
            if r >= args.warmup:
                samples[name].append(ms)
    return {name: stats(ms) for name, ms in samples.items()}


def inside(x, ref):
    return bool(ref["min_ms"] <= x["median_ms"] <= ref["max_ms"])


def u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


torch.manual_seed(29)
k, p, L, S = 10, 4, args.cell, args.stripes
n = k + p
code = HipReedSolomonCode(k, p)
st = torch.randint(0, 256, (S, n, L), dtype=torch.uint8, device="cuda")
device.encode_stripes(code, st)
nbytes = n * L * S
res = {"bench": "heal", "k": k, "p": p, "cell": L, "stripes": S, "bytes_read": nbytes, "reps": args.reps}

# (1) clean: heal against scrub
assert not u32(device.heal_stripes(code, st))[:, [0, 3]].any(), "encoded stripes must heal clean"
res["heal_kernel"] = code.lastKernel()
t = interleaved({"scrub": lambda: device.scrub_stripes(code, st), "heal": lambda: device.heal_stripes(code, st)})
res["clean"] = {"scrub": t["scrub"], "heal": t["heal"], "heal_median_inside_scrub_range": inside(t["heal"], t["scrub"]),
                "heal_GBps": round(nbytes / (t["heal"]["median_ms"] * 1e-3) / 1e9, 1),
                "scrub_GBps": round(nbytes / (t["scrub"]["median_ms"] * 1e-3) / 1e9, 1)}

# (2) clean scrub: this build against another one, through the same raw calls
if args.parent_lib:
    reports = torch.empty((S, 4 + n), dtype=torch.int32, device="cuda")
    rows = _lib.ptr_array([st.data_ptr() + l * st.stride(1) for l in range(n)])
    stream = torch.cuda.current_stream().cuda_stream

    def raw_scrub(lib, handle):
        argt = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.hrs_scrub_dev.argtypes, lib.hrs_scrub_dev.restype = argt, ctypes.c_int

        def call():
            st_ = lib.hrs_scrub_dev(handle, rows, st.stride(0), L, S, reports.data_ptr(), 4 + n, stream)
            assert st_ == 0, st_
        return call

    other = ctypes.CDLL(os.path.abspath(args.parent_lib))
    other.hrs_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    other.hrs_create.restype = ctypes.c_int
    oh = ctypes.c_void_p()
    assert other.hrs_create(k, p, None, ctypes.byref(oh)) == 0
    t = interleaved({"this": raw_scrub(_lib.lib(), code._handle()), "parent": raw_scrub(other, oh)})
    assert not u32(reports)[:, 0].any()
    res["clean_scrub_vs_parent"] = {"this": t["this"], "parent": t["parent"],
                                    "this_median_inside_parent_range": inside(t["this"], t["parent"])}

# (3) one whole corrupted cell per stripe
idx_s = torch.arange(S, device="cuda")
idx_l = idx_s % n


def flip_cells():
    st[idx_s, idx_l] = st[idx_s, idx_l].bitwise_not()


flip_cells()
r = u32(device.heal_stripes(code, st))
assert (r[:, 0] == L).all() and (r[:, 1] == 0).all() and (r[:, 3] == L).all(), "one error in every column"
assert not u32(device.scrub_stripes(code, st))[:, 0].any(), "healed stripes must scrub clean"
flip_cells()
out = torch.empty((S, p, L), dtype=torch.uint8, device="cuda")


def two_pass():
    reports = device.scrub_stripes(code, st)
    device.decode_batch(code, st, device.scrub_to_erased(reports, p), out)


t = interleaved({"scrub": lambda: device.scrub_stripes(code, st), "two_pass": two_pass}, host_clock=True)
res["cell_per_stripe"] = {"scrub": t["scrub"], "scrub_then_decode_batch": t["two_pass"]}
flip_cells()  # clean again: the heal leg corrupts before each call
res["cell_per_stripe"]["heal"] = interleaved({"heal": lambda: device.heal_stripes(code, st)},
                                             before={"heal": flip_cells}, host_clock=True)["heal"]
assert not u32(device.scrub_stripes(code, st))[:, 0].any()
del out

# (4) one single-byte error per stripe: heal, then the heal of the now clean stripes
idx_c = (idx_s * 7919) % L


def flip_bytes():
    st[idx_s, idx_l, idx_c] ^= 0x5A


t = interleaved({"one_byte": lambda: device.heal_stripes(code, st), "clean": lambda: device.heal_stripes(code, st)},
                before={"one_byte": flip_bytes})
flip_bytes()
r = u32(device.heal_stripes(code, st))
assert (r[:, [0, 1, 3]] == [1, 0, 1]).all()
res["byte_per_stripe"] = {"heal": t["one_byte"], "clean_heal": t["clean"]}
del st
torch.cuda.empty_cache()

# (5) host batch from pinned memory, heal against scrub
hk, hp, hL, hS = 12, 4, args.host_cell, args.host_stripes
hn = hk + hp
hcode = HipReedSolomonCode(hk, hp)
dev = torch.randint(0, 256, (hS, hn, hL), dtype=torch.uint8, device="cuda")
device.encode_stripes(hcode, dev)
pinned = dev.cpu().pin_memory()
del dev
hbytes = hn * hL * hS
assert not device.heal_batch_host(hcode, pinned)[:, [0, 3]].any(), "encoded host stripes must heal clean"
path = hcode.lastHostPath()
t = interleaved({"scrub": lambda: device.scrub_batch_host(hcode, pinned),
                 "heal": lambda: device.heal_batch_host(hcode, pinned)}, host_clock=True)
res["host"] = {"k": hk, "p": hp, "cell": hL, "stripes": hS, "bytes_moved": hbytes, "path": path,
               "scrub": t["scrub"], "heal": t["heal"],
               "scrub_GiBps": round(hbytes / (t["scrub"]["median_ms"] * 1e-3) / 2 ** 30, 2),
               "heal_GiBps": round(hbytes / (t["heal"]["median_ms"] * 1e-3) / 2 ** 30, 2),
               "heal_median_inside_scrub_range": inside(t["heal"], t["scrub"])}

line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
