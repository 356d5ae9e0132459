"""A/B report over tools/bench_host_legs.py lines: DIR holds parent_*.json and new_*.json of one session.
Per leg: the parent's range (min, median, max over all its timed calls), the new build's median, and whether
that lies under, inside or ABOVE the range.

Run: python tools/bench_host_legs_report.py DIR [summary.json]
"""
import glob
import json
import sys

import numpy as np

d = sys.argv[1]
runs = {"parent": {}, "new": {}}
libs = {"parent": set(), "new": set()}
for f in sorted(glob.glob(d + "/*.json")):
    who = "parent" if "parent" in f.rsplit("/", 1)[1] else "new"
    j = json.loads(open(f).read().strip().splitlines()[-1])
    libs[who].add(j["lib"])
    for leg, ms in j["legs_ms"].items():
        runs[who].setdefault(leg, []).extend(ms)
print(libs)
out = {}
for leg in runs["parent"]:
    pa, nw = np.array(runs["parent"][leg]), np.array(runs["new"][leg])
    row = {"parent_min": round(float(pa.min()), 3), "parent_median": round(float(np.median(pa)), 3),
           "parent_max": round(float(pa.max()), 3), "new_median": round(float(np.median(nw)), 3)}
    row["verdict"] = "under" if row["new_median"] < row["parent_min"] else \
        "inside" if row["new_median"] <= row["parent_max"] else "ABOVE"
    out[leg] = row
    print(f"{leg:28s} parent [{row['parent_min']:9.3f} {row['parent_median']:9.3f} {row['parent_max']:9.3f}]  "
          f"new {row['new_median']:9.3f}  {row['new_median'] / row['parent_median']:.3f}  {row['verdict']}")
if len(sys.argv) > 2:
    json.dump(out, open(sys.argv[2], "w"), indent=1)
