"""HBM read bytes of the clean-path scrub kernel from a rocprofv3 counter pass
(the figure in DESIGN.md §10, profiles/scrub/pmc_fetch.json).

  run    the profiled program: three clean scrubs of RS(10,4), 1 MiB cells,
         256 stripes (3.5 GiB, past the Infinity Cache)
  parse  FETCH_SIZE of every scrub_kernel dispatch in <dir>'s counter CSV
         against the algorithmic bytes n * L * S (KiB units; doubled, as
         tools/pmc_traffic.py does for 16-B-per-lane streaming reads on gfx950)

Counters in a run of their own, no tracing beside them (profiles/run_rocprof.sh):

  rocprofv3 --pmc FETCH_SIZE --output-format csv -d <dir> -o run -- python3 tools/scrub_pmc.py run
  python3 tools/scrub_pmc.py parse <dir> profiles/scrub/pmc_fetch.json
"""
import csv
import glob
import json
import os
import sys

K, P, L, S = 10, 4, 1 << 20, 256
ALGORITHMIC = (K + P) * L * S


def run():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from lambdafs_amd import HipReedSolomonCode, device
    code = HipReedSolomonCode(K, P)
    torch.manual_seed(3)
    st = torch.randint(0, 256, (S, K + P, L), dtype=torch.uint8, device="cuda")
    device.encode_stripes(code, st)
    for _ in range(3):
        reports = device.scrub_stripes(code, st)
    torch.cuda.synchronize()
    assert int((reports[:, 0] != 0).sum()) == 0, "encoded stripes must scrub clean"
    print("algorithmic_read_bytes", ALGORITHMIC)


def parse(path, out):
    vals = []
    for f in glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if row["Counter_Name"] == "FETCH_SIZE" and "scrub_kernel" in row["Kernel_Name"]:
                    vals.append(float(row["Counter_Value"]))
    if not vals:
        sys.exit(f"no scrub_kernel dispatch with FETCH_SIZE under {path}")
    res = {"kernel": f"scrub_kernel<{P}>", "dispatches": len(vals), "FETCH_SIZE_KiB": vals,
           "read_bytes_x2": [2 * v * 1024 for v in vals], "algorithmic_read_bytes": ALGORITHMIC,
           "ratio": [2 * v * 1024 / ALGORITHMIC for v in vals]}
    line = json.dumps(res)
    print(line)
    with open(out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 4 and sys.argv[1] == "parse":
        parse(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
