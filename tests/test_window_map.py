"""The window map the static encode and the runtime-matrix repairs walk
(lambdafs_amd/csrc/hrs_window_map.hpp; HRS_WINDOW_SPLIT), enumerated on the
CPU by tests/cpp/window_map.cpp: every row of 0..600 whole windows under every
half distance from 1 KiB (contiguous, today's offsets) to 1 MiB. The two 1 KiB
pieces of all tasks partition the row exactly once, none crosses the row end,
strided windows lie where the definition puts them and rows shorter than a
group stay contiguous. Pins the map without a GPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_map_partitions_every_row():
    binary = os.path.join(ROOT, "tests", "cpp", "window_map")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", ROOT, "tests/cpp/window_map"])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["window_map_cases"] == 11 * 601
    assert all(res[k] == 0 for k in ("bad_cover", "bad_bounds", "bad_contiguous", "bad_definition", "bad_parse")), res
