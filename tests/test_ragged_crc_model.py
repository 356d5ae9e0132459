"""The CRC side of the ragged encode + CRC kernels, restated on the CPU with
the kernels' own tables (tests/cpp/ragged_crc_model.cpp) and checked against
zlib over the zero-filled cell: masked lane words, dead sub-windows that
advance the chain, raw 0 for dead windows, the fold; 2 KiB sub-windows at
subs 1, 2 and 16 and the 32 KiB windows with their right-aligned tail, at every
valid class of ragged_inputs.valid_classes. Pins the algebra without a GPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_crc_model_against_zlib():
    binary = os.path.join(ROOT, "tests", "cpp", "ragged_crc_model")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", ROOT, "tests/cpp/ragged_crc_model"])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["ragged_crc_model_cases"] >= 200
    assert res["mismatches"] == 0 and res["dead_windows_nonzero"] == 0 and res["dead_windows_read"] == 0
