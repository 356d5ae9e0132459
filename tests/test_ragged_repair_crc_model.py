"""The fold of the ragged repair + CRC calls, restated on the CPU with the
kernels' own tables and the field algebra of crc32.hpp that the fold kernel
compiles (tests/cpp/ragged_repair_crc_model.cpp), checked against zlib over
EXACTLY the cell's first v bytes, with and without a seeded crc_in: raw words
per 2 KiB window of a masked cell with dead windows absent (poisoned: a fold
that reads one fails), then unpad; raw words per 32 KiB window with the
right-aligned tail window, then unpad by len - v. Lengths: every class of
ragged_repair_inputs.length_classes for L = 4096 and 4176, and for L = 66 x
2048 (+ 80) also the 63-66-window lengths, where a lane holds two windows.
Pins the algebra without a GPU."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_repair_crc_model_against_zlib():
    binary = os.path.join(ROOT, "tests", "cpp", "ragged_repair_crc_model")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", ROOT, "tests/cpp/ragged_repair_crc_model"])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    # 12 classes at each short length, 21 and 24 at the long ones; both forms at whole windows, the
    # window form alone otherwise; two seeds
    assert res["ragged_repair_crc_model_cases"] == 2 * (12 * 2 + 12 + 21 * 2 + 24)
    assert res["mismatches"] == 0 and res["unwritten_words_read"] == 0 and res["algebra_failures"] == 0
