"""CPU tests of hrs_heal_ragged_host (one stripe on the CPU, host-only handle)
against the oracle's expectations of tests/ragged_scrub_inputs.py, demotion
included, for every code of the GPU tests; its all-full equality with
hrs_heal_host; and that every GPU batch, by the oracle alone, holds at least
one column of every class its parity size allows, so no test passes by
covering nothing."""
import os
import subprocess

import numpy as np
import pytest

import ragged_scrub_inputs as R
from lambdafs_amd import HipReedSolomonCode, device

NONE = -2  # HRS_DEVICE_NONE


@pytest.mark.parametrize("k,p,L", R.all_cases())
def test_batches_hold_every_class(k, p, L):
    stored, valid, healed, rep, rep2, classes, kinds = R.batch(k, p, L)
    print(f"RS({k},{p}) L={L} S={len(kinds)}: { {c: v for c, v in classes.items() if c != 'bad'} }")
    assert (6 <= len(kinds) <= 40) or (k, p) == R.WIDE
    for name in R.required_classes(p, L):
        assert classes[name] >= 1, (name, classes)
    n = k + p
    for s in range(len(kinds)):  # junk behind every length, none of it zero
        for l in range(n):
            assert stored[s, l, valid[s, l]:].all()
    # the heal changes exactly the patched bytes, all of them below their cell's length
    assert rep[:, 3].tolist() == [int(np.count_nonzero(stored[s] != healed[s])) for s in range(len(kinds))]
    for s, l, c in np.argwhere(stored != healed):
        assert c < valid[s, l]
    # a second heal finds the unresolved and demoted columns only
    assert rep2[:, 0].tolist() == rep2[:, 1].tolist() == rep[:, 1].tolist()
    assert not rep2[:, 3].any() and not rep2[:, 4:].any()
    if (k, p) != R.WIDE:
        assert {"low", "top", "run", "gap", "zero", "short"} <= set(kinds)
        cl = set(R.length_classes(L))
        assert cl <= set(int(v) for v in valid[:, 0]) and cl <= set(int(v) for v in valid[:, n - 1])
        assert cl <= set(int(v) for v in valid[:, p - 1])
        if n >= 9:
            assert cl <= set(int(v) for v in valid[:, n - 9]) | set(int(v) for v in valid[:, n - 8])
        zero = kinds.index("zero")
        assert not valid[zero].any() and rep[zero].tolist() == [0, 0, R.NONE, 0] + [0] * n


@pytest.mark.parametrize("k,p,L", R.all_cases())
def test_heal_ragged_host_matches_oracle(k, p, L):
    stored, valid, healed, rep, rep2, _, kinds = R.batch(k, p, L)
    code = HipReedSolomonCode(k, p, device=NONE)
    for s in range(len(kinds)):
        rows = [stored[s, l].copy() for l in range(k + p)]
        got = device.heal_host_ragged(code, rows, valid[s])
        assert got.tolist() == rep[s].tolist(), (s, kinds[s], valid[s].tolist())
        assert R.mismatch(np.stack(rows), healed[s], f"stripe {s} ({kinds[s]})") is None
        got = device.heal_host_ragged(code, rows, valid[s])
        assert got.tolist() == rep2[s].tolist() and (np.stack(rows) == healed[s]).all()


@pytest.mark.parametrize("k,p", R.CODES)
def test_all_full_equals_heal_host(k, p):
    stored, valid, *_ = R.batch(k, p, R.L_TAIL)
    code = HipReedSolomonCode(k, p, device=NONE)
    full = np.full(k + p, R.L_TAIL, np.uint32)
    for s in range(stored.shape[0]):
        a = [stored[s, l].copy() for l in range(k + p)]
        b = [stored[s, l].copy() for l in range(k + p)]
        assert device.heal_host_ragged(code, a, full).tolist() == device.heal_host(code, b).tolist()
        assert (np.stack(a) == np.stack(b)).all()


def test_ragged_heal_logic_program():
    """tests/cpp/ragged_heal_logic.cpp: hrs_heal_ragged_host against a model over
    the scalar hrs_compute_error_locations, every cell allocated with exactly
    its valid bytes (also part of the `make asan` run)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "ragged_heal_logic")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", root, "tests/cpp/ragged_heal_logic"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ragged_heal_logic: ok" in out.stdout
