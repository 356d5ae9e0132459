"""bench.py's plain run and --dump-outputs: the dump is whole where an output
fits its share of the 64 MB, else a sample at the same seeded positions in
every run (CPU); a plain run prints the headline line alone, and what it
dumps is the oracle's parity and the lost shard (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_options_default_to_a_plain_run():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_small_outputs_are_dumped_whole(tmp_path):
    import torch
    import bench
    par = torch.arange(2 * 4 * 64, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(2, 4, 64)
    stripes = torch.zeros((2, 14, 64), dtype=torch.uint8)
    stripes[:, :4] = par
    dec = par[:, :1] + 1
    bench.dump_outputs(str(tmp_path / "d"), (("parity", stripes[:, :4]), ("decode", dec)), 0, 1)
    got = np.load(tmp_path / "d" / "parity.npy")
    assert got.dtype == np.float32 and np.array_equal(got, par.numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "d" / "decode.npy"), dec.numpy().astype(np.float32))


def test_large_outputs_are_sampled_at_fixed_positions(tmp_path, monkeypatch):
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 1000)  # 1,000 float32 over both outputs
    g = torch.Generator().manual_seed(5)
    stripes = torch.randint(0, 256, (8, 6, 512), dtype=torch.uint8, generator=g)
    dec = torch.randint(0, 256, (8, 1, 512), dtype=torch.uint8, generator=g)
    outs = (("parity", stripes[:, :2]), ("decode", dec))  # a strided view, as the bench passes
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, 0, 1)
    a, b = np.load(tmp_path / "a" / "parity.npy"), np.load(tmp_path / "b" / "parity.npy")
    da = np.load(tmp_path / "a" / "decode.npy")
    assert a.dtype == np.float32 and a.ndim == 1 and a.size + da.size <= 1000 and a.size == 2 * da.size
    assert np.array_equal(a, b)
    # the sample is the bytes at the seeded, sorted positions of the [S, p, L] parity
    pos = np.sort(np.random.default_rng([0x5EED00D0, 0]).integers(0, 8 * 2 * 512, a.size))
    assert np.array_equal(a, stripes[:, :2].contiguous().numpy().reshape(-1)[pos].astype(np.float32))
    # one changed byte at a sampled position shows in the dump
    s, r, c = np.unravel_index(pos[3], (8, 2, 512))
    stripes[s, r, c] ^= 0x40
    bench.dump_outputs(str(tmp_path / "c"), outs, 0, 1)
    assert not np.array_equal(np.load(tmp_path / "c" / "parity.npy"), a)
    # ranks split the budget and write their own files
    bench.dump_outputs(str(tmp_path / "r"), outs, 1, 2)
    assert np.load(tmp_path / "r" / "parity_rank1.npy").size == a.size // 2


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(cuda, tmp_path):
    import synth
    from oracle import rs_oracle as C
    k, p, L, S = 10, 4, 64 << 10, 6
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--stripes", str(S), "--cell", str(L), "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["metric"].startswith("RS encode+decode GiB/s device-resident")
    assert line["ms_per_step"] > 0
    # value is the user bytes of the timed steps over their time (both rounded to 3 places in the line)
    want = 2 * k * L * S / 2.0 ** 30 / (line["ms_per_step"] * 1e-3)
    assert abs(line["value"] - want) <= want * 0.0006 / line["ms_per_step"] + 0.001
    for key in ("hbm_probes", "cpu_baseline", "host_calls", "e2e_config5", "parity_sha256", "roofline"):
        assert key not in line  # legs of --full
    par, dec = np.load(tmp_path / "parity.npy"), np.load(tmp_path / "decode.npy")
    assert par.dtype == dec.dtype == np.float32 and par.shape == (S, p, L) and dec.shape == (S, 1, L)
    for s in range(S):
        data = list(synth.stripe_numpy(3, s, k, L))
        ref = C.encode_bulk(k, p, data)
        assert all(np.array_equal(par[s, r], ref[r].astype(np.float32)) for r in range(p))
        assert np.array_equal(dec[s, 0], data[0].astype(np.float32))
