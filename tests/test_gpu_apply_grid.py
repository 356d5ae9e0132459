"""The runtime-matrix apply (run_apply, csrc/hrs_dispatch.cpp) over its whole
kernel routing table: every bitsliced_kernel, bitsliced_pipe_kernel,
bitsliced_stream_kernel and xor_kernel instantiation hrs_runtime.hip and
hrs_kernels.hip can launch, and bytewise_kernel, each bit-exact against GF(2^8)
products from the oracle's multiply and each named: every case requires
lastKernel() to be the kernel apply_grid.routes says the dispatch picks, so a
shape that silently moves to another kernel fails here.

1..8 outputs x 1..40 live inputs in kernel mode 0 (resident, pipelined and
streaming kernels; 33..40 inputs run the streaming kernel's accumulating second
chunk over 1..8 inputs) and in mode 1 (every resident and pipelined kernel as
the accumulating later chunk, and <3..5, 16>, which mode 0 never reaches),
under HRS_TASK_ORDER=32 so that one block's four waves run all 7, 14 or 21
windows (2/1, 4/3, 6/5 per wave: the pipelined kernel leaves its loop at either
exit, with either register set); sparse matrices and dead columns passed as
None (the first input among them); the XOR route and its chunks; output
chunks; the byte-granular kernel's own chunks; the production window order;
and, in one child process started with HRS_PIPE=0, the 15 plain kernels that
stand in for the pipelined ones. test_apply_grid_inputs.py proves on the CPU
that these cases' kernels are the whole table."""
import json
import os
import subprocess
import sys

import pytest

import apply_grid as G
from lambdafs_amd import HipReedSolomonCode

pytestmark = pytest.mark.gpu

NOUTS = list(G.NOUTS)


def _sweep(cases):
    """Runs the cases; returns the kernels seen."""
    code = HipReedSolomonCode(10, 4)
    seen = set()
    for case in cases:
        bad, kernel = G.run_case(code, *case)
        assert kernel == G.last_kernel(case), (tuple(case), kernel, G.case_routes(case))
        assert bad is None, (tuple(case), kernel, bad)
        seen.add(kernel)
    return seen


@pytest.fixture
def order32(cuda, monkeypatch):
    monkeypatch.setenv("HRS_TASK_ORDER", "32")
    return cuda


@pytest.mark.parametrize("nout", NOUTS)
def test_mode0_grid(order32, nout):
    seen = _sweep(G.mode0_cases(nout))
    want = {name for n in G.NLIVES for name, _, _ in G.routes(nout, n, 0, G.pipe_on())}
    if nout == 1:
        want.add("xor_kernel<4>")  # bits at one input is the matrix [1]
    assert seen == want


@pytest.mark.parametrize("nout", NOUTS)
def test_mode1_grid(order32, nout):
    seen = _sweep(G.mode1_cases(nout))
    assert seen == {name for n in G.NLIVES for name, _, _ in G.routes(nout, n, 1, G.pipe_on())}


@pytest.mark.parametrize("nout", NOUTS)
def test_sparse_and_dead_columns(order32, nout):
    """A zero coefficient skips an output, an all-zero output row is written
    as zeros (not left as poison), and an all-zero column's input is never
    read: it is passed as None, at the first, a middle and the last place."""
    _sweep(G.sparse_dead_cases(nout))


def test_xor_route(order32):
    seen = _sweep(G.xor_cases())
    assert seen >= {"xor_kernel<4>", "xor_kernel<8>", "xor_kernel<12>", "xor_kernel<16>"}


def test_output_chunks(order32):
    assert G.case_routes(G.Case(9, 12, "random", 0), True) == [
        ("bitsliced_stream_kernel<8, 4>", 12, False), ("bitsliced_pipe_kernel<1, 12>", 12, False)]
    _sweep(G.output_chunk_cases())


@pytest.mark.parametrize("nout", NOUTS)
def test_byte_granular_chunks(cuda, nout):
    assert _sweep(G.byte_granular_cases(nout)) == {G.BYTEWISE}


def test_default_order_one_window_per_wave(cuda, monkeypatch):
    monkeypatch.delenv("HRS_TASK_ORDER", raising=False)
    _sweep(G.default_order_cases())


def test_pipe_off_in_a_child_process(cuda):
    """use_pipe() is read once per process: the plain twins of the 15
    pipelined kernels run in one fresh child started with HRS_PIPE=0."""
    # 75 cases. In this process a grid case takes about 4 ms on an MI355X box (test_mode0_grid[8]:
    # 87 cases in 0.31 s, test_mode1_grid[8]: 40 in 0.17 s), so the cases are about 0.3 s; the
    # whole child (python, torch, the library, the 256 x 256 product table, the cases) took
    # 2.1 s. 60 s is that nearly thirty times over, for a busy machine; a child still
    # running then hangs.
    child = subprocess.run(
        [sys.executable, os.path.join(G.ROOT, "tests", "apply_grid.py"), "pipe_twins"], cwd=G.ROOT,
        env={**os.environ, "HRS_PIPE": "0", "HRS_TASK_ORDER": "32"}, timeout=60, capture_output=True, text=True)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-4000:]
    lines = [json.loads(line) for line in child.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == len(G.pipe_twin_cases())
    for line, case in zip(lines, G.pipe_twin_cases()):
        assert (line["nout"], line["nlive"], line["mode"]) == (case.nout, case.nlive, case.mode)
        assert line["mismatch"] is None, line
        assert line["kernel"] == G.last_kernel(case, pipe=False), line
    assert {line["kernel"] for line in lines} == {G.plain_name(o, b) for o, b in G.pipe_classes()}
