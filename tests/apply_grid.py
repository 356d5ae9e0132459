"""Cases, routing model and reference of the runtime-matrix apply tests
(test_apply_grid_inputs.py on the CPU, test_gpu_apply_grid.py on the device).

hrs_apply_dev, the device decodes and the encodes without a compile-time
kernel all end in run_apply (csrc/hrs_dispatch.cpp), which plans one or more
launches per call. `routes` restates that planning from the source rules
(runtime_in_chunk, the stream predicate, launch_bits' NINB ladder, kPipeFits,
BitLoop::kRolled, kMaxOut, kMaxIn), without calling the library, so a test can
say which instantiation a shape must reach and then require lastKernel() to
name it. `walk_lengths` restates wave_tasks (hrs_device.hpp) the same way.

A case is (nout, nlive, kind, mode, L, shift): a matrix kind over nlive live
inputs, S = 1 + nlive % 3 stripes of L-byte rows; shift = 1 moves every row
view off its 16-byte alignment. Inputs come from one seeded pool per L; the
outputs are prefilled with POISON. The expectation is GF(2^8) products from
the oracle's multiply, nothing else.

Run as a program it executes named case lists on the device and prints one
JSON line per case (shape, kind, kernel, first mismatch):
    python tests/apply_grid.py pipe_twins
    HRS_TASK_ORDER=32 python tests/apply_grid.py mode0 mode1
"""
import collections
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import rs_oracle as C  # noqa: E402

WINDOW = 2048  # kWindowBytes
WPB = 4  # kWavesPerBlock
POISON = 0xA5
L_GRID = 7 * WINDOW + 48  # seven windows and a 16-byte-aligned tail for the byte-granular kernel
MAX_OUT, MAX_IN = 8, 32  # kMaxOut, kMaxIn
MAX_IN_RUNTIME, MAX_IN_RUNTIME_WIDE = 16, 8  # kMaxInRuntime, kMaxInRuntimeWide
NOUTS = range(1, 9)
NLIVES = range(1, 41)
KINDS = ("random", "bits", "bits7", "sparse", "dead", "ones")
BYTEWISE = "bytewise_kernel"

Case = collections.namedtuple("Case", "nout nlive kind mode L shift", defaults=(L_GRID, 0))


# ---- the dispatch, restated

def runtime_in_chunk(nout):
    return MAX_IN_RUNTIME if nout <= 5 else MAX_IN_RUNTIME_WIDE


def rolled(nout, ninb):
    """BitLoop<NOUT, NINB>::kRolled."""
    return nout * ninb >= 40


def pipe_fits(nout, ninb):
    """kPipeFits<NOUT, NINB>."""
    return not rolled(nout, ninb) and 16 * ninb + 8 * nout <= 232


def ninb_ladder(nout):
    """The NINB steps launch_bits<NOUT> has."""
    return (4, 8, 12, 16) if nout < 6 else (4, 8)


def ninb_of(nout, nin):
    for b in ninb_ladder(nout):
        if nin <= b:
            return b
    raise ValueError("launch_bits<%d> takes no %d inputs" % (nout, nin))


def plain_name(nout, ninb):
    return "bitsliced_kernel<%d, %d>" % (nout, ninb)


def pipe_name(nout, ninb):
    return "bitsliced_pipe_kernel<%d, %d>" % (nout, ninb)


def stream_name(nout):
    return "bitsliced_stream_kernel<%d, 4>" % nout


def xor_name(nin):
    return "xor_kernel<%d>" % next(b for b in (4, 8, 12, 16) if nin <= b)


def bits_name(nout, nin, pipe):
    b = ninb_of(nout, nin)
    return pipe_name(nout, b) if pipe and pipe_fits(nout, b) else plain_name(nout, b)


def routes(nout, nlive, mode, pipe=True, ones=False, windows=True):
    """run_apply's launches over the whole windows of a call, in order:
    [(kernel name as hrs_last_kernel spells it, nin, accumulate)]. ones: a
    single output whose live coefficients are all 1. windows=False: the call
    has no whole window the vector kernels may take (unaligned rows, L < 2048;
    mode 2 implies it), so every launch is the byte-granular kernel's. The
    row tails' byte-granular launches behind a vector launch are not listed:
    they do not change the call's lastKernel()."""
    assert mode in (0, 1, 2) and nout >= 1 and nlive >= 1
    windows = windows and mode != 2
    if nout == 1 and ones and windows and mode == 0:
        return [(xor_name(min(MAX_IN_RUNTIME, nlive - i0)), min(MAX_IN_RUNTIME, nlive - i0), i0 > 0)
                for i0 in range(0, nlive, MAX_IN_RUNTIME)]
    out = []
    for o0 in range(0, nout, MAX_OUT):
        no = min(MAX_OUT, nout - o0)
        resident = runtime_in_chunk(no)
        stream = mode == 0 and windows and (nlive > resident or (nlive > 12 and no >= 3))
        chunk = MAX_IN if stream else resident
        for i0 in range(0, nlive, chunk):
            ni = min(chunk, nlive - i0)
            name = BYTEWISE if not windows else stream_name(no) if stream else bits_name(no, ni, pipe)
            out.append((name, ni, i0 > 0))
    return out


def instantiations():
    """Every kernel run_apply's runtime routes can launch, by family."""
    plain = {plain_name(o, b) for o in NOUTS for b in ninb_ladder(o)}
    pipe = {pipe_name(o, b) for o in NOUTS for b in ninb_ladder(o) if pipe_fits(o, b)}
    return {"plain": plain, "pipe": pipe, "stream": {stream_name(o) for o in NOUTS},
            "xor": {xor_name(n) for n in (4, 8, 12, 16)}, "bytewise": {BYTEWISE}}


def twin(name):
    """The plain kernel HRS_PIPE=0 runs in place of a pipelined one."""
    return name.replace("bitsliced_pipe_kernel", "bitsliced_kernel")


# ---- the window -> wave assignment, restated

def walk_lengths(ntasks, order, grid):
    """Tasks per wave of a launch of `grid` blocks (wave_tasks, hrs_device.hpp;
    the _walks of test_gpu_ragged_waves.py, counted)."""
    out = []
    for b in range(grid):
        for w in range(WPB):
            if order >= 1:
                t0, jump, end = b * order * WPB + w, grid * order * WPB, ntasks
                at = lambda j: t0 + (j // order) * jump + (j % order) * WPB  # noqa: E731
            else:
                per = -(-ntasks // grid)
                t0, end = per * b + w, min(per * b + per, ntasks)
                at = lambda j: t0 + j * WPB  # noqa: E731
            j = 0
            while at(j) < end:
                j += 1
            out.append(j)
    return out


def launch_grid(ntasks, cus=256, per_cu=2):
    """stream_grid (hrs_launch.hpp) without a grid cap."""
    return max(1, min(-(-ntasks // WPB), per_cu * cus))


def stripes_of(nlive):
    return 1 + nlive % 3


# windows per wave of block 0 under HRS_TASK_ORDER=32, by stripe count, at L_GRID
ORDER32_WALKS = {1: [2, 2, 2, 1], 2: [4, 4, 3, 3], 3: [6, 5, 5, 5]}


def check_walks(S, order, cus=256, L=L_GRID):
    """The walk lengths the grid's launches have; asserts what the tests rely
    on: under order 32 block 0's four waves run every window (2/1, 4/3 or 6/5
    each) and no other wave runs any; under the default order no wave runs
    more than one."""
    assert "HRS_BLOCKS_PER_CU" not in os.environ, \
        "HRS_BLOCKS_PER_CU changes the grid these cases' wave schedules are checked for: unset it"
    ntasks = S * (L // WINDOW)
    grid = launch_grid(ntasks, cus)
    assert grid <= 6
    lengths = walk_lengths(ntasks, order, grid)
    assert sum(lengths) == ntasks
    if order == 32 and L == L_GRID:
        assert lengths[:WPB] == ORDER32_WALKS[S] and not any(lengths[WPB:]), lengths
    if order == 1:
        assert max(lengths) == 1, lengths
    return lengths


# ---- matrices

def _random(nout, nlive, seed):
    rng = np.random.default_rng([seed, nout, nlive])
    if nout == 1:  # a zero here would be a dead column (kind "dead"), all ones the XOR route (kind "ones")
        m = rng.integers(1, 256, (1, nlive), dtype=np.uint8)
        if (m == 1).all():
            m[0, 0] = 2
        return m
    m = rng.integers(0, 256, (nout, nlive), dtype=np.uint8)
    for i in range(nlive):
        if not m[:, i].any():
            m[i % nout, i] = 1 + i % 255
    if nout * nlive >= 4 and m.all():
        m[0, 0] = 0
        if not m[:, 0].any():
            m[1, 0] = 3
    return m


def matrix(kind, nout, nlive):
    """(m[nout, nin] uint8, the input indices passed as None). nin = nlive
    except for "dead", which has three all-zero columns more."""
    if kind == "random":
        return _random(nout, nlive, 1), ()
    if kind in ("bits", "bits7"):
        add = 4 if kind == "bits7" else 0
        return np.array([[1 << ((o + i + add) % 8) for i in range(nlive)] for o in range(nout)], np.uint8), ()
    if kind == "sparse":
        rng = np.random.default_rng([2, nout, nlive])
        zero_row = nlive % nout if nout >= 2 else None
        live_rows = [o for o in range(nout) if o != zero_row]
        m = np.zeros((nout, nlive), np.uint8)
        for i in range(nlive):
            m[live_rows[i % len(live_rows)], i] = rng.integers(2, 256)
        return m, ()
    if kind == "dead":
        nin = nlive + 3
        null = (0, nin // 2, nin - 1)
        m = np.zeros((nout, nin), np.uint8)
        m[:, [i for i in range(nin) if i not in null]] = _random(nout, nlive, 3)
        return m, null
    if kind == "ones":
        assert nout == 1
        return np.ones((1, nlive), np.uint8), ()
    raise ValueError(kind)


def all_ones(m):
    live = m[:, m.any(axis=0)]
    return m.shape[0] == 1 and bool((live == 1).all())


def pipe_on():
    """use_pipe (hrs_runtime.hip) for this process."""
    return not os.environ.get("HRS_PIPE", "").startswith("0")


def case_routes(case, pipe=None):
    case = Case(*case)
    m, _ = matrix(case.kind, case.nout, case.nlive)
    windows = case.shift == 0 and case.L >= WINDOW
    return routes(case.nout, case.nlive, case.mode, pipe_on() if pipe is None else pipe, all_ones(m), windows)


def last_kernel(case, pipe=None):
    """What lastKernel() must say after the case."""
    return case_routes(case, pipe)[-1][0]


# ---- case lists

def mode0_cases(nout):
    return [Case(nout, n, kind, 0) for n in NLIVES for kind in ("random", "bits") + (("bits7",) if n < 8 else ())]


def mode1_cases(nout):
    return [Case(nout, n, "random", 1) for n in NLIVES]


SPARSE_DEAD_NLIVES = (1, 4, 5, 12, 13, 16, 17, 32, 33)


def sparse_dead_cases(nout):
    return [Case(nout, n, kind, 0) for n in SPARSE_DEAD_NLIVES for kind in ("sparse", "dead")]


def xor_cases():
    return [Case(1, n, "ones", mode) for mode in (0, 1) for n in NLIVES]


def output_chunk_cases():
    return [Case(nout, n, "random", 0) for nout in (9, 13, 16, 17) for n in (5, 12, 20, 33)]


def byte_granular_cases(nout):
    """Rows under one window; whole windows on views one byte off their
    alignment; and aligned whole windows under kernel mode 2."""
    out = [Case(nout, n, "random", 0, L, shift) for L, shift in ((100, 0), (L_GRID, 1)) for n in (1, 16, 17, 40)]
    return out + [Case(nout, 17, "random", 2)]


def default_order_cases():
    return [Case(nout, n, "random", 0) for nout in NOUTS for n in (4, 8, 12, 16, 24, 32)]


def pipe_classes():
    """The (nout, NINB) pairs with a pipelined kernel."""
    return [(o, b) for o in NOUTS for b in ninb_ladder(o) if pipe_fits(o, b)]


def pipe_twin_cases():
    """Per pipe-fitting class one nlive at its bottom and one at its top, in
    modes 0 and 1 (one launch each), and in mode 1 the top once more behind a
    full first chunk, where the class's kernel accumulates."""
    out = []
    for o, b in pipe_classes():
        out += [Case(o, n, "random", mode) for mode in (0, 1) for n in (b - 3, b)]
        out.append(Case(o, runtime_in_chunk(o) + b, "random", 1))
    return out


LISTS = {
    "mode0": lambda: [c for o in NOUTS for c in mode0_cases(o)],
    "mode1": lambda: [c for o in NOUTS for c in mode1_cases(o)],
    "sparse_dead": lambda: [c for o in NOUTS for c in sparse_dead_cases(o)],
    "xor": xor_cases,
    "output_chunks": output_chunk_cases,
    "byte_granular": lambda: [c for o in NOUTS for c in byte_granular_cases(o)],
    "default_order": default_order_cases,
    "pipe_twins": pipe_twin_cases,
}


# ---- inputs and the reference

MAX_NIN = 43  # 40 live inputs and the three dead ones


@functools.lru_cache(maxsize=None)
def mul_table():
    t = np.array([[C.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def input_pool(L):
    """x[3, MAX_NIN, L]: a case takes its first S stripes and nin rows."""
    x = np.random.default_rng([4, L]).integers(0, 256, (3, MAX_NIN, L), dtype=np.uint8)
    x.setflags(write=False)
    return x


def reference(m, x):
    """out[S, nout, L] = XOR_i m[o, i] * x[:, i] over x[S, nin, L]."""
    mul = mul_table()
    S, nin, L = x.shape
    ref = np.zeros((S, m.shape[0], L), np.uint8)
    for o in range(m.shape[0]):
        for i in range(nin):
            if m[o, i]:
                ref[:, o] ^= mul[m[o, i]][x[:, i]]
    return ref


def mismatch(got, want):
    """None, or where got[S, nout, L] first differs from want."""
    differ = got != want
    if not differ.any():
        return None
    o = int(np.flatnonzero(differ.any(axis=(0, 2)))[0])  # first by output, then stripe, then byte
    s = int(np.flatnonzero(differ[:, o].any(axis=1))[0])
    b = int(np.flatnonzero(differ[s, o])[0])
    w, off = divmod(b, WINDOW)
    return "%d bytes differ; first: output %d stripe %d byte %d (window %d, lane %d, half %d): got %#x, want %#x" % (
        int(differ.sum()), o, s, b, w, off % 1024 // 16, off // 1024, int(got[s, o, b]), int(want[s, o, b]))


_device_pools = {}


def _device_pool(torch, L, shift):
    """The input pool on the device, its rows `shift` bytes into a 16-byte-
    aligned pitch of L + 16 when shifted."""
    if (L, shift) not in _device_pools:
        host = torch.from_numpy(np.array(input_pool(L)))
        if shift:
            buf = torch.zeros((3, MAX_NIN, L + 16), dtype=torch.uint8, device="cuda")
            buf[:, :, shift:shift + L] = host.to("cuda")
            _device_pools[L, shift] = buf[:, :, shift:shift + L]
        else:
            _device_pools[L, shift] = host.to("cuda")
    return _device_pools[L, shift]


def run_case(code, nout, nlive, kind, mode, L=L_GRID, shift=0):
    """One apply_rows call of the case on the device -> (mismatch or None,
    lastKernel). nlive is the matrix's number of live inputs (its nin, but for
    the three dead columns of kind "dead")."""
    import torch

    from lambdafs_amd import device
    assert "HRS_STREAM" not in os.environ, "HRS_STREAM changes the routes these cases are checked for: unset it"
    m, null = matrix(kind, nout, nlive)
    nin, S = m.shape[1], stripes_of(nlive)
    if shift == 0 and L >= WINDOW and mode != 2:
        order = int(os.environ.get("HRS_TASK_ORDER") or 1)
        check_walks(S, order, torch.cuda.get_device_properties(0).multi_processor_count, L)
    x = _device_pool(torch, L, shift)
    pitch = L + 16 if shift else L
    ybuf = torch.full((S, nout, pitch), POISON, dtype=torch.uint8, device="cuda")
    y = ybuf[:, :, shift:shift + L]
    code.setKernelMode(mode)
    device.apply_rows(code, m, [None if i in null else x[:S, i] for i in range(nin)], [y[:, o] for o in range(nout)])
    kernel = code.lastKernel()
    got = ybuf.cpu().numpy()
    bad = mismatch(got[:, :, shift:shift + L], reference(m, input_pool(L)[:S, :nin]))
    if bad is None and shift and not ((got[:, :, :shift] == POISON).all() and (got[:, :, shift + L:] == POISON).all()):
        bad = "bytes outside the output views were written"
    return bad, kernel


def main(argv):
    from lambdafs_amd import HipReedSolomonCode
    names = argv or sorted(LISTS)
    unknown = [n for n in names if n not in LISTS]
    if unknown:
        print("unknown case list(s) %s; known: %s" % (unknown, sorted(LISTS)), file=sys.stderr)
        return 2
    code = HipReedSolomonCode(10, 4)
    failed = 0
    for name in names:
        for case in LISTS[name]():
            bad, kernel = run_case(code, *case)
            want = last_kernel(case)
            failed += bad is not None or kernel != want
            print(json.dumps({"list": name, **case._asdict(), "kernel": kernel, "want_kernel": want, "mismatch": bad}),
                  flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
