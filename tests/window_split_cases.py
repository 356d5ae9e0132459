"""Cases of tests/test_gpu_window_split.py: the kernels that take the window
map (hrs_window_map.hpp: plain static encodes, runtime-matrix repairs, the
streaming apply and the chunked accumulate launches) at the shapes that put a
row through every part of the map, each compared bit for bit, over the whole
output tensor, with the byte-granular kernel (kernel mode 2: no windows, so no
map), whose result is itself checked against the oracle on stripes 0, S/2 and
S - 1. The references depend on the shape alone and are computed once.

Rows are laid out with a pitch that is a multiple of 64 bytes, so that a row
length with a tail (… + 100) still takes the 16-byte-aligned window kernels
for its whole windows and the byte-granular kernel for the tail only; every
case asserts the kernel the call reports.

Run as a program (`python tests/window_split_cases.py stream0`, started by the
test with HRS_STREAM=0, which the library reads once per process) it runs the
20-input apply over every (H, order, shape) and prints one JSON line per case.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K, P = 10, 4
N = K + P
SHAPES = {
    2048: [(1, 4096), (3, 4096 + 2048 + 100), (7, 5 * 4096), (513, 8192)],
    65536: [(1, 65536), (2, 131072), (3, 131072 + 2048 + 100), (5, 393216)],
}
ORDERS = [1, 0, 2]
ERASED = [[4], [0, 5], [1, 6, 11], [0, 1, 2, 3]]
APPLY_IN, APPLY_OUT = 20, 2
CASES = [(h, o, s, l) for h in SHAPES for o in ORDERS for (s, l) in SHAPES[h]]

# the kernel each call reports (lastKernel): pipelined repairs for 1-3 losses,
# the plain (rolled) kernel for 4; 20 inputs stream, or go 16 + 4 accumulating
KERNELS = {
    "rs": "encode_static_kernel<10, 4>",
    "nrs": "encode_cauchy_kernel<10, 4>",
    1: "bitsliced_pipe_kernel<1, 12>",
    2: "bitsliced_pipe_kernel<2, 12>",
    3: "bitsliced_pipe_kernel<3, 12>",
    4: "bitsliced_kernel<4, 12>",
    "apply_stream": "bitsliced_stream_kernel<2, 4>",
    "apply_chunked": "bitsliced_pipe_kernel<2, 4>",
}

_cache = {}
_mul = []


def set_knobs(h, order):
    os.environ["HRS_WINDOW_SPLIT"] = str(h)
    os.environ["HRS_TASK_ORDER"] = str(order)


def sample(S):
    return sorted({0, S // 2, S - 1})


def rows_tensor(torch, S, m, L, seed=None, fill=None):
    """[S, m, L] uint8 on the device with a row pitch that is a multiple of 64."""
    pitch = (L + 63) // 64 * 64
    if seed is None:
        t = torch.full((S, m, pitch), fill, dtype=torch.uint8, device="cuda")
    else:
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        t = torch.randint(0, 256, (S, m, pitch), dtype=torch.uint8, device="cuda", generator=g)
    return t[:, :, :L]


def _code(kind):
    from lambdafs_amd import HipNativeReedSolomonCode, HipReedSolomonCode
    return (HipNativeReedSolomonCode if kind == "nrs" else HipReedSolomonCode)(K, P)


def _bytewise(code, fn):
    """fn() on the byte-granular kernel: one byte column per lane, no windows,
    so neither the window order nor the window map reaches it."""
    code.setKernelMode(2)
    try:
        fn()
    finally:
        code.setKernelMode(0)
    assert code.lastKernel() == "bytewise_kernel", code.lastKernel()


def _gf_products(m, x):
    from oracle import rs_oracle as C
    if not _mul:
        _mul.append(np.array([[C.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8))
    out = [np.zeros_like(x[0]) for _ in range(m.shape[0])]
    for o in range(m.shape[0]):
        for i, r in enumerate(x):
            if m[o, i]:
                out[o] ^= _mul[0][m[o, i]][r]
    return out


def encode_ref(torch, kind, S, L):
    """(stripes with the byte-granular kernel's parity, oracle-checked)."""
    from lambdafs_amd import device
    from oracle import rs_oracle as C
    key = ("enc", kind, S, L)
    if key not in _cache:
        code = _code(kind)
        st = rows_tensor(torch, S, N, L, seed=S * 7 + L)
        st[:, :P] = 0x33
        _bytewise(code, lambda: device.encode_stripes(code, st))
        torch.cuda.synchronize()
        for s in sample(S):
            host = st[s].cpu().numpy()
            enc = C.nrs_encode_bulk if kind == "nrs" else C.encode_bulk
            ref = np.stack(enc(K, P, [host[P + c] for c in range(K)]))
            assert np.array_equal(host[:P], ref), (kind, S, L, s)
        _cache[key] = st
    return _cache[key]


def check_encode(torch, kind, S, L):
    from lambdafs_amd import device
    ref = encode_ref(torch, kind, S, L)
    code = _code(kind)
    st = rows_tensor(torch, S, N, L, fill=0xA5)
    st.copy_(ref)
    st[:, :P] = 0xA5
    device.encode_stripes(code, st)
    torch.cuda.synchronize()
    assert code.lastKernel() == KERNELS[kind], code.lastKernel()
    assert torch.equal(st, ref), (kind, S, L)


def repair_ref(torch, erased, S, L):
    from lambdafs_amd import device
    from oracle import rs_oracle as C
    key = ("rep", tuple(erased), S, L)
    if key not in _cache:
        code = _code("rs")
        st = rows_tensor(torch, S, N, L, seed=S * 3 + L)  # not codewords: every coefficient counts
        to_read = sorted(C.locations_to_read(K, P, erased))
        ntr = [x for x in range(N) if x not in to_read]
        out = rows_tensor(torch, S, len(erased), L, fill=0x33)
        _bytewise(code, lambda: device.decode_stripes(code, st, erased, ntr, out))
        torch.cuda.synchronize()
        for s in sample(S):
            host, got = st[s].cpu().numpy(), out[s].cpu().numpy()
            reads = [host[i] if i in to_read else np.zeros(L, np.uint8) for i in range(N)]
            ref = C.decode_bulk5(K, P, reads, erased, to_read, ntr)
            for i in range(len(erased)):
                assert np.array_equal(got[i], ref[i]), (erased, S, L, s, i)
        _cache[key] = (st, ntr, out)
    return _cache[key]


def check_repair(torch, erased, S, L):
    from lambdafs_amd import device
    st, ntr, ref = repair_ref(torch, erased, S, L)
    code = _code("rs")
    out = rows_tensor(torch, S, len(erased), L, fill=0x5A)
    device.decode_stripes(code, st, erased, ntr, out)
    torch.cuda.synchronize()
    assert code.lastKernel() == KERNELS[len(erased)], code.lastKernel()
    assert torch.equal(out, ref), (erased, S, L)


def apply_matrix():
    m = np.random.default_rng(2002).integers(1, 256, (APPLY_OUT, APPLY_IN), dtype=np.uint8)
    return m


def apply_ref(torch, S, L):
    from lambdafs_amd import device
    key = ("apply", S, L)
    if key not in _cache:
        code = _code("rs")
        m = apply_matrix()
        x = rows_tensor(torch, S, APPLY_IN, L, seed=S * 11 + L)
        y = rows_tensor(torch, S, APPLY_OUT, L, fill=0x33)
        _bytewise(code, lambda: device.apply_rows(code, m, [x[:, i] for i in range(APPLY_IN)],
                                                  [y[:, o] for o in range(APPLY_OUT)]))
        torch.cuda.synchronize()
        for s in sample(S):
            ref = _gf_products(m, [x[s, i].cpu().numpy() for i in range(APPLY_IN)])
            for o in range(APPLY_OUT):
                assert np.array_equal(y[s, o].cpu().numpy(), ref[o]), (S, L, s, o)
        _cache[key] = (m, x, y)
    return _cache[key]


def check_apply(torch, S, L, kernel):
    from lambdafs_amd import device
    m, x, ref = apply_ref(torch, S, L)
    code = _code("rs")
    y = rows_tensor(torch, S, APPLY_OUT, L, fill=0x5A)
    device.apply_rows(code, m, [x[:, i] for i in range(APPLY_IN)], [y[:, o] for o in range(APPLY_OUT)])
    torch.cuda.synchronize()
    assert code.lastKernel() == kernel, code.lastKernel()
    assert torch.equal(y, ref), (S, L)


def main(argv):
    import torch
    assert argv[1:] == ["stream0"] and os.environ.get("HRS_STREAM") == "0", "run by tests/test_gpu_window_split.py"
    for h, order, S, L in CASES:
        set_knobs(h, order)
        err = None
        try:
            check_apply(torch, S, L, KERNELS["apply_chunked"])
        except AssertionError as e:
            err = repr(e)
        print(json.dumps({"split": h, "order": order, "S": S, "L": L, "error": err}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
