"""What test_gpu_apply_grid.py relies on, checked without a device: the
routing model of apply_grid.py names the kernels the dispatch source says it
does, the matrix kinds have their stated properties at every shape of the
grid, the waves walk the windows as stated, and no case is left out.

The kernel counts are derived from the source rules, not from a run:
  launch_bits<NOUT> has the NINB steps 4, 8, 12, 16 for NOUT <= 5 and 4, 8
  for NOUT 6..8: 5 * 4 + 3 * 2 = 26 bitsliced_kernel instantiations. kRolled
  is NOUT * NINB >= 40: <5..8, 8>, <4..5, 12>, <3..5, 16>, nine of them.
  kPipeFits is !kRolled and 16 NINB + 8 NOUT <= 232: <1..8, 4>, <1..4, 8>,
  <1..3, 12>, 15 pipelined kernels. One streaming kernel per NOUT, 8.
  Mode 0 keeps a shape resident up to 16 inputs with 1-2 outputs, 12 with
  3-5, 8 with 6-8 (8 + 3 * 3 + 3 * 2 = 23 names) and streams the rest (8
  names): 31. Only the streaming kernels meet a second chunk there (33..40
  inputs). Mode 1 never streams, so every resident name runs as a first and as
  a later chunk: 26, of which <3..5, 16> are the three mode 0 never reaches.

Two properties the kinds cannot have at every shape, and what is asserted
in their place:
  "random" at one output has no zero entry: a zero there is an all-zero
  column, which would make the input dead (that is the kind "dead"). The zero
  entry is required from two outputs on.
  "bits" and "bits7" together set 2 * nin distinct bits per output when
  nin < 4 (two matrices of nin columns cannot set more); all eight from
  nin = 4 on."""
import numpy as np
import pytest

import apply_grid as G
from oracle import rs_oracle as C

GRID = [(o, n) for o in G.NOUTS for n in G.NLIVES]


def _names(mode, pipe=True, accumulating=False):
    return {name for o, n in GRID for name, _, acc in G.routes(o, n, mode, pipe) if acc or not accumulating}


def test_instantiation_counts():
    inst = G.instantiations()
    assert [len(inst[f]) for f in ("plain", "pipe", "stream", "xor", "bytewise")] == [26, 15, 8, 4, 1]
    assert sum(G.rolled(o, b) for o in G.NOUTS for b in G.ninb_ladder(o)) == 9
    assert len(G.pipe_classes()) == 15
    assert {G.twin(p) for p in inst["pipe"]} <= inst["plain"]
    assert not any(G.rolled(o, b) for o, b in G.pipe_classes())


def test_mode0_names_31_kernels_8_of_them_accumulating():
    assert len(_names(0)) == 31
    acc = _names(0, accumulating=True)
    assert acc == G.instantiations()["stream"] and len(acc) == 8


def test_mode1_names_26_kernels_all_of_them_accumulating():
    assert len(_names(1)) == 26
    assert _names(1, accumulating=True) == _names(1)


def test_pipe_off_gives_the_plain_twins():
    inst = G.instantiations()
    for mode in (0, 1):
        on, off = _names(mode), _names(mode, pipe=False)
        assert off == {G.twin(n) for n in on}
        assert not off & inst["pipe"]
    assert _names(1, pipe=False) == inst["plain"]
    assert inst["pipe"] <= _names(0) | _names(1)


def test_modes_0_and_1_cover_all_but_the_plain_twins():
    inst = G.instantiations()
    twins = {G.twin(p) for p in inst["pipe"]}
    assert _names(0) | _names(1) == (inst["plain"] | inst["pipe"] | inst["stream"]) - twins
    assert len(_names(0) | _names(1)) == 26 + 15 + 8 - 15


def test_routes_chunking():
    assert G.routes(1, 20, 0) == [("bitsliced_stream_kernel<1, 4>", 20, False)]
    assert G.routes(2, 17, 0) == [("bitsliced_stream_kernel<2, 4>", 17, False)]
    assert G.routes(1, 20, 1) == [("bitsliced_kernel<1, 16>", 16, False), ("bitsliced_pipe_kernel<1, 4>", 4, True)]
    assert G.routes(3, 13, 0) == [("bitsliced_stream_kernel<3, 4>", 13, False)]
    assert G.routes(2, 16, 0) == [("bitsliced_kernel<2, 16>", 16, False)]
    assert G.routes(8, 40, 0) == [("bitsliced_stream_kernel<8, 4>", 32, False), ("bitsliced_stream_kernel<8, 4>", 8, True)]
    assert G.routes(7, 20, 1) == [("bitsliced_kernel<7, 8>", 8, False), ("bitsliced_kernel<7, 8>", 8, True),
                                  ("bitsliced_pipe_kernel<7, 4>", 4, True)]
    assert G.routes(9, 12, 0) == [("bitsliced_stream_kernel<8, 4>", 12, False), ("bitsliced_pipe_kernel<1, 12>", 12, False)]
    assert G.routes(1, 37, 0, ones=True) == [("xor_kernel<16>", 16, False), ("xor_kernel<16>", 16, True),
                                             ("xor_kernel<8>", 5, True)]
    assert G.routes(1, 37, 1, ones=True)[-1] == ("bitsliced_pipe_kernel<1, 8>", 5, True)
    assert G.routes(6, 17, 0, windows=False) == [(G.BYTEWISE, 8, False), (G.BYTEWISE, 8, True), (G.BYTEWISE, 1, True)]
    assert G.routes(3, 40, 2) == [(G.BYTEWISE, 16, False), (G.BYTEWISE, 16, True), (G.BYTEWISE, 8, True)]


def test_the_gpu_cases_last_kernels_are_every_instantiation():
    """lastKernel() names a call's last vector launch, so it is the cases'
    LAST routes that the device tests pin: together they must still be every
    kernel the runtime-matrix routes can launch, the plain twins coming from
    the child that runs with HRS_PIPE=0."""
    inst = G.instantiations()
    in_process = {G.last_kernel(c, pipe=True) for name, cases in G.LISTS.items() if name != "pipe_twins" for c in cases()}
    twins = {G.last_kernel(c, pipe=False) for c in G.pipe_twin_cases()}
    assert twins == {G.twin(p) for p in inst["pipe"]} and len(twins) == 15
    assert in_process | twins == set().union(*inst.values())
    for o in G.NOUTS:  # per nout, the grid tests see what routes names for that nout
        assert {G.last_kernel(c, True) for c in G.mode0_cases(o)} >= {r[0] for n in G.NLIVES for r in G.routes(o, n, 0)}
        assert {G.last_kernel(c, True) for c in G.mode1_cases(o)} == {r[0] for n in G.NLIVES for r in G.routes(o, n, 1)}
    # the resident and pipelined kernels' accumulate branch, every one as a last launch
    acc = {G.case_routes(c, True)[-1][0] for o in G.NOUTS for c in G.mode1_cases(o) if G.case_routes(c, True)[-1][2]}
    assert acc == _names(1)
    assert {G.last_kernel(c, True) for c in G.xor_cases() if c.mode == 0} == inst["xor"]
    assert {G.last_kernel(c, True) for o in G.NOUTS for c in G.byte_granular_cases(o)} == inst["bytewise"]


def test_no_case_is_left_out():
    """Every list is the whole product its test names: nothing filtered."""
    for o in G.NOUTS:
        assert len(G.mode0_cases(o)) == 40 * 2 + 7 and len(G.mode1_cases(o)) == 40
        assert {(c.nlive, c.kind) for c in G.mode0_cases(o)} == (
            {(n, k) for n in G.NLIVES for k in ("random", "bits")} | {(n, "bits7") for n in range(1, 8)})
        assert [c.nlive for c in G.mode1_cases(o)] == list(G.NLIVES)
        assert len(G.sparse_dead_cases(o)) == 9 * 2
        assert len(G.byte_granular_cases(o)) == 2 * 4 + 1
    assert len(G.xor_cases()) == 2 * 40
    assert len(G.output_chunk_cases()) == 4 * 4
    assert len(G.default_order_cases()) == 8 * 6
    assert len(G.pipe_twin_cases()) == 15 * 5
    for cases in G.LISTS.values():
        for c in cases():
            assert G.case_routes(c, True) and G.case_routes(c, False)
            m, null = G.matrix(c.kind, c.nout, c.nlive)
            assert m.shape == (c.nout, c.nlive + len(null)) and m.shape[1] <= G.MAX_NIN


def test_pipe_twin_cases_sit_at_the_classes_edges():
    for o, b in G.pipe_classes():
        mine = [c for c in G.pipe_twin_cases() if c.nout == o and G.last_kernel(c, False) == G.plain_name(o, b)]
        assert sorted((c.mode, c.nlive) for c in mine) == sorted(
            [(0, b - 3), (0, b), (1, b - 3), (1, b), (1, G.runtime_in_chunk(o) + b)])
        assert [G.case_routes(c, False)[-1][2] for c in mine].count(True) == 1


SHAPES = sorted(set(GRID) | {(c.nout, c.nlive) for c in G.output_chunk_cases()})


def test_random_matrices():
    for o, n in SHAPES:
        m, null = G.matrix("random", o, n)
        assert m.dtype == np.uint8 and m.shape == (o, n) and null == ()
        assert m.any(axis=0).all()
        assert not G.all_ones(m)
        if o >= 2 and o * n >= 4:
            assert (m == 0).any()
    assert max(int(G.matrix("random", o, n)[0].max()) for o, n in GRID) > 127


def test_bit_matrices_set_every_output_bit():
    for o, n in GRID:
        b0, b7 = G.matrix("bits", o, n)[0], G.matrix("bits7", o, n)[0]
        assert (b0 == [[1 << ((r + i) % 8) for i in range(n)] for r in range(o)]).all()
        assert (b7 == [[1 << ((r + i + 4) % 8) for i in range(n)] for r in range(o)]).all()
        for r in range(o):
            bits = {int(v).bit_length() - 1 for v in b0[r]} | ({int(v).bit_length() - 1 for v in b7[r]} if n < 8 else set())
            assert len(bits) == min(8, 2 * n)


def test_sparse_matrices():
    for o, n in GRID:
        m, null = G.matrix("sparse", o, n)
        assert null == () and ((m != 0).sum(axis=0) == 1).all()
        assert not G.all_ones(m)
        if o >= 2:
            assert not m[n % o].any()


def test_dead_matrices():
    for o, n in GRID:
        m, null = G.matrix("dead", o, n)
        nin = n + 3
        assert m.shape == (o, nin) and len(set(null)) == 3
        assert null[0] == 0 and null[2] == nin - 1 and 0 < null[1] < nin - 1
        assert [i for i in range(nin) if not m[:, i].any()] == list(null)


def test_ones_matrices():
    for n in G.NLIVES:
        m, null = G.matrix("ones", 1, n)
        assert m.shape == (1, n) and (m == 1).all() and G.all_ones(m) and null == ()


def test_walk_lengths():
    assert G.L_GRID == 7 * 2048 + 48 and G.L_GRID % 16 == 0
    assert {G.stripes_of(n) for n in G.NLIVES} == {1, 2, 3}
    for S, want in ((1, [2, 2, 2, 1]), (2, [4, 4, 3, 3]), (3, [6, 5, 5, 5])):
        for cus in (3, 64, 256):
            grid = G.launch_grid(7 * S, cus)
            assert grid == -(-7 * S // 4) <= 6
            lengths = G.check_walks(S, 32, cus)
            assert lengths[:4] == want and sum(lengths[4:]) == 0
            assert sorted(G.check_walks(S, 1, cus)) == [0] * (4 * grid - 7 * S) + [1] * (7 * S)
    # every NINB class spans four consecutive nin, so every instantiation meets all three stripe counts
    for lo in range(1, 38, 4):
        assert {G.stripes_of(n) for n in range(lo, lo + 4)} == {1, 2, 3}
    # the two orders the launches can have, against a walk written out by hand
    assert G.walk_lengths(21, 32, 6) == [6, 5, 5, 5] + [0] * 20
    assert G.walk_lengths(21, 1, 6) == [1] * 21 + [0] * 3
    assert G.walk_lengths(21, 0, 6) == [1, 1, 1, 1] * 5 + [1, 0, 0, 0]


def test_check_walks_refuses_a_changed_grid(monkeypatch):
    monkeypatch.setenv("HRS_BLOCKS_PER_CU", "1")
    with pytest.raises(AssertionError):
        G.check_walks(1, 32)


def test_reference_and_mismatch():
    rng = np.random.default_rng(7)
    m = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    x = rng.integers(0, 256, (2, 5, 9), dtype=np.uint8)
    ref = G.reference(m, x)
    for s in range(2):
        for o in range(3):
            for b in range(9):
                want = 0
                for i in range(5):
                    want ^= C.gf_mul(int(m[o, i]), int(x[s, i, b]))
                assert ref[s, o, b] == want
    assert G.mismatch(ref, ref) is None
    got = ref.copy()
    got[1, 2, 4] ^= 1
    got[0, 2, 7] ^= 1
    assert "2 bytes differ; first: output 2 stripe 0 byte 7 " in G.mismatch(got, ref)
    pool = G.input_pool(100)
    assert pool.shape == (3, G.MAX_NIN, 100) and not pool.flags.writeable
