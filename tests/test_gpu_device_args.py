"""GPU tests of lambdafs_amd/device.py's own layer: the refusals that need a
device tensor to be reached (CRC tensors, decode_batch's dtypes, row-view
counts), none of which may launch anything; the two *_rows wrappers that had
no test, heal_erased_rows and repair_checked_rows, against their *_stripes
forms and the host references; and the CRC wrappers over empty cells."""
import random

import numpy as np
import pytest

import heal_erased_inputs as H
import repair_checked_inputs as R
from lambdafs_amd import HipReedSolomonCode, device

pytestmark = pytest.mark.gpu

NONE = -2  # HRS_DEVICE_NONE
K, P, S = 6, 3, 3
N = K + P
E = 2
LENGTHS = [2 * H.WINDOW, H.WINDOW + 48]  # two whole windows; one window and a ragged tail
ERASED_SE = np.array([[0, 5], [3, -1], [-1, -1]], np.int32)
ERASED_LISTS = [[2], [], [0, 8]]


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def on_device(torch, host):
    return torch.from_numpy(np.array(host)).to("cuda:0")


def row_views(torch, host):
    """host[S, n, L] as n strided [S, L] views cut out of a wider [S, n, L + 64] tensor."""
    s, n, length = host.shape
    wide = torch.full((s, n, length + 64), 0xC3, dtype=torch.uint8, device="cuda:0")
    wide[:, :, :length].copy_(on_device(torch, host))
    return wide, [wide[:, l, :length] for l in range(n)]


def empty_cells(torch, rows=N, stripes=S):
    """A [S, rows, 0] batch, cut from whole cells (torch gives it no address all the same)."""
    return torch.zeros((stripes, rows, 16), dtype=torch.uint8, device="cuda:0")[:, :, :0]


# ------------------------------------------------------------------ refusals

def crc_calls(torch, st, crc_kw):
    """name -> (call with the CRC keywords given, width of its CRC tensors)."""
    out = torch.zeros((S, E, st.shape[2]), dtype=torch.uint8, device="cuda:0")
    views = [st[:, l] for l in range(N)]
    return {
        "encode_stripes_crc": (lambda c: device.encode_stripes_crc(c, st, **crc_kw), N),
        "decode_stripes_crc": (lambda c: device.decode_stripes_crc(c, st, [0, 5], [1], out, **crc_kw), E),
        "crc32_rows": (lambda c: device.crc32_rows(c, views, **crc_kw), N),
        "scrub_stripes_crc": (lambda c: device.scrub_stripes_crc(c, st, **crc_kw), N),
        "heal_erased_stripes_crc": (lambda c: device.heal_erased_stripes_crc(c, st, ERASED_LISTS, **crc_kw), N),
        "decode_batch_crc": (lambda c: device.decode_batch_crc(c, st, ERASED_SE, out, **crc_kw), E),
    }


def bad_crc_in(torch, width):
    dev = dict(dtype=torch.int32, device="cuda:0")
    return {
        "on_the_cpu": torch.zeros((S, width), dtype=torch.int32),
        "int64": torch.zeros((S, width), dtype=torch.int64, device="cuda:0"),
        "one_column_more": torch.zeros((S, width + 1), **dev),
        "one_row_more": torch.zeros((S + 1, width), **dev),
        "transposed": torch.zeros((width, S), **dev).T,
        "every_other_column": torch.zeros((S, 2 * width), **dev)[:, ::2],
    }


@pytest.mark.parametrize("bad", ["on_the_cpu", "int64", "one_column_more", "one_row_more", "transposed",
                                 "every_other_column"])
@pytest.mark.parametrize("name", ["encode_stripes_crc", "decode_stripes_crc", "crc32_rows", "scrub_stripes_crc",
                                  "heal_erased_stripes_crc", "decode_batch_crc"])
def test_crc_wrappers_refuse_a_bad_crc_in(cuda, name, bad):
    torch = cuda
    st = torch.zeros((S, N, 64), dtype=torch.uint8, device="cuda:0")
    width = crc_calls(torch, st, {})[name][1]
    call, _ = crc_calls(torch, st, dict(crc_in=bad_crc_in(torch, width)[bad]))[name]
    code = HipReedSolomonCode(K, P, device=0)
    with pytest.raises(ValueError):
        call(code)
    torch.cuda.synchronize()
    assert code.lastKernel() == "" and not st.any()  # nothing ran


def test_decode_batch_refuses_other_dtypes(cuda):
    torch = cuda
    code = HipReedSolomonCode(K, P, device=0)
    st = torch.zeros((S, N, 64), dtype=torch.uint8, device="cuda:0")
    out = torch.zeros((S, E, 64), dtype=torch.uint8, device="cuda:0")
    for call in (device.decode_batch, device.decode_batch_crc):
        with pytest.raises(ValueError):
            call(code, st.view(torch.int8), ERASED_SE, out)
        with pytest.raises(ValueError):
            call(code, st, ERASED_SE, out.view(torch.int8))
        with pytest.raises(ValueError):
            call(code, st, ERASED_SE, torch.zeros((S, E, 16), dtype=torch.int32, device="cuda:0"))
        with pytest.raises(ValueError):
            call(code, st, ERASED_SE, out.cpu())
    torch.cuda.synchronize()
    assert code.lastKernel() == "" and not out.any()


ROWS_CALLS = {
    "scrub_rows": lambda c, v, stored: device.scrub_rows(c, v),
    "scrub_rows_crc": lambda c, v, stored: device.scrub_rows_crc(c, v),
    "heal_rows": lambda c, v, stored: device.heal_rows(c, v),
    "heal_rows_crc": lambda c, v, stored: device.heal_rows_crc(c, v),
    "heal_erased_rows": lambda c, v, stored: device.heal_erased_rows(c, v, ERASED_LISTS),
    "heal_erased_rows_crc": lambda c, v, stored: device.heal_erased_rows_crc(c, v, ERASED_LISTS),
    "repair_checked_rows": lambda c, v, stored: device.repair_checked_rows(c, v, stored),
}


@pytest.mark.parametrize("name", list(ROWS_CALLS))
def test_rows_wrappers_need_every_row(cuda, name):
    torch = cuda
    code = HipReedSolomonCode(K, P, device=0)
    st = torch.zeros((S, N, 64), dtype=torch.uint8, device="cuda:0")
    stored = torch.zeros((S, N), dtype=torch.int32, device="cuda:0")
    views = [st[:, l] for l in range(N)]
    with pytest.raises(ValueError):
        ROWS_CALLS[name](code, views[:-1], stored)
    with pytest.raises(ValueError):
        ROWS_CALLS[name](code, views[:4] + [None] + views[5:], stored)
    with pytest.raises(ValueError):
        ROWS_CALLS[name](code, views + views[:1], stored)
    torch.cuda.synchronize()
    assert code.lastKernel() == "" and not st.any()


# ------------------------------------- the rows form equals the stripes form

_heal_erased_cases = {}


def heal_erased_case(L):
    """(damaged, patterns, bytes after, reports) by hrs_heal_erased_host: a
    data cell lost; nothing lost; p cells lost; survivor errors planted within
    capacity at the window, piece and row edges."""
    if L not in _heal_erased_cases:
        rnd = random.Random(L)
        pats = [[P + rnd.randrange(K)], [], sorted(rnd.sample(range(N), P))]
        clean = H.clean_stripes(K, P, S, L, 21)
        bad, planted = H.plant(K, P, clean, pats, H.columns_of(L), clean_stripes_=(), seed=21)
        assert {s for s, _, _ in planted} == {0, 1}  # stripe 2 has no syndrome to spare
        after, reps = H.host_reference(HipReedSolomonCode(K, P, device=NONE), bad, pats)
        _heal_erased_cases[L] = (bad, pats, after, reps)
    return _heal_erased_cases[L]


@pytest.mark.parametrize("L", LENGTHS)
def test_heal_erased_rows_equals_heal_erased_stripes(cuda, L):
    torch = cuda
    bad, pats, after, reps = heal_erased_case(L)
    code = HipReedSolomonCode(K, P, device=0)
    st = on_device(torch, bad)
    rep_stripes = device.heal_erased_stripes(code, st, pats)
    kernel = code.lastKernel()
    wide, views = row_views(torch, bad)
    rep_rows = device.heal_erased_rows(code, views, H.erased_array(pats))
    assert code.lastKernel() == kernel
    torch.cuda.synchronize()
    assert torch.equal(wide[:, :, :L], st) and torch.equal(rep_rows, rep_stripes)
    assert (wide[:, :, L:] == 0xC3).all()  # nothing past the views
    assert (st.cpu().numpy() == after).all() and u32(rep_rows).tolist() == reps.tolist()
    assert reps[:, device.SCRUB_PATCHED].sum() > 0


_repair_cases = {}


def repair_case(L, join):
    """(stripes, stored, reference by hrs_repair_checked_host stripe by
    stripe): a repaired stripe, a clean one, a restamped one."""
    if (L, join) not in _repair_cases:
        stripes, stored = R.mix(K, P, L, S, {0, 2}, seed=7)
        code = HipReedSolomonCode(K, P, device=NONE)
        out = np.array(stripes)
        verdicts, erased, reports, crcs = [], [], [], []
        for s in range(S):
            rows = [np.ascontiguousarray(out[s, l]) for l in range(N)]
            v, e, r, c = device.repair_checked_host(code, rows, stored[s], join)
            out[s] = np.stack(rows)
            verdicts.append(v), erased.append(e.tolist()), reports.append(r.tolist()), crcs.append(c.tolist())
        _repair_cases[(L, join)] = (stripes, stored, (out, verdicts, erased, reports, crcs))
    return _repair_cases[(L, join)]


@pytest.mark.parametrize("join", [False, True])
@pytest.mark.parametrize("L", LENGTHS)
def test_repair_checked_rows_equals_repair_checked_stripes(cuda, L, join):
    torch = cuda
    stripes, stored, (out, verdicts, erased, reports, crcs) = repair_case(L, join)
    assert verdicts == [R.REPAIRED, R.CLEAN, R.RESTAMP]
    sdev = on_device(torch, stored.view(np.int32))
    code = HipReedSolomonCode(K, P, device=0)
    st = on_device(torch, stripes)
    by_stripes = device.repair_checked_stripes(code, st, sdev, join_syndromes=join)
    wide, views = row_views(torch, stripes)
    by_rows = device.repair_checked_rows(code, views, sdev, join_syndromes=join)
    torch.cuda.synchronize()
    assert torch.equal(wide[:, :, :L], st) and (wide[:, :, L:] == 0xC3).all()
    for a, b in zip(by_rows, by_stripes):  # verdicts, erased lists, reports, CRCs
        assert torch.equal(a, b)
    gv, ge, gr, gc = by_rows
    assert (st.cpu().numpy() == out).all()
    assert u32(gv).tolist() == verdicts and ge.cpu().numpy().tolist() == erased
    assert u32(gr).tolist() == reports and u32(gc).tolist() == crcs


# --------------------------------------------------------------- empty calls

def not_read(code, erased):
    to_read = set(code.locationsToReadForDecode(erased))
    return [loc for loc in range(N) if loc not in to_read]


def empty_crc_calls(torch, crc_kw):
    """Every device CRC wrapper over [2, n, 0] cells: name -> (call, width)."""
    s = 2
    st = empty_cells(torch, N, s)
    out = empty_cells(torch, E, s)
    views = [st[:, l] for l in range(N)]
    lists = [[2], []]
    return {
        "encode_stripes_crc": (lambda c: device.encode_stripes_crc(c, st, **crc_kw), N),
        "decode_stripes_crc": (lambda c: device.decode_stripes_crc(c, st, [0, 5], not_read(c, [0, 5]), out,
                                                                   **crc_kw), E),
        "crc32_rows": (lambda c: device.crc32_rows(c, views, **crc_kw), N),
        "decode_batch_crc": (lambda c: device.decode_batch_crc(c, st, ERASED_SE[:s], out, **crc_kw), E),
        "scrub_stripes_crc": (lambda c: device.scrub_stripes_crc(c, st, **crc_kw)[1], N),
        "scrub_rows_crc": (lambda c: device.scrub_rows_crc(c, views, **crc_kw)[1], N),
        "heal_stripes_crc": (lambda c: device.heal_stripes_crc(c, st, **crc_kw)[1], N),
        "heal_rows_crc": (lambda c: device.heal_rows_crc(c, views, **crc_kw)[1], N),
        "heal_erased_stripes_crc": (lambda c: device.heal_erased_stripes_crc(c, st, lists, **crc_kw)[1], N),
        "heal_erased_rows_crc": (lambda c: device.heal_erased_rows_crc(c, views, lists, **crc_kw)[1], N),
    }


@pytest.mark.parametrize("name", ["encode_stripes_crc", "decode_stripes_crc", "crc32_rows", "decode_batch_crc",
                                  "scrub_stripes_crc", "scrub_rows_crc", "heal_stripes_crc", "heal_rows_crc",
                                  "heal_erased_stripes_crc", "heal_erased_rows_crc"])
def test_crcs_of_empty_cells_continue_over_no_bytes(cuda, name):
    """[2, n, 0]: zeros without crc_in, crc_in's values with it. torch gives a
    tensor without elements a null data_ptr(), which the library's scrub, heal
    and decode entry points refuse as a NULL row (hrs_crc32_dev and
    hrs_encode_crc_dev let it pass when the length is 0), so for the other
    eight the wrappers answer such a call themselves."""
    torch = cuda
    code = HipReedSolomonCode(K, P, device=0)
    call, width = empty_crc_calls(torch, {})[name]
    got = call(code)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, width)
    assert not got.cpu().numpy().any()
    start = np.random.default_rng(width).integers(1, 1 << 32, (2, width), dtype=np.uint32)
    cin = on_device(torch, start.view(np.int32))
    call, _ = empty_crc_calls(torch, dict(crc_in=cin))[name]
    got = call(code)
    assert got is not cin and u32(got).tolist() == start.tolist() and u32(cin).tolist() == start.tolist()


def test_empty_cells_are_clean_and_decode_to_nothing(cuda):
    """The calls without CRCs and the reports of [2, n, 0]: every stripe clean
    (no bad column, first bad column SCRUB_NONE), nothing decoded, no error."""
    torch = cuda
    code = HipReedSolomonCode(K, P, device=0)
    st, out = empty_cells(torch, N, 2), empty_cells(torch, E, 2)
    views = [st[:, l] for l in range(N)]
    clean = np.zeros((2, 4 + N), np.uint32)
    clean[:, device.SCRUB_FIRST_BAD] = device.SCRUB_NONE
    stored = torch.zeros((2, N), dtype=torch.int32, device="cuda:0")
    checked = device.repair_checked_rows(code, views, stored)
    for reports in (device.scrub_stripes(code, st), device.scrub_rows(code, views), device.heal_stripes(code, st),
                    device.heal_erased_rows(code, views, [[2], []]), device.scrub_stripes_crc(code, st)[0],
                    device.heal_erased_stripes_crc(code, st, [[2], []])[0], checked[2]):
        assert u32(reports).tolist() == clean.tolist()
    assert not u32(checked[0]).any() and (checked[1] == -1).all() and not u32(checked[3]).any()
    assert device.decode_stripes(code, st, [0, 5], not_read(code, [0, 5]), out) is None
    assert device.decode_batch(code, st, ERASED_SE[:2], out) is None
    with pytest.raises(ValueError):  # the wrappers' own rules still hold
        device.heal_erased_stripes(code, st, [[2]])
    torch.cuda.synchronize()
    assert code.lastKernel() == ""
