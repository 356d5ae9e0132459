"""Scrub and heal kernels (hrs_scrub.hip) with many dirty windows per wave,
under every window order, on a capped grid, at scale and for every parity
size. The other scrub / heal suites run at most 6 window tasks per launch, so
there no wave runs a second task: the flush of the per-wave LDS histogram to a
window's stripe, and its re-arming by the exchange, never met a second dirty
window, let alone one of another stripe.

Every expectation comes from the oracle (encode_bulk, compute_error_locations):
stripes of codeword columns by construction, planted columns one by one under
the heal rule (resolved: the oracle's post-call data; unresolved: the bytes as
they were). Nothing comes from hrs_heal_host or from a kernel. Every
comparison is bit-exact over every stripe and every byte.

The inputs only test the hand-over if some wave really runs several dirty
windows, so the window -> wave assignment of wave_tasks (hrs_device.hpp) is
restated here and three properties are asserted of it, each for some wave:
  run       at least 3 dirty windows of at least 2 stripes;
  handover  two consecutive dirty windows of different stripes;
  gap       a dirty - clean - dirty run.
What a schedule can show depends on the longest run of windows it gives a
wave. RS(10,4) x 40 stripes is 120 windows on a grid of 30 blocks (120 waves):
under HRS_TASK_ORDER 1 and 0 every wave runs one window and none of the three
can hold; under order 2 the waves of the working blocks run two, which allows
the handover alone. Those three launches check the orders' coverage (every
window once, reports and bytes exact). Every other case here gives some wave
3 to 30 windows, and all three properties are required of it."""
import os
import random

import numpy as np
import pytest

from lambdafs_amd import HipReedSolomonCode, _lib, device
from oracle import rs_oracle as C
from test_gpu_heal import _device_view, _guarded, _guards_intact, _outside_unchanged, _search
from test_gpu_scrub import NONE, _u32
from test_heal_host import heal_expected

WINDOW = 2048    # kWindowBytes
WPB = 4          # waves per 256-thread block (kWavesPerBlock)
FILL = 0x5A5A5A5A
SPARE = 3        # report_stride = 4 + n + SPARE

# case -> (k, p, L, seed); S is _stripes_of(case, cus). The seeds are picked so
# that the schedule properties hold (test_inputs_and_schedules asserts them).
CASES = {
    "orders": (10, 4, 3 * WINDOW + 33, 3),        # a and b
    "scale": (6, 3, 9 * WINDOW + 96, 1),          # c
    "p5": (9, 5, 2 * WINDOW + 17, 1),             # d: every P, n = 8 and 17 around the 8-row load group
    "p6": (12, 6, 2 * WINDOW + 17, 1),
    "p7": (40, 7, 2 * WINDOW + 17, 1),
    "n8": (6, 2, 2 * WINDOW + 17, 1),
    "n17": (12, 5, 2 * WINDOW + 17, 2),
}
EVERY_P = ["p5", "p6", "p7", "n8", "n17"]
FULL_ORACLE = set(EVERY_P)  # every column of these goes through the oracle

# (case, HRS_TASK_ORDER, HRS_ZC_BLOCKS or None, longest run of windows on one wave with 256 CUs)
SCHEDULES = [("orders", 1, None, 1), ("orders", 0, None, 1), ("orders", 2, None, 2), ("orders", 32, None, 30),
             ("orders", 1, 1, 30), ("orders", 0, 1, 30), ("orders", 1, 3, 10), ("orders", 0, 3, 10),
             ("scale", 1, None, 3), ("scale", 0, None, 3)] + [(c, 32, None, 6) for c in EVERY_P]


def _stripes_of(case, cus):
    if case == "orders":
        return 40
    if case == "scale":  # window tasks >= 2.5 x resident waves (2 blocks per CU)
        nwin = CASES[case][2] // WINDOW
        return -(-(5 * 2 * cus * WPB) // (2 * nwin))
    return 12


# --------------------------------------------------------------- inputs

_cache = {}


def _error_counts(p):
    return sorted({1, p // 2, p // 2 + 1} - {0})


def _plant(k, p, clean, rnd, errors):
    """A corruption of the codeword column `clean` with `errors` wrong symbols.
    p / 2 + 1 errors: searched (as test_gpu_heal._search does) for a column
    the oracle calls unresolved after writing into it; p = 2 has none (one it
    leaves alone), for p = 1 every nonzero syndrome is unresolved."""
    n = k + p
    if errors == p // 2 + 1:
        if p == 1:
            return _search(k, p, clean, rnd, errors, lambda ok, found, after, t: not ok)
        if p == 2:
            return _search(k, p, clean, rnd, errors, lambda ok, found, after, t: not ok and after == t)
        return _search(k, p, clean, rnd, errors, lambda ok, found, after, t: not ok and after != t)
    trial = list(clean)
    for l in rnd.sample(range(n), errors):
        trial[l] ^= rnd.randrange(1, 256)
    return trial


def _column_report(k, p, rep, c, column):
    """The oracle on one column into the report `rep`; (ok, found, after) or
    None for a codeword."""
    ok, found, after = C.compute_error_locations(k, p, column)
    if ok and not found:
        return None
    rep[0] += 1
    rep[2] = min(int(rep[2]), c)
    if not ok:
        rep[1] += 1
    else:
        for l in found:
            rep[4 + l] += 1
    return ok, found, after


def _inputs(case, cus=256):
    """(host[S, n, L], healed[S, n, L], reports[S, 4 + n]) of a case, built once
    and read-only; _meta(case, cus) has the rest. Stripes by kind, shuffled by
    the seed:
      clean  stripe 0, the last one, and a quarter of all in total;
      rows   two stripes with one whole row replaced (every lane of every
             window takes the slow path), expected by heal_expected;
      dirty  the rest (over half): columns with 1, p / 2 and p / 2 + 1 errors
             in 2 or more windows (their first and last byte included) and in
             the row tail (its last byte included); for p >= 7 one 2-error
             column that the oracle resolves with more than 2 locations."""
    key = (case, cus)
    if key in _cache:
        return _cache[key][:3]
    k, p, L, seed = CASES[case]
    S = _stripes_of(case, cus)
    n, nwin = k + p, L // WINDOW
    rng = np.random.default_rng([seed, k, p, S, L])
    rnd = random.Random(1000003 * seed + 7919 * k + 31 * p + S + L)
    host = np.empty((S, n, L), dtype=np.uint8)
    host[:, p:] = rng.integers(0, 256, (S, k, L), dtype=np.uint8)
    for s in range(S):
        host[s, :p] = np.stack(C.encode_bulk(k, p, [host[s, p + c] for c in range(k)]))
    inner = list(range(1, S - 1))
    rnd.shuffle(inner)
    nclean = -(-S // 4) - 2
    kind = ["dirty"] * S
    for s in [0, S - 1] + inner[:nclean]:
        kind[s] = "clean"
    for s in inner[nclean:nclean + 2]:
        kind[s] = "rows"
    healed = host.copy()
    rep = np.zeros((S, 4 + n), dtype=np.uint32)
    rep2 = np.zeros((S, 4 + n), dtype=np.uint32)  # of the healed stripes: what a second heal reports
    rep[:, 2] = rep2[:, 2] = NONE
    classes = {"patched": 0, "unresolved_written": 0, "unresolved_untouched": 0, "spurious": 0}
    dirty = [set() for _ in range(S)]  # the windows of each stripe with a nonzero syndrome
    counts = _error_counts(p)
    spurious_left = 1 if p >= 7 else 0
    for s in range(S):
        if kind[s] == "rows":
            host[s, rnd.randrange(n)] = rng.integers(0, 256, L, dtype=np.uint8)
            healed[s], rep[s] = heal_expected(k, p, host[s])
            rep2[s] = heal_expected(k, p, healed[s])[1]
            dirty[s] = set(range(nwin))
            continue
        if kind[s] != "dirty":
            continue
        wins = sorted(rnd.sample(range(nwin), rnd.randint(2, nwin)))
        cols = []
        for i, w in enumerate(wins):
            inside = set(rnd.sample(range(WINDOW), rnd.randint(1, 3)))
            if i == 0:
                inside.add(0)
            if i == len(wins) - 1:
                inside.add(WINDOW - 1)
            cols += [w * WINDOW + c for c in sorted(inside)]
        tail = range(nwin * WINDOW, L)
        cols += sorted(set(rnd.sample(tail, min(2, len(tail)))) | {L - 1})
        dirty[s] = set(wins)
        turn = rnd.randrange(len(counts))
        plan = [(c, counts[(turn + i) % len(counts)]) for i, c in enumerate(cols)]
        if spurious_left:
            spurious_left = 0
            c = next(c for c in range(wins[0] * WINDOW + 1, L) if c not in cols)
            plan.append((c, "spurious"))
        for c, errors in sorted(plan):
            clean = host[s, :, c].tolist()
            if errors == "spurious":
                column = _search(k, p, clean, rnd, 2, lambda ok, found, after, t: ok and len(found) > 2)
                assert C.compute_error_locations(k, p, list(column))[2] == clean
                classes["spurious"] += 1
            else:
                column = _plant(k, p, clean, rnd, errors)
            host[s, :, c] = column
            got = _column_report(k, p, rep[s], c, list(column))
            assert got is not None, "a planted column is no codeword"
            ok, found, after = got
            if ok:
                healed[s, :, c] = after
                classes["patched"] += after != column
            else:
                healed[s, :, c] = column
                classes["unresolved_written" if after != column else "unresolved_untouched"] += 1
            _column_report(k, p, rep2[s], c, healed[s, :, c].tolist())
        rep[s, 3] = np.count_nonzero(healed[s] != host[s])
    if case in FULL_ORACLE:  # every column through the oracle: the same stripes and reports
        for s in range(S):
            want, want_rep = heal_expected(k, p, host[s])
            assert (want == healed[s]).all() and want_rep.tolist() == rep[s].tolist(), (case, s)
    for a in (host, healed, rep, rep2):
        a.setflags(write=False)
    _cache[key] = (host, healed, rep, dict(kind=kind, dirty=dirty, classes=classes, rep2=rep2, nwin=nwin))
    return _cache[key][:3]


def _meta(case, cus=256):
    _inputs(case, cus)
    return _cache[(case, cus)][3]


# ------------------------------------------------------------- schedule

def _grid(ntasks, cus, cap=None):
    """stream_grid (hrs_launch.hpp): min(ceil(tasks / 4), 2 x CUs, cap)."""
    g = min(-(-ntasks // WPB), 2 * cus)
    return max(1, min(g, cap) if cap else g)


def _wave_tasks(ntasks, order, grid):
    """wave_tasks (hrs_device.hpp) restated: the tasks of every wave of the
    grid, in the order the wave runs them."""
    waves = []
    for b in range(grid):
        for w in range(WPB):
            if order >= 1:
                t0, end, jump, chunk = b * order * WPB + w, ntasks, grid * order * WPB, order
            else:
                per = -(-ntasks // grid)
                t0, end, jump, chunk = per * b + w, min(per * b + per, ntasks), 0, 0xFFFFFFFF
            tasks, j = [], 0
            while True:
                q = j // chunk
                t = t0 + q * jump + (j - q * chunk) * WPB
                if t >= end:
                    break
                tasks.append(t)
                j += 1
            waves.append(tasks)
    return waves


def _schedule_facts(case, order, cap, cus):
    """(longest run of windows on a wave, most dirty windows on a wave, the
    properties some wave shows) for the case's window launch."""
    meta = _meta(case, cus)
    nwin = meta["nwin"]
    ntasks = _stripes_of(case, cus) * nwin
    waves = _wave_tasks(ntasks, order, _grid(ntasks, cus, cap))
    assert sorted(t for w in waves for t in w) == list(range(ntasks))  # every window once
    shown, most = set(), 0
    for tasks in waves:
        seq = [(t % nwin in meta["dirty"][t // nwin], t // nwin) for t in tasks]
        bad = [s for d, s in seq if d]
        most = max(most, len(bad))
        if len(bad) >= 3 and len(set(bad)) >= 2:
            shown.add("run")
        for (d0, s0), (d1, s1) in zip(seq, seq[1:]):
            if d0 and d1 and s0 != s1:
                shown.add("handover")
        for (d0, _), (d1, _), (d2, _) in zip(seq, seq[1:], seq[2:]):
            if d0 and not d1 and d2:
                shown.add("gap")
    return max(len(w) for w in waves), most, shown


def _required(longest):
    """What a schedule can show (module docstring): all three properties from
    3 windows per wave on, the handover alone with 2, nothing with 1."""
    return {"run", "handover", "gap"} if longest >= 3 else {"handover"} if longest == 2 else set()


def _check_schedule(case, order, cap, cus, longest=None):
    got_longest, most, shown = _schedule_facts(case, order, cap, cus)
    print(f"{case} order={order} cap={cap} cus={cus}: longest run {got_longest} windows, "
          f"most dirty windows on one wave {most}, shows {sorted(shown)}")
    if longest is not None:
        assert got_longest == longest
    assert _required(got_longest) <= shown, (case, order, cap, sorted(shown))
    return most


@pytest.mark.parametrize("case", list(CASES))
def test_inputs_hold_every_outcome(case):
    """The conditions on the inputs that make the GPU cases mean something (no GPU call)."""
    k, p, L, _ = CASES[case]
    host, healed, rep = _inputs(case)
    meta = _meta(case)
    S, kind, rep2 = host.shape[0], meta["kind"], meta["rep2"]
    print(f"{case}: RS({k},{p}) S={S} L={L} kinds "
          f"{ {x: kind.count(x) for x in ('clean', 'dirty', 'rows')} } classes {meta['classes']}")
    assert kind[0] == kind[-1] == "clean" and kind.count("clean") * 4 >= S
    assert kind.count("dirty") * 2 >= S and kind.count("rows") == 2
    for s in range(S):
        if kind[s] == "clean":
            assert rep[s].tolist() == [0, 0, NONE, 0] + [0] * (k + p) and (host[s] == healed[s]).all()
            par = C.encode_bulk(k, p, [host[s, p + c] for c in range(k)])
            assert (np.stack(par) == host[s, :p]).all()
        elif kind[s] == "dirty":
            assert len(meta["dirty"][s]) >= 2 and rep[s, 0] >= len(meta["dirty"][s]) + 1  # windows + tail
            assert rep[s, 2] % WINDOW == 0 and rep[s, 2] // WINDOW == min(meta["dirty"][s])
            assert rep[s, 1] >= 1  # its p / 2 + 1 column(s)
        else:
            assert len(meta["dirty"][s]) == meta["nwin"] and rep[s, 0] >= L - L // 64
    # every outcome class
    cl = meta["classes"]
    assert cl["patched"] >= 1
    assert cl["unresolved_written" if p > 2 else "unresolved_untouched"] >= 1
    assert (cl["spurious"] == 1) == (p >= 7)
    if p >= 7:
        assert int(rep[:, 4:].sum()) > int(rep[:, 3].sum())  # locations blamed > bytes changed
    # the healed stripes: only the unresolved columns are left, nothing to store
    assert rep2[:, 0].tolist() == rep2[:, 1].tolist() == rep[:, 1].tolist()
    assert not rep2[:, 3].any() and not rep2[:, 4:].any() and rep[:, 1].any()
    assert rep[:, 3].tolist() == [int(np.count_nonzero(host[s] != healed[s])) for s in range(S)]


@pytest.mark.parametrize("case,order,cap,longest", SCHEDULES)
def test_schedules_run_dirty_windows_back_to_back(case, order, cap, longest):
    """Under the grid of a 256-CU device, every launch of the GPU cases gives
    some wave what its schedule can show of: 3 or more dirty windows of 2 or
    more stripes, two consecutive dirty windows of different stripes, a
    dirty - clean - dirty run (no GPU call)."""
    _check_schedule(case, order, cap, 256, longest)
    if case == "orders" and cap:  # the capped byte-granular launch takes a second grid-stride step
        L, S = CASES[case][2], _stripes_of(case, 256)
        assert S * (L % WINDOW) == 1320 > cap * 256


# ------------------------------------------------------------ GPU cases

def _same_bytes(got, want, what):
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    s, l, c = (int(x) for x in bad[0])
    pytest.fail(f"{what}: {len(bad)} bytes differ, first at stripe {s} row {l} column {c}: "
                f"got {int(got[s, l, c]):#04x}, want {int(want[s, l, c]):#04x}")


def _same_reports(got, want, what):
    if np.array_equal(got, want):
        return
    rows = np.flatnonzero((got != want).any(axis=1))
    lines = [f"stripe {int(s)}: got {got[s].tolist()} want {want[s].tolist()}" for s in rows[:4]]
    pytest.fail(f"{what}: the reports of {len(rows)} stripes differ\n" + "\n".join(lines))


def _cus(torch):
    assert "HRS_BLOCKS_PER_CU" not in os.environ, \
        "HRS_BLOCKS_PER_CU changes the grid these cases' wave schedules are checked for: unset it"
    return torch.cuda.get_device_properties(0).multi_processor_count


def _strided(raw, n):
    """Reports [S, 4 + n] out of a strided buffer whose spare words must survive."""
    assert (raw[:, 4 + n:] == FILL).all(), "words past 4 + n of a report were written"
    return raw[:, :4 + n]


def _run_device(torch, case, cus, mode):
    """Scrub, heal and a second heal of the case's stripes through
    hrs_scrub_dev / hrs_heal_dev, everything compared with the oracle's."""
    k, p, L, _ = CASES[case]
    n = k + p
    host, healed, want = _inputs(case, cus)
    rep2 = _meta(case, cus)["rep2"]
    S = host.shape[0]
    code = HipReedSolomonCode(k, p, device=0)
    code.setKernelMode(mode)
    big, view = _device_view(torch, host)
    before = big.clone()
    rows = _lib.ptr_array([view.data_ptr() + l * view.stride(1) for l in range(n)])
    name = "kernel" if mode == 0 else "bytewise_kernel"

    def call(fn):
        rep = torch.full((S, 4 + n + SPARE), FILL, dtype=torch.int32, device="cuda:0")
        code._check(fn(code._handle(), rows, view.stride(0), L, S, rep.data_ptr(), 4 + n + SPARE,
                       torch.cuda.current_stream().cuda_stream))
        return _strided(_u32(rep), n)

    scrub_want = np.array(want)
    scrub_want[:, 3] = 0
    got = call(_lib.lib().hrs_scrub_dev)
    assert code.lastKernel() == f"scrub_{name}<{p}>"
    _same_reports(got, scrub_want, "scrub")
    assert torch.equal(big, before), "the scrub wrote into the stripes"
    got = call(_lib.lib().hrs_heal_dev)
    assert code.lastKernel() == f"heal_{name}<{p}>"
    _same_bytes(view.cpu().numpy(), healed, "heal")
    assert _outside_unchanged(big, before, host.shape)
    _same_reports(got, want, "heal")
    after_first = big.clone()
    got = call(_lib.lib().hrs_heal_dev)
    assert torch.equal(big, after_first), "the second heal stored something"
    _same_reports(got, rep2, "second heal")


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 0, 2, 32])
def test_window_orders(cuda, monkeypatch, order):
    """a. RS(10,4), 40 stripes of 3 windows + 33 bytes, device entry: under
    order 32 one block runs all 120 windows, 30 per wave; under order 2 each
    wave of a working block runs 2; under 1 and 0 each wave runs one."""
    cus = _cus(cuda)
    _check_schedule("orders", order, None, cus)
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    _run_device(cuda, "orders", cus, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("cap", [1, 3])
def test_capped_grid_pinned_host_batch(cuda, monkeypatch, cap, order):
    """b. The same stripes in pinned host memory through hrs_scrub_batch_host
    and hrs_heal_batch_host, the grid capped at 1 block (4 waves x 30 windows;
    256 threads stride over the 1,320 tail columns) and at 3."""
    torch = cuda
    case = "orders"
    cus = _cus(torch)
    _check_schedule(case, order, cap, cus)
    monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    monkeypatch.setenv("HRS_ZC_BLOCKS", str(cap))
    k, p, L, _ = CASES[case]
    n = k + p
    host, healed, want = _inputs(case, cus)
    rep2 = _meta(case, cus)["rep2"]
    S = host.shape[0]
    code = HipReedSolomonCode(k, p, device=0)
    big, view, arg = _guarded(host, True, torch)
    before = big.copy()

    def call(fn):
        rep = np.full((S, 4 + n + SPARE), FILL, dtype=np.uint32)
        code._check(fn(code._handle(), arg.data_ptr(), arg.stride(1), arg.stride(0), L, S, rep.ctypes.data,
                       4 + n + SPARE))
        assert code.lastHostPath() == "pinned"
        return _strided(rep, n)

    scrub_want = np.array(want)
    scrub_want[:, 3] = 0
    _same_reports(device.scrub_batch_host(code, arg), scrub_want, "scrub_batch_host")
    assert code.lastHostPath() == "pinned" and code.lastKernel() == f"scrub_kernel<{p}>"
    _same_reports(call(_lib.lib().hrs_scrub_batch_host), scrub_want, "scrub, strided reports")
    assert code.lastKernel() == f"scrub_kernel<{p}>"
    assert (big == before).all(), "the scrub wrote into the stripes"
    got = call(_lib.lib().hrs_heal_batch_host)
    assert code.lastKernel() == f"heal_kernel<{p}>"
    _same_bytes(view, healed, "heal")
    assert _guards_intact(big, n, L)
    _same_reports(got, want, "heal")
    after_first = big.copy()
    got = device.heal_batch_host(code, arg)
    assert code.lastHostPath() == "pinned"
    assert (big == after_first).all(), "the second heal stored something"
    _same_reports(got, rep2, "second heal")
    _same_reports(call(_lib.lib().hrs_heal_batch_host), rep2, "third heal, strided reports")
    assert (big == after_first).all()


@pytest.mark.gpu
@pytest.mark.parametrize("order,mode", [(1, 0), (0, 0), (None, 2)], ids=["grid_stride", "block_range", "bytewise"])
def test_at_scale_default_grid(cuda, monkeypatch, order, mode):
    """c. RS(6,3), 9 windows + 96 bytes, as many stripes as give the default
    grid 2.5 window tasks per resident wave (569 on 256 CUs): waves run 3
    windows of 3 stripes. Kernel mode 2: every thread of the byte-granular
    kernels takes several of the S x L columns."""
    cus = _cus(cuda)
    S, nwin = _stripes_of("scale", cus), CASES["scale"][2] // WINDOW
    assert 2 * S * nwin >= 5 * 2 * cus * WPB
    if order is None:
        monkeypatch.delenv("HRS_TASK_ORDER", raising=False)
    else:
        _check_schedule("scale", order, None, cus)
        monkeypatch.setenv("HRS_TASK_ORDER", str(order))
    _run_device(cuda, "scale", cus, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("case", EVERY_P)
def test_every_parity_size(cuda, monkeypatch, case, mode):
    """d. P = 5, 6, 7 and n = 8, 17 (either side of the 8-row load group), 12
    stripes of 2 windows + 17 bytes, every column through the oracle; order 32
    puts the 24 windows on one block, 6 per wave."""
    cus = _cus(cuda)
    _check_schedule(case, 32, None, cus)
    monkeypatch.setenv("HRS_TASK_ORDER", "32")
    _run_device(cuda, case, cus, mode)
