"""Tiled window sweeps (tp_batch_window_sweep_tiled / Batch.window_sweep_tiled, k > 143): L nested window lengths per window
from one pass over the rows of the longest, on the large-k tiled pipeline.  Checked against the oracle called once per length on
the suffix rows (the table of tests/_window_sweep_tiled_cases.py, vouched for on the CPU by
tests/test_host_window_sweep_tiled_cases.py); bit for bit against itself across W, the slot, P, the sub-ranges, the arena's size
and a zero delta; to rounding across lists of lengths and against the tiled prior sweep and the run on the whole window; for
isolation of a length from older rows; for a rank-deficient Jeffreys length; the refusals; and the product path
(calculate_weights_for_windows with WINDOW_SWEEP_TILED).  Every test calls the new entry point.  -m gpu."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from incorporating_different_sources_amd import _native, synthetic

import _window_sweep_tiled_cases as cases
from _window_sweep_tiled_cases import GAMMA, TOL

pytestmark = pytest.mark.gpu

FLAGS = {0: 0, 1: _native.FLAG_CENTER_BY_ROWS, 2: _native.FLAG_NO_CENTER}      # the case table's flag -> TP_FLAG_*


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


def assert_close(x, ref, tol=TOL, what=""):
    bound = tol * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(x - ref).max())
    print(f"{what}: max|sweep - ref| = {err:.3e} = {err / bound:.3e} of the bound {bound:.3e} (|ref|.max() = {np.abs(ref).max():.3e})")
    assert np.isfinite(x).all()
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"
    return err / bound


def upload(dev, pr, flags=0):
    inp, conj = pr["inp"], pr["strategy"] == "conjugate"
    b = dev.batch(pr["strategy"], pr["k"], inp["N"], inp["n_r"], GAMMA, cases.W, inp["m"] if conj else 0, flags)
    ukw = pr["upload"] if conj else {key: val for key, val in pr["upload"].items() if not key.startswith("hf_") and key not in ("w0", "n0")}
    b.upload(pr["panel"], **ukw)
    return b


# ---- 1. against the oracle --------------------------------------------------------------------------------------------
CONJ = list(cases.problems("conjugate"))
JEFF = [(pr, f) for pr in cases.problems("jeffreys") for f in cases.jeffreys_flags(pr["k"])]


@pytest.mark.parametrize("pr", CONJ, ids=[pr["id"] for pr in CONJ])
def test_window_sweep_tiled_matches_oracle_conjugate(dev, pr):
    L, k = len(pr["N"]), pr["k"]
    b = upload(dev, pr)
    wts, status, aux = b.window_sweep_tiled(pr["N"], pr["rows"], pr["n0"], pr["w0"], delta=pr["delta"])
    b.close()
    assert wts.shape == (cases.W, cases.P, L, k) and status.shape == (cases.W, cases.P, L) and aux.shape == (cases.W, cases.P, L, 8)
    ref, rstat, raux = cases.reference(pr)
    worst = max(assert_close(wts[:, :, l], ref[:, :, l], what=f"{pr['id']} rows={pr['rows'][:, l].tolist()}") for l in range(L))
    print(f"{pr['id']}: worst |sweep - oracle| = {worst:.3e} of the bound; aux {cases.aux_ratio(aux[..., :6], raux[..., :6]):.3e} of its tolerance")
    assert np.array_equal(status, rstat) and (status == _native.STATUS_OK).all(), status
    np.testing.assert_allclose(aux[..., :6], raux[..., :6], **cases.AUX_TOL)
    assert np.array_equal(aux[..., 0], pr["n0"]) and not aux[..., 6:].any()


@pytest.mark.parametrize("pr,flag", JEFF, ids=[f"{pr['id']}-flag{f}" for pr, f in JEFF])
def test_window_sweep_tiled_matches_oracle_jeffreys(dev, pr, flag):
    L, k = len(pr["N"]), pr["k"]
    b = upload(dev, pr, FLAGS[flag])
    wts, status, aux = b.window_sweep_tiled(pr["N"], pr["rows"], delta=pr["delta"])
    b.close()
    assert wts.shape == (cases.W, 1, L, k) and status.shape == (cases.W, 1, L) and aux.shape == (cases.W, 1, L, 8)
    ref, rstat, _ = cases.reference(pr, flag)
    worst = max(assert_close(wts[:, :, l], ref[:, :, l], what=f"{pr['id']} flag={flag} rows={pr['rows'][:, l].tolist()}") for l in range(L))
    print(f"{pr['id']} flag={flag}: worst |sweep - oracle| = {worst:.3e} of the bound")
    assert np.array_equal(status, rstat) and (status == _native.STATUS_OK).all(), status
    # aux: what tp_batch_download gives a Jeffreys window - zeros except q1 = t'M^-1 t = gamma t'(the weights); the oracle has
    # no q1 for Jeffreys, gamma t'(its weights) stands in (the CPU test holds the stand-in to a quarter of the tolerance)
    assert not aux[..., [0, 1, 2, 3, 5, 6, 7]].any()
    for w in range(cases.W):
        for l in range(L):
            X, _ = cases.window_rows(pr, w, l)
            q1 = GAMMA * X.sum(axis=0) @ ref[w, 0, l]
            np.testing.assert_allclose(aux[w, 0, l, 4], q1, **cases.AUX_TOL)


# ---- 2. bit for bit, and to rounding ----------------------------------------------------------------------------------
IND_K, IND_N, IND_W, IND_P = 260, 320, 2, 2
IND_ROWS = {"conjugate": [5, 120, 299, 319], "jeffreys": [280, 290, 299, 319]}


def _ind_problem(strategy):
    inp = synthetic.make_kernel_inputs(IND_K, IND_N, IND_W, seed=971000, hf_days=cases.hf_days(IND_K))
    rng = np.random.default_rng(971000)
    rows0 = np.asarray(IND_ROWS[strategy], dtype=np.int32)
    Nl = rows0 + 1
    rows = np.stack([rows0 - w for w in range(IND_W)]).astype(np.int32)
    L = len(Nl)
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(IND_W, IND_P, L))
    w0 = rng.dirichlet(np.ones(IND_K), size=(IND_W, IND_P))
    delta = rng.normal(0.0, 1e-6, size=(IND_W, L, inp["n_r"]))
    return inp, Nl, rows, n0, w0, delta


def _ind_sweep(dev, strategy, windows, priors, lengths=None, chunk=0, arena_mib=0, delta="own"):
    inp, Nl, rows, n0, w0, dl = _ind_problem(strategy)
    conj = strategy == "conjugate"
    ws = np.asarray(windows)
    ls = np.arange(len(Nl)) if lengths is None else np.asarray(lengths)
    d = None if delta is None else (np.zeros_like(dl) if delta == "zero" else dl)[np.ix_(ws, ls)]
    dev.set_option("sweep_chunk_windows", chunk)
    dev.set_option("tiled_arena_mib", arena_mib)
    try:
        b = dev.batch(strategy, IND_K, IND_N, inp["n_r"], GAMMA, len(ws), inp["m"] if conj else 0)
        if conj:
            b.upload(inp["panel"], start=inp["start"][ws], hf_start=inp["hf_start"][ws], w0=inp["w0"][ws], n0=inp["n0"][ws],
                     hf_panel=inp["hf_panel"])
        else:
            b.upload(inp["panel"], start=inp["start"][ws])
        pri = (n0[np.ix_(ws, priors, ls)], w0[np.ix_(ws, priors)]) if conj else ()
        out = b.window_sweep_tiled(Nl[ls], rows[np.ix_(ws, ls)], *pri, delta=d)
        b.close()
        return out
    finally:
        dev.set_option("sweep_chunk_windows", 0)
        dev.set_option("tiled_arena_mib", 0)


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_window_sweep_tiled_is_bitwise_independent_of_W_slot_P_chunking_and_arena(dev, strategy):
    conj = strategy == "conjugate"
    allp = list(range(IND_P)) if conj else [0]
    full = _ind_sweep(dev, strategy, range(IND_W), allp)
    assert (full[1] == 0).all(), full[1]
    for w in range(IND_W):                                  # W = 1 against 2
        one = _ind_sweep(dev, strategy, [w], allp)
        for a, f in zip(one, full):
            assert np.array_equal(a[0], f[w])
    rev = _ind_sweep(dev, strategy, list(range(IND_W))[::-1], allp)       # every window in the other slot
    for a, f in zip(rev, full):
        assert np.array_equal(a[::-1], f)
    if conj:
        single = _ind_sweep(dev, strategy, range(IND_W), [1])              # P = 1 against 2
        for a, f in zip(single, full):
            assert np.array_equal(a[:, 0], f[:, 1])
        swapped = _ind_sweep(dev, strategy, range(IND_W), allp[::-1])      # every prior in the other slot
        for a, f in zip(swapped, full):
            assert np.array_equal(a[:, ::-1], f)
    cut = _ind_sweep(dev, strategy, range(IND_W), allp, chunk=1)           # sub-ranges of one window against automatic
    for a, f in zip(cut, full):
        assert np.array_equal(a, f)
    # an arena of 1 MiB holds ONE entry at k = 260 (KP = 320: 0.94 MiB of arena, inverse blocks and scratch): the W x P entries of
    # a length go through it one by one
    small = _ind_sweep(dev, strategy, range(IND_W), allp, arena_mib=1)
    for a, f in zip(small, full):
        assert np.array_equal(a, f)


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_an_all_zero_delta_gives_the_bits_of_no_delta(dev, strategy):
    allp = list(range(IND_P)) if strategy == "conjugate" else [0]
    none = _ind_sweep(dev, strategy, range(IND_W), allp, delta=None)
    zero = _ind_sweep(dev, strategy, range(IND_W), allp, delta="zero")
    own = _ind_sweep(dev, strategy, range(IND_W), allp)
    assert (none[1] == 0).all()
    for a, z in zip(none, zero):
        assert np.array_equal(a, z)
    assert not np.array_equal(none[0], own[0])                             # (a delta that is not zero is applied)


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_a_sub_list_of_lengths_agrees_to_rounding(dev, strategy):
    allp = list(range(IND_P)) if strategy == "conjugate" else [0]
    full = _ind_sweep(dev, strategy, range(IND_W), allp)
    some = _ind_sweep(dev, strategy, range(IND_W), allp, lengths=[1, 3])
    assert_close(some[0], full[0][:, :, [1, 3]], what=f"{strategy}: lengths [1, 3] alone vs the list of 4")
    assert np.array_equal(some[1], full[1][:, :, [1, 3]])


def test_whole_window_equals_prior_sweep_tiled_and_run(dev):
    """L = 1 with rows = n_w and N = the batch's N: the tiled prior sweep (conjugate) and tp_batch_run (Jeffreys) on the same batch."""
    k, N, W, P = 260, 320, 2, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=971100, hf_days=cases.hf_days(k))
    n_r = inp["n_r"]
    rng = np.random.default_rng(971100)
    rows = np.full((W, 1), n_r, dtype=np.int32)
    n0 = N * rng.uniform(1.0, 1.6, size=(W, P, 1))
    w0 = np.stack([inp["w0"], np.full((W, k), 1.0 / k)], axis=1)
    b = dev.batch("conjugate", k, N, n_r, GAMMA, W, inp["m"])
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    pw, pstat, paux = b.prior_sweep_tiled(np.ascontiguousarray(n0[:, :, 0]), w0)
    wts, status, aux = b.window_sweep_tiled([N], rows, n0, w0)
    b.close()
    assert (pstat == 0).all() and (status == 0).all()
    assert_close(wts[:, :, 0], pw, what="conjugate, whole window vs prior_sweep_tiled")
    np.testing.assert_allclose(aux[:, :, 0, :6], paux[..., :6], **cases.AUX_TOL)
    for flags in (0, _native.FLAG_CENTER_BY_ROWS, _native.FLAG_NO_CENTER):
        j = dev.batch("jeffreys", k, N, n_r, GAMMA, W, 0, flags)
        j.upload(inp["panel"], start=inp["start"])
        full, fstat, faux = j.run().download()
        wts, status, aux = j.window_sweep_tiled([N], rows)
        j.close()
        assert (fstat == 0).all() and (status == 0).all()
        assert_close(wts[:, 0, 0], full, what=f"jeffreys flags={flags}, whole window vs run")
        np.testing.assert_allclose(aux[:, 0, 0, 4], faux[:, 4], **cases.AUX_TOL)


# ---- 3. isolation -----------------------------------------------------------------------------------------------------
ISO_K, ISO_N, ISO_W = 150, 320, 2
ISO_ROWS = [200, 240, 280, 319]


def _iso_sweep(dev, strategy, panel, row_idx, inp):
    conj = strategy == "conjugate"
    rng = np.random.default_rng(972000)
    Nl = np.asarray(ISO_ROWS, dtype=np.int32) + 1
    rows = np.tile(np.asarray(ISO_ROWS, dtype=np.int32), (ISO_W, 1))
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(ISO_W, 2, len(ISO_ROWS)))
    w0 = rng.dirichlet(np.ones(ISO_K), size=(ISO_W, 2))
    delta = rng.normal(0.0, 1e-6, size=(ISO_W, len(ISO_ROWS), inp["n_r"]))
    b = dev.batch(strategy, ISO_K, ISO_N, inp["n_r"], GAMMA, ISO_W, inp["m"] if conj else 0)
    if conj:
        b.upload(panel, row_idx=row_idx, hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
        out = b.window_sweep_tiled(Nl, rows, n0, w0, delta=delta)
    else:
        b.upload(panel, row_idx=row_idx)
        out = b.window_sweep_tiled(Nl, rows, delta=delta)
    b.close()
    return out


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("damage", [np.nan, 1e6])
def test_a_row_older_than_a_suffix_never_reaches_it(dev, strategy, damage):
    """Window 1 reads a damaged row at position n_r - 260: inside segment 2 (the rows of length 280 that length 240 does not
    have).  Lengths 200 and 240 are bit for bit those of the clean run and TP_STATUS_OK; lengths 280 and 319 are flagged (NaN)
    or changed (outlier)."""
    inp = synthetic.make_kernel_inputs(ISO_K, ISO_N, ISO_W, seed=972000, hf_days=cases.hf_days(ISO_K))
    n_r = inp["n_r"]
    row_idx = (inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32)
    clean = _iso_sweep(dev, strategy, inp["panel"], row_idx, inp)
    assert (clean[1] == 0).all()
    pos = n_r - 260
    extra = inp["panel"][row_idx[1, pos]].copy()
    extra[70] = damage
    bad_idx = row_idx.copy()
    bad_idx[1, pos] = inp["panel"].shape[0]                # window 1 alone reads the extra row
    hit = _iso_sweep(dev, strategy, np.concatenate([inp["panel"], extra[None, :]], axis=0), bad_idx, inp)
    for c, h in zip(clean, hit):
        assert np.array_equal(c[0], h[0])                  # the other window
        assert np.array_equal(c[1][:, :2], h[1][:, :2])    # lengths 200 and 240 of the damaged window: bit for bit
    assert (hit[1][1][:, :2] == _native.STATUS_OK).all()
    if np.isnan(damage):
        assert (hit[1][1][:, 2:] != _native.STATUS_OK).all(), hit[1]
    else:
        assert (np.abs(hit[0][1][:, 2:] - clean[0][1][:, 2:]).max(axis=-1) > 0).all()


def test_jeffreys_length_of_fewer_rows_than_columns_gets_the_status_of_a_run_on_that_suffix(dev):
    k, N, W = 260, 340, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=972100)
    n_r = inp["n_r"]
    short = 100                                            # fewer rows than columns
    Nl = np.array([short + 1, 300, N], dtype=np.int32)
    rows = np.tile(np.array([short, 299, n_r], dtype=np.int32), (W, 1))
    b = dev.batch("jeffreys", k, N, n_r, GAMMA, W, 0)
    b.upload(inp["panel"], start=inp["start"])
    wts, status, _ = b.window_sweep_tiled(Nl, rows)
    b.close()
    # the expectation: a plain batch (k = 260: the tiled pipeline) over the last `short` rows of every window
    s = dev.batch("jeffreys", k, short + 1, short, GAMMA, W, 0)
    s.upload(inp["panel"], start=inp["start"] + (n_r - short))
    _, sstat, _ = s.run().download()
    s.close()
    print(f"status of the short length: sweep {status[:, 0, 0].tolist()}, run on the suffix {sstat.tolist()}")
    assert (sstat != _native.STATUS_OK).all()
    assert np.array_equal(status[:, 0, 0], sstat)
    assert (status[:, 0, 1:] == _native.STATUS_OK).all(), status
    from oracle import oracle
    for l in (1, 2):
        ref = np.stack([oracle.jeffreys_window(inp["panel"][inp["start"][w] + n_r - rows[w, l]:inp["start"][w] + n_r], int(Nl[l]), GAMMA)
                        for w in range(W)])
        assert_close(wts[:, 0, l], ref, what=f"rows={rows[0, l]} next to a rank-deficient length")


# ---- 4. refusals ------------------------------------------------------------------------------------------------------
def test_window_sweep_tiled_refusals(dev):
    smax = _native.sweep_max_assets()
    assert smax == 143
    pd_ = ctypes.POINTER(ctypes.c_double)
    ptr = lambda a: a.ctypes.data_as(pd_)

    def code(fn):
        with pytest.raises(_native.TangencyError) as e:
            fn()
        return e.value.code

    def batch_of(k, N=200, W=2):
        inp = synthetic.make_kernel_inputs(k, N, W, seed=973000 + k, hf_days=cases.hf_days(k))
        b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
        b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
        Nl = np.array([50, N], dtype=np.int32)
        rows = np.tile(np.array([49, inp["n_r"]], dtype=np.int32), (W, 1))
        n0 = np.repeat(inp["n0"][:, None, None], 2, axis=2)
        return b, inp, Nl, rows, n0, np.ascontiguousarray(inp["w0"][:, None, :])

    b, inp, Nl, rows, n0, w0 = batch_of(smax)              # k = 143: the LDS sweep serves it
    assert code(lambda: b.window_sweep_tiled(Nl, rows, n0, w0)) == _native.TP_ERR_UNSUPPORTED
    assert (b.window_sweep(Nl, rows, n0, w0)[1] == 0).all()
    b.close()

    b, inp, Nl, rows, n0, w0 = batch_of(smax + 1)          # k = 144
    assert code(lambda: b.window_sweep(Nl, rows, n0, w0)) == _native.TP_ERR_UNSUPPORTED     # the LDS sweep still stops at 143
    out = np.empty((2, 1, 2, smax + 1))
    assert _native.lib.tp_batch_download_window_sweep(b._b, ptr(out), None, None) == _native.TP_ERR_INVALID   # no sweep before it
    wts, status, aux = b.window_sweep_tiled(Nl, rows, n0, w0)
    assert (status == 0).all()
    # invalid rows / N / delta: TP_ERR_INVALID, and the previous sweep's download stays intact
    INV = _native.TP_ERR_INVALID
    for w, l, bad in ((0, 0, 0), (1, 1, inp["n_r"] + 1), (0, 1, 48)):                       # < 1, > n_w, decreasing
        rb = rows.copy()
        rb[w, l] = bad
        assert code(lambda: b.window_sweep_tiled(Nl, rb, n0, w0)) == INV, (w, l, bad)
    for badN in ([0, 200], [50, 50], [200, 50]):                                            # < 1, not strictly increasing
        assert code(lambda: b.window_sweep_tiled(np.asarray(badN, dtype=np.int32), rows, n0, w0)) == INV, badN
    db = np.zeros((2, 2, inp["n_r"]))
    db[1, 0, inp["n_r"] - 1] = np.nan
    assert code(lambda: b.window_sweep_tiled(Nl, rows, n0, w0, delta=db)) == INV
    n0b = n0.copy()
    n0b[1, 0, 1] = -1.0
    assert code(lambda: b.window_sweep_tiled(Nl, rows, n0b, w0)) == INV
    out[:] = 0
    st = np.full((2, 1, 2), -1, dtype=np.int32)
    assert _native.lib.tp_batch_download_window_sweep(b._b, ptr(out), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None) == 0
    assert np.array_equal(out, wts) and np.array_equal(st, status)
    again = b.window_sweep_tiled(Nl, rows, n0, w0)                                          # the batch still works
    for x, y in zip((wts, status, aux), again):
        assert np.array_equal(x, y)
    b.close()

    j = dev.batch("jeffreys", smax + 1, 200, 199, GAMMA, 2, 0)
    j.upload(inp["panel"], start=inp["start"])
    assert code(lambda: j.window_sweep_tiled(Nl, rows, n0, w0)) == INV                      # Jeffreys with priors
    j.close()


# ---- 5. the product path ----------------------------------------------------------------------------------------------
def _spec(strat, k, N, scaling=1):
    return {"weighting_strategy": strat, "size": k, "risk_aversion": 5, "turnover_cost": 15,
            "rebalancing_frequency": "daily", "rolling_window": N, "rolling_window_frequency": "daily",
            "mcm_scaling": scaling, "display_name": f"{strat}_{N}_{scaling}"}


@pytest.mark.parametrize("names", [("conjugate_hf_vix_vw", "conjugate_hf_epu_ew"), ("jeffreys",)])
def test_calculate_weights_for_windows_takes_the_tiled_sweep_when_switched_on(names, monkeypatch):
    """k = 150, daily windows of 300, 330 and 360 days (about twice the columns: windows with barely more rows than columns are
    ill-conditioned, and two device paths then differ by their roundings times the condition number, which tests neither) at
    six dates; the first dates lie fewer than 360 days into the data, so the longest window is truncated there."""
    from incorporating_different_sources_amd import batch, portfolio_calculations as pc
    k, windows = 150, [300, 330, 360]
    md, _ = synthetic.make_market_data(n_tickers=160, n_days=372, seed=20240095)
    days = md["stock_prices_df"].index
    dates = [pd.Timestamp(d) for d in days[347:371:4]]
    assert len(dates) <= 12
    specs = [_spec(name, k, N, 5 if name.endswith("ew") else 1) for name in names for N in windows]
    batch.clear_panel_cache()
    plain = [pc._weights_for_dates(dates, sp, md) for sp in specs]
    batch.clear_panel_cache()
    packs, sweeps = [], []
    real_pack, real_sweep = batch.pack_windows_lengths, _native.Batch.window_sweep_tiled

    def pack(d, sp, wins, m, **kw):
        packs.append(real_pack(d, sp, wins, m, **kw))
        return packs[-1]

    def sweep(self, N, rows, n0=None, w0=None, delta=None, **kw):
        sweeps.append((list(N), None if n0 is None else n0.shape, None if w0 is None else w0.shape))
        return real_sweep(self, N, rows, n0, w0, delta=delta, **kw)

    monkeypatch.setattr(batch, "pack_windows_lengths", pack)
    monkeypatch.setattr(_native.Batch, "window_sweep_tiled", sweep)
    monkeypatch.setattr(_native.Batch, "window_sweep", lambda *a, **kw: pytest.fail("the LDS sweep was called at k = 150"))
    monkeypatch.setattr(pc, "WINDOW_SWEEP_TILED", True)
    shared = pc.calculate_weights_for_windows(dates, specs, md)
    W = len(dates)
    conj = names[0] != "jeffreys"
    assert len(packs) == 1 and packs[0][5].all()
    rows = packs[0][3]
    assert (rows[:, 2] < 359).any() and (rows[:, 2] >= 359).any()      # the longest window is truncated at the first dates only
    assert sweeps == [(windows, (W, 2, 3) if conj else None, (W, 2, k) if conj else None)]
    for sp, a, b in zip(specs, plain, shared):
        assert b[0].shape == (W, k)
        assert_close(b[0], a[0], what=sp["display_name"])
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    batch.clear_panel_cache()
