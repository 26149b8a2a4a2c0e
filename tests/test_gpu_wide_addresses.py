"""Panels of 4 GiB and more and every edge of the 32-bit offsets (-m gpu): the 64-bit branches of every Gram kernel family,
the 32-bit branches at the top of their range, the flag word each panel of a batch gets, the gate of the shared block sums and
the sweeps' Gram passes.  The cases are tests/_wide_address_cases.py (tests/test_host_addressing.py pins their flags on the CPU).

A far panel is np.zeros whose pages are never touched, apart from a low block of live rows at its top and a high block at
its very end; every window takes rows of both.  A truncated offset lands in the low block (finite, wrong) or in the zero
middle (a non-positive pivot): statuses or weights miss.  The oracle gets the compact panel of the live rows alone, row indices
remapped - the same operation on the same numbers - and the same windows, uploaded as the compact panel (the 32-bit form the
rest of the suite vouches for), must agree with the far run too.  Tolerances: those of tests/test_gpu_fuzz.py (flat 1e-10 on
the weights, rtol 1e-11 / atol 1e-14 on conjugate aux), WTOL of tests/test_gpu_round3b.py on the tiled path (the same figure),
and the sweep tests' own helpers and bounds.  Every test prints its flags and whether far and compact runs were bit-equal."""
import numpy as np
import pytest

from incorporating_different_sources_amd import _native
from oracle import oracle

import _wide_address_cases as cases
from _window_sweep_cases import bound as window_sweep_bound
from test_gpu_prior_sweep import assert_close, make_priors, oracle_sweep
from test_gpu_round3b import WTOL

pytestmark = pytest.mark.gpu

GAMMA = 5.0
AUX_TOL = dict(rtol=1e-11, atol=1e-14)


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


# ---- data -------------------------------------------------------------------------------------------------------------------
def returns(rng, n, width, intraday):
    """Rows with the statistics of synthetic.make_kernel_inputs: one-factor daily excess returns, iid intraday returns."""
    if intraday:
        return rng.normal(0.0, 0.001, size=(n, width))
    beta = rng.uniform(0.5, 1.5, size=width)
    f = rng.normal(0.0, 0.01, size=n)
    return 3e-4 + f[:, None] * beta[None, :] + rng.normal(0.0, 0.01, size=(n, width))


def far_panel(rng, rows, ld, live, intraday=False):
    """(far [rows x ld], compact [2 live x ld]): untouched zero pages between a low block at rows [0, live) and a high block at
    rows [rows - live, rows)."""
    compact = returns(rng, 2 * live, ld, intraday)
    far = np.zeros((rows, ld))
    far[:live] = compact[:live]
    far[rows - live:] = compact[live:]
    return far, compact


def window_rows(rng, W, count, live, rows, last_row=True):
    """([W x count] rows of the far panel, the same rows of the compact one): every window takes about half its rows from
    each block, sorted; windows 0 and 2 end on the panel's last row."""
    far = np.empty((W, count), dtype=np.int32)
    compact = np.empty((W, count), dtype=np.int32)
    for w in range(W):
        n_low = count // 2 + int(rng.integers(-2, 3)) if count > 8 else count // 2
        low = np.sort(rng.choice(live, n_low, replace=False))
        high = np.sort(rng.choice(live, count - n_low, replace=False))
        if last_row and w != 1:
            high[-1] = live - 1
        compact[w] = np.concatenate([low, live + high])
        far[w] = np.concatenate([low, rows - live + high])
    assert (np.diff(far.astype(np.int64), axis=1) > 0).all() and (not last_row or far.max() == rows - 1)
    return far, compact


def gathered_columns(rng, W, k, ld):
    """[W x k] sorted columns out of ld, column ld - 1 among them: the largest offset a load forms is the panel's last element."""
    cols = np.stack([np.sort(np.append(rng.choice(ld - 1, k - 1, replace=False), ld - 1)) for _ in range(W)])
    return cols.astype(np.int32)


def ragged(count, W, by):
    """Row counts: window 1 is `by` rows short."""
    n = np.full(W, count, dtype=np.int32)
    n[1] = count - by
    return n


def explicit_inputs(c):
    """(far upload keywords, compact upload keywords) of an explicit-row case; the panels travel under "panel" / "hf_panel"."""
    rng = np.random.default_rng(sum(map(ord, c["id"])) + 7700000)
    k, ld, W, n_r, m = c["k"], c["ld"], c["W"], c["n_r"], c["m"]
    conj = c["strategy"] == "conjugate"
    daily_far = c["far"] == "daily"
    if daily_far:
        panel, cpanel = far_panel(rng, c["panel_rows"], ld, n_r)
        rows, crows = window_rows(rng, W, n_r, n_r, c["panel_rows"], c["last_row"])
    else:
        cpanel = returns(rng, 2 * n_r, ld, False)
        panel = cpanel
        rows = crows = np.stack([np.sort(rng.choice(2 * n_r, n_r, replace=False)) for _ in range(W)]).astype(np.int32)
    common = dict(col_idx=gathered_columns(rng, W, k, ld), n_rows=ragged(n_r, W, 3))
    if c["rf_adj"]:
        common["rf_adj"] = rng.normal(1e-4, 3e-5, size=(W, n_r))
    far = dict(common, panel=panel, row_idx=rows)
    compact = dict(common, panel=cpanel, row_idx=crows)
    if conj:
        if daily_far:
            chf = returns(rng, 2 * m, ld, True)
            hf = chf
            hrows = chrows = np.stack([np.sort(rng.choice(2 * m, m, replace=False)) for _ in range(W)]).astype(np.int32)
        else:
            hf, chf = far_panel(rng, c["hf_rows"], ld, m, intraday=True)
            hrows, chrows = window_rows(rng, W, m, m, c["hf_rows"])
        w0 = np.abs(rng.normal(size=(W, k))) + 0.1
        prior = dict(w0=w0 / w0.sum(1, keepdims=True), n0=c["N"] * rng.uniform(1.0, 1.6, size=W), hf_count=ragged(m, W, 5))
        far.update(prior, hf_panel=hf, hf_row_idx=hrows)
        compact.update(prior, hf_panel=chf, hf_row_idx=chrows)
    return far, compact


def contiguous_inputs(c):
    """(upload keywords of the wide panel, of its compact twin, which holds the live columns alone)."""
    rng = np.random.default_rng(sum(map(ord, c["id"])) + 7800000)
    k, ld, W, n_r, m = c["k"], c["ld"], c["W"], c["n_r"], c["m"]
    rows = c["panel_rows"]
    common = dict(start=np.asarray(c["starts"], dtype=np.int64))
    if W <= 16:
        common["n_rows"] = ragged(n_r, W, 3)
    if c["cols"]:
        live = np.sort(np.append(rng.choice(ld - 1, k + 7, replace=False), ld - 1))      # k + 8 live columns over the whole width
        pick = np.stack([np.sort(np.append(rng.choice(k + 7, k - 1, replace=False), k + 7)) for _ in range(W)])
        cpanel = returns(rng, rows, k + 8, False)
        wide, compact = dict(common, col_idx=live[pick].astype(np.int32)), dict(common, col_idx=pick.astype(np.int32))
    else:
        live = np.arange(k)
        cpanel = returns(rng, rows, k, False)
        wide, compact = dict(common), dict(common)
    panel = np.zeros((rows, ld))
    panel[:, live] = cpanel
    wide["panel"], compact["panel"] = panel, cpanel
    if m:
        hf = returns(rng, c["hf_rows"], c["hf_ld"], True)
        w0 = np.abs(rng.normal(size=(W, k))) + 0.1
        prior = dict(hf_panel=hf, hf_start=np.arange(W, dtype=np.int64) * cases.BARS, w0=w0 / w0.sum(1, keepdims=True),
                     n0=c["N"] * rng.uniform(1.0, 1.6, size=W))
        wide.update(prior)
        compact.update(prior)
    return wide, compact


# ---- running ----------------------------------------------------------------------------------------------------------------
def run(dev, c, kw, flags=0):
    """Upload, run, download, close -> (weights, status, aux, (daily flags, intraday flags), shared daily blocks, last launch)."""
    kw = dict(kw)
    panel = kw.pop("panel")
    b = dev.batch(c["strategy"], c["k"], c["N"], c["n_r"], GAMMA, c["W"], c["m"], flags)
    try:
        b.upload(panel, **kw)
        addressing, shared = b.addressing(), b.shared_gram_blocks()
        wts, status, aux = b.run().download()
        launch = dev.last_launch()
    finally:
        b.close()
    return wts, status, aux, addressing, shared, launch


def reference(c, kw, sample=None):
    kw = dict(kw)
    panel = kw.pop("panel")
    if sample is not None:
        kw = {key: (val[list(sample)] if key not in ("hf_panel",) and val is not None else val) for key, val in kw.items()}
    kw.setdefault("start", None)
    if c["m"]:
        kw["m"] = c["m"]
    return oracle.posterior_batch_c(c["strategy"], c["k"], c["N"], GAMMA, panel, n_r=c["n_r"], **kw)


def check_run(c, got, ref, twin, sample=None):
    """Statuses and weights (aux: conjugate) of the wide run against the oracle and against the compact run."""
    wts, status, aux = got[:3]
    rw, rstat, raux = ref
    sel = slice(None) if sample is None else list(sample)
    assert (rstat == 0).all(), (c["id"], "the oracle itself rejects a window of this case", rstat)
    assert (status[sel] == rstat).all(), (c["id"], status[sel], rstat)
    err = float(np.abs(wts[sel] - rw).max())
    tw, tstat, taux = twin[:3]
    equal = bool(np.array_equal(wts, tw) and np.array_equal(status, tstat) and np.array_equal(aux, taux))
    print(f"wide-address {c['id']}: flags={got[3]} compact flags={twin[3]} shared blocks={got[4]} launch={tuple(got[5].values())} "
          f"max|hip - oracle|={err:.3e} max|wide - compact|={float(np.abs(wts - tw).max()):.3e} bit_equal={equal}")
    np.testing.assert_allclose(wts[sel], rw, err_msg=c["id"], **WTOL)
    assert (tstat == status).all(), (c["id"], tstat, status)
    np.testing.assert_allclose(tw, wts, err_msg=c["id"] + " compact", **WTOL)
    if c["strategy"] == "conjugate":
        np.testing.assert_allclose(aux[sel, :6], raux[:, :6], err_msg=c["id"], **AUX_TOL)
        np.testing.assert_allclose(taux[:, :6], aux[:, :6], err_msg=c["id"] + " compact", **AUX_TOL)


def with_options(dev, options):
    for name, value in options.items():
        dev.set_option(name, value)


# ---- A - F: runs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cases.RUN_CASES, ids=[c["id"] for c in cases.RUN_CASES])
def test_run_matches_oracle_and_compact_twin(dev, c):
    wide, compact = explicit_inputs(c) if c["kind"] == "explicit" else contiguous_inputs(c)
    with_options(dev, c["options"])
    try:
        got = run(dev, c, wide)
        assert got[3] == c["expect"], (c["id"], got[3])
        del wide
        twin = run(dev, c, compact)
    finally:
        with_options(dev, {name: -1 for name in c["options"]})
    if c["options"]:
        # the option really changed the kernel: the same (compact) batch under the default options launches another one
        default = run(dev, c, compact)
        assert default[5] != twin[5], (c["id"], default[5], twin[5])
        assert np.array_equal(default[1], twin[1])
        np.testing.assert_allclose(default[0], twin[0], err_msg=c["id"] + " default kernel", **WTOL)
    if c["kind"] == "explicit":
        assert twin[3][0] & 1 and (not c["m"] or twin[3][1] & 1), (c["id"], twin[3])      # the compact twin: 32-bit form
    check_run(c, got, reference(c, compact), twin)


# ---- G: the gate of the shared block sums -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cases.G, ids=[c["id"] for c in cases.G])
def test_shared_sums_gate(dev, c):
    wide, compact = contiguous_inputs(c)
    got = run(dev, c, wide)
    assert got[3] == c["expect"], (c["id"], got[3])
    assert (got[4] > 0) == c["shared"], (c["id"], got[4])
    del wide
    twin = run(dev, c, compact)
    assert twin[4] > 0                             # ld = k: the compact twin always shares
    check_run(c, got, reference(c, compact, c["sample"]), twin, c["sample"])


# ---- H: the sweeps' Gram passes ---------------------------------------------------------------------------------------------
PRIOR = [c for c in cases.H if c["sweep"] == "prior"]
WINDOW = [c for c in cases.H if c["sweep"] == "window"]


def sweep_batch(dev, c, kw):
    kw = dict(kw)
    panel = kw.pop("panel")
    b = dev.batch(c["strategy"], c["k"], c["N"], c["n_r"], GAMMA, c["W"], c["m"])
    b.upload(panel, **kw)
    return b


@pytest.mark.parametrize("c", PRIOR, ids=[c["id"] for c in PRIOR])
def test_prior_sweep_over_a_far_panel(dev, c):
    """Daily panel far: the daily Gram pass in 64-bit form.  Intraday panel far: the intraday pass runs as a daily pass over
    the intraday panel and must be handed the intraday flag word."""
    W, P, k = c["W"], 4, c["k"]
    wide, compact = explicit_inputs(c)
    n0, w0 = make_priors(np.random.default_rng(7900000 + k), W, P, k, c["N"])
    out = []
    for kw in (wide, compact):
        b = sweep_batch(dev, c, kw)
        try:
            flags = b.addressing()
            out.append(b.prior_sweep(n0, w0) + (flags,))
        finally:
            b.close()
    del wide
    (wts, status, aux, flags), (tw, tstat, taux, tflags) = out
    assert flags == c["expect"] and tflags == (3, 3), (c["id"], flags, tflags)
    assert (status == _native.STATUS_OK).all() and (tstat == _native.STATUS_OK).all(), (status, tstat)
    okw = {key: val for key, val in compact.items() if key != "panel"}
    ref, raux = oracle_sweep(k, c["N"], compact["panel"], dict(okw, start=None, n_r=c["n_r"], m=c["m"]), n0, w0)
    equal = bool(np.array_equal(wts, tw) and np.array_equal(aux, taux))
    print(f"wide-address {c['id']}: flags={flags} compact flags={tflags} bit_equal={equal}")
    assert_close(wts, ref, what=c["id"])
    np.testing.assert_allclose(aux[..., :6], raux[..., :6], **AUX_TOL)
    assert_close(tw, wts, what=c["id"] + " compact vs far")
    np.testing.assert_allclose(taux[..., :6], aux[..., :6], **AUX_TOL)


@pytest.mark.parametrize("c", WINDOW, ids=[c["id"] for c in WINDOW])
def test_window_sweep_over_a_far_panel(dev, c):
    W, k, n_r = c["W"], c["k"], c["n_r"]
    wide, compact = explicit_inputs(c)
    n_w = compact["n_rows"]
    Nl = np.asarray(c["lengths"], dtype=np.int32) + 1
    rows = np.stack([np.minimum(np.asarray(c["lengths"]) - w, n_w[w]) for w in range(W)]).astype(np.int32)
    out = []
    for kw in (wide, compact):
        b = sweep_batch(dev, c, kw)
        try:
            flags = b.addressing()
            out.append(b.window_sweep(Nl, rows) + (flags,))
        finally:
            b.close()
    del wide
    (wts, status, aux, flags), (tw, tstat, taux, tflags) = out
    assert flags == c["expect"] and tflags == (3, 0), (c["id"], flags, tflags)
    assert (status == _native.STATUS_OK).all() and (tstat == _native.STATUS_OK).all(), (status, tstat)
    equal = bool(np.array_equal(wts, tw) and np.array_equal(aux, taux))
    print(f"wide-address {c['id']}: flags={flags} compact flags={tflags} bit_equal={equal}")
    for l in range(len(Nl)):
        # the oracle on the suffix: the last rows[w, l] rows of the window as uploaded, with that length's N (what
        # _window_sweep_cases.suffix_inputs does for its own table of two windows; this case has three and no rf_adj)
        suffix = np.zeros((W, n_r), dtype=np.int32)
        for w in range(W):
            r = int(rows[w, l])
            suffix[w, :r] = compact["row_idx"][w, n_w[w] - r:n_w[w]]
        ref, rstat, _ = oracle.posterior_batch("jeffreys", k, int(Nl[l]), GAMMA, compact["panel"], None, n_r, row_idx=suffix,
                                               n_rows=rows[:, l].copy(), col_idx=compact["col_idx"])
        assert (rstat == 0).all()
        assert_close(wts[:, 0, l], ref, what=f"{c['id']} rows={rows[:, l].tolist()}")
        assert float(np.abs(tw[:, 0, l] - wts[:, 0, l]).max()) <= window_sweep_bound(ref)
