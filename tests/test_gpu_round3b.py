"""Round 3 (-m gpu): gaps the round-2 verdict and advice named.

* a non-finite panel row in the contiguous (shared-Gram) layout poisons exactly the windows that contain it;
* the reference golden at k = 200 - the multi-wave / two-wave kernels' own range - on the GPU;
* configs[2] at its full 50,000 windows: determinism + sampled oracle windows (item 6c);
* a synchronous upload, a run, then an asynchronous upload of the same batch: the copy waits for the launch;
* handle options replace the environment switches (item 3)."""
import os

import numpy as np
import pytest

from oracle import oracle
from incorporating_different_sources_amd import synthetic

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
WTOL = dict(rtol=0, atol=1e-10)


@pytest.fixture(scope="module")
def native():
    from incorporating_different_sources_amd import _native
    return _native


@pytest.mark.parametrize("k,N,hf_days", [(20, 60, 1), (100, 250, 1), (150, 200, 2), (260, 300, 4)])
@pytest.mark.parametrize("bad", [np.nan, np.inf, 1e200])
def test_a_non_finite_row_poisons_only_the_windows_that_contain_it(native, k, N, hf_days, bad):
    """Rolling windows over one panel take their whole 16-row blocks from sliding block-window sums.
    One NaN / Inf / overflowing value in panel row r must flag the windows [r - n_r + 1, r] and nobody else: round 2's
    slide (add the entering block, subtract the leaving one) kept Inf - Inf = NaN in every later position of its run.
    Statuses equal the no-sharing path's (TP_FLAG_NO_SHARED_GRAM) window by window; clean windows agree to 1e-12."""
    W = 400
    inp = synthetic.make_kernel_inputs(k, N, W, seed=4242 + k, hf_days=hf_days)
    n_r = inp["n_r"]
    panel = inp["panel"].copy()
    r_bad, c_bad = n_r + 37, min(3, k - 1)
    panel[r_bad, c_bad] = bad
    kw = dict(panel=panel, start=inp["start"], n_r=n_r, hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=inp["m"],
              w0=inp["w0"], n0=inp["n0"])
    dev = native.default_device()
    b = native.Batch(dev, "conjugate", k, N, n_r, 5.0, W, inp["m"])
    try:
        b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
        assert b.shared_gram_blocks() > 0                                  # the layout under test
        b.run()
        w_sh, s_sh, _ = b.download()
    finally:
        b.close()
    w_no, s_no, _ = native.posterior_batch("conjugate", k, N, 5.0, flags=native.FLAG_NO_SHARED_GRAM, **kw)
    contains = (inp["start"] <= r_bad) & (r_bad < inp["start"] + n_r)
    assert contains.sum() == n_r
    assert (s_sh[contains] != 0).all() and (s_no[contains] != 0).all()
    assert (s_sh[~contains] == 0).all(), np.flatnonzero((s_sh != 0) & ~contains)[:10]
    assert np.array_equal(s_sh != 0, s_no != 0)
    np.testing.assert_allclose(w_sh[~contains], w_no[~contains], rtol=0, atol=1e-12)
    clean = dict(kw, panel=inp["panel"])
    w_clean, s_clean, _ = native.posterior_batch("conjugate", k, N, 5.0, **clean)
    np.testing.assert_allclose(w_sh[~contains], w_clean[~contains], rtol=0, atol=1e-12)


@pytest.mark.parametrize("strat", ["conjugate_hf_vix_vw", "conjugate_hf_vix_ew", "jeffreys"])
@pytest.mark.parametrize("choice", [-1, 0])
def test_k200_matches_reference_golden(native, strat, choice):
    """`single_k200_n250`: outputs of the unmodified reference at k = 200 (13 tiles per side: above the one-wave kernel's
    range) - conjugate vw / ew at the flat 1e-10, and the Jeffreys parity SURVEY section 8(d) asks for at a shape where
    J is invertible (k <= N - 2).  Jeffreys at k = 200 over 249 rows has a rank margin of 49: the reference's own LU
    inverse is only good to ~1e-8 relative there (tests/test_oracle_golden.py uses the same bound for the oracle).
    choice: -1 = the kernel the library picks for this size, 0 = the multi-wave kernel."""
    g = np.load(os.path.join(GOLDEN, "single_k200_n250.npz"))
    k, N, hf_days, seed = int(g["k"]), int(g["N"]), int(g["hf_days"]), int(g["seed"])
    inp = synthetic.make_kernel_inputs(k, N, 1, seed, hf_days=hf_days)
    n_r, m = inp["n_r"], inp["m"]
    P = 100.0 * np.exp(np.concatenate([np.zeros((1, k)), np.cumsum(inp["panel"][:n_r], axis=0)]))
    X = oracle.excess_log_returns_from_prices(P)
    H = 50.0 * np.exp(np.concatenate([np.zeros((1, k)), np.cumsum(inp["hf_panel"][:m], axis=0)]))
    Y = oracle.excess_log_returns_from_prices(H)
    dev = native.default_device()
    dev.set_option("wave_kernel", choice)
    try:
        if strat == "jeffreys":
            wts, status, _ = native.posterior_batch("jeffreys", k, N, 5.0, panel=X, start=np.zeros(1, np.int64), n_r=n_r)
            tol = dict(rtol=1e-7, atol=1e-9)
        else:
            order = g[f"w0_{strat}_order"].astype(np.int32)
            wts, status, aux = native.posterior_batch(
                "conjugate", k, N, 5.0, panel=X, start=np.zeros(1, np.int64), n_r=n_r, hf_panel=Y,
                hf_start=np.zeros(1, np.int64), m=m, w0=g[f"w0_{strat}_w0"][None, :],
                n0=np.array([float(g[f"w0_{strat}_n0"])]), col_idx=order[None, :])
            tol = WTOL
            assert aux[0, 2] == pytest.approx(float(g[f"w0_{strat}_c"]), rel=1e-11)
            assert aux[0, 4] == pytest.approx(float(g[f"w0_{strat}_q1"]), rel=1e-8)
    finally:
        dev.set_option("wave_kernel", -1)
    assert status[0] == 0
    np.testing.assert_allclose(wts[0], g[f"w0_{strat}_weights"], **tol)


def test_configs2_at_its_full_window_count(native):
    """BASELINE configs[2] as stated: k = 500, N = 250, m = 389, 50,000 windows on one GPU - determinism (two runs
    bit-identical), every status OK, 8 sampled windows against the oracle at the flat 1e-10.  The intraday panel wraps
    after 8,192 days (2.5 GB of host memory instead of 15.6 GB; a window's rows are the same kind of data either way -
    what the wrap does to the HBM footprint is measured in DESIGN section 5, not here)."""
    shp = synthetic.config_shapes(3)
    W = 50_000
    inp = synthetic.make_kernel_inputs(shp["k"], shp["N"], W, seed=shp["seed"], hf_days=shp["hf_days"], hf_period=8192)
    kw = dict(panel=inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"],
              n0=inp["n0"])
    dev = native.default_device()
    b = native.Batch(dev, "conjugate", shp["k"], shp["N"], shp["n_r"], 5.0, W, shp["m"])
    try:
        b.upload(**kw)
        b.run()
        w1, s1, a1 = b.download()
        b.run()
        w2, s2, a2 = b.download()
    finally:
        b.close()
    assert (s1 == 0).all() and np.isfinite(w1).all()
    assert np.array_equal(w1, w2) and np.array_equal(a1, a2)
    sample = np.unique(np.concatenate([[0, W - 1], np.random.default_rng(3).integers(0, W, 6)]))
    sub = {key: (val[sample] if key in ("start", "hf_start", "w0", "n0") else val) for key, val in kw.items()}
    ref, rstat, raux = oracle.posterior_batch_c("conjugate", shp["k"], shp["N"], 5.0, n_r=shp["n_r"], m=shp["m"], **sub)
    assert (rstat == 0).all()
    np.testing.assert_allclose(w1[sample], ref, **WTOL)
    np.testing.assert_allclose(a1[sample, :6], raux[:, :6], rtol=1e-11, atol=1e-14)


def test_async_upload_after_a_run_waits_for_the_launch(native):
    """tp_batch_upload (synchronous), tp_batch_run, tp_batch_upload_async on the SAME batch: the copy stream
    must not overwrite the panels the running launch still reads.  The end of every launch is an event the next
    asynchronous upload waits for; results of run 1 are those of inputs 1, of run 2 those of inputs 2."""
    k, N, W = 100, 250, 6000
    a = synthetic.make_kernel_inputs(k, N, W, seed=501)
    c = synthetic.make_kernel_inputs(k, N, W, seed=502)
    names = ("panel", "start", "hf_panel", "hf_start", "w0", "n0")
    ref_a, _, _ = native.posterior_batch("conjugate", k, N, 5.0, n_r=a["n_r"], m=a["m"], **{n: a[n] for n in names})
    ref_c, _, _ = native.posterior_batch("conjugate", k, N, 5.0, n_r=c["n_r"], m=c["m"], **{n: c[n] for n in names})
    pinned_c = {n: native.pinned_copy(c[n]) for n in names}
    dev = native.default_device()
    b = native.Batch(dev, "conjugate", k, N, a["n_r"], 5.0, W, a["m"])
    try:
        b.upload(**{n: a[n] for n in names})
        for _ in range(3):
            b.run()                                   # three launches queued: the kernel stream is busy ...
        b.upload_async(**pinned_c)                    # ... while the copies are queued on the copy stream
        w_a, s_a, _ = b.download()                    # results of the launches that read inputs A
        b.run()
        w_c, s_c, _ = b.download()
    finally:
        b.close()
    assert np.array_equal(w_a, ref_a) and np.array_equal(w_c, ref_c)


def test_options_are_per_handle_and_the_environment_is_read_once(native, monkeypatch):
    """kernel-selection switches live on the handle.  Changing the environment after a Device exists
    changes nothing for it; `set_option` does; an unknown option is an error."""
    k, N, W = 100, 120, 64
    inp = synthetic.make_kernel_inputs(k, N, W, seed=9)
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
    dev = native.Device(0)
    try:
        native.posterior_batch("jeffreys", k, N, 5.0, device=dev, **kw)
        one_wave = dev.last_launch()["block"]
        monkeypatch.setenv("TP_WAVE_KERNEL", "0")
        native.posterior_batch("jeffreys", k, N, 5.0, device=dev, **kw)
        assert dev.last_launch()["block"] == one_wave == 64              # the environment is not consulted at launch
        dev.set_option("wave_kernel", 0)
        native.posterior_batch("jeffreys", k, N, 5.0, device=dev, **kw)
        assert dev.last_launch()["block"] == 256                        # the multi-wave kernel: 4 waves per window
        with pytest.raises(native.TangencyError):
            dev.set_option("no_such_switch", 1)
        dev2 = native.Device(0)                                          # a NEW handle reads the environment
        try:
            native.posterior_batch("jeffreys", k, N, 5.0, device=dev2, **kw)
            assert dev2.last_launch()["block"] == 256
        finally:
            dev2.close()
    finally:
        dev.close()


def test_retired_large_k_options_are_refused_and_leave_the_handle_usable(native):
    """The depth-first sub-batches ("tiled_lanes") and the 64 x 128 Gram kernel ("tiled_wave" = 2) were measured, not
    adopted and removed: `set_option` answers both with an error, and the handle that refused them
    still runs the large-k path - bit-equal to a fresh handle's run of the same batch."""
    k, N, W = 260, 520, 4
    inp = synthetic.make_kernel_inputs(k, N, W, seed=13)
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
    dev = native.Device(0)
    try:
        with pytest.raises(native.TangencyError):
            dev.set_option("tiled_lanes", 2)
        with pytest.raises(native.TangencyError):
            dev.set_option("tiled_wave", 2)
        wts, status, aux = native.posterior_batch("jeffreys", k, N, 5.0, device=dev, **kw)
    finally:
        dev.close()
    fresh = native.Device(0)
    try:
        wts_f, status_f, aux_f = native.posterior_batch("jeffreys", k, N, 5.0, device=fresh, **kw)
    finally:
        fresh.close()
    assert (status == 0).all() and (status_f == 0).all()
    assert np.array_equal(wts, wts_f) and np.array_equal(aux, aux_f)


# ---- the two- / four-wave-per-window kernel (csrc/posterior_wave2_impl.h): 10..15 tiles per side, 144 <= k <= 239 ------
def _kw(inp, strat):
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
    if strat == "conjugate":
        kw.update(hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    return kw


@pytest.mark.parametrize("strat", ["conjugate", "jeffreys"])
def test_every_universe_size_of_the_two_wave_kernel(native, strat):
    """EVERY k = 144 .. 239 (six tile counts; two waves per window up to 12 tiles per side, four above; every position
    of the border column inside its tile, the two-pass sizes k + 1 = 0 mod 16) on the kernel the library now picks for
    these sizes: against the oracle at the flat 1e-10 and against the multi-wave kernel it replaces (same arithmetic per
    element up to the order of the partial sums of the back substitution: 1e-12)."""
    dev = native.default_device()
    worst = 0.0
    try:
        for k in range(144, 240):
            N = max(2 * k + 10, 40) if strat == "jeffreys" else max(k + 30, 40)
            inp = synthetic.make_kernel_inputs(k, N, 7, seed=41000 + k, hf_days=2 if k > 150 else 1)
            kw = _kw(inp, strat)
            ref, rstat, _ = oracle.posterior_batch_c(strat, k, N, 5.0, **kw)
            dev.set_option("wave_kernel", 0)
            w_multi, s_multi, a_multi = native.posterior_batch(strat, k, N, 5.0, **kw)
            assert dev.last_launch()["block"] >= 256
            dev.set_option("wave_kernel", 2)
            w_two, s_two, a_two = native.posterior_batch(strat, k, N, 5.0, **kw)
            assert dev.last_launch()["block"] == (128 if k <= 191 else 256), (k, dev.last_launch())
            assert (s_two == rstat).all() and (s_multi == rstat).all(), (k, s_two, rstat)
            np.testing.assert_allclose(w_two, ref, rtol=0, atol=1e-10, err_msg=f"k={k}")
            # (k + 1 = 0 mod 16: one-pass centred scatter here, two-pass in the multi-wave kernel: 2 ulp apart on S0)
            np.testing.assert_allclose(w_two, w_multi, rtol=0, atol=1e-11 if k % 16 == 15 else 1e-12, err_msg=f"k={k}")
            np.testing.assert_allclose(a_two[:, :6], a_multi[:, :6], rtol=1e-11 if k % 16 == 15 else 1e-12, atol=1e-300, err_msg=f"k={k}")
            worst = max(worst, float(np.abs(w_two - ref).max()))
            dev.set_option("wave_kernel", -1)                          # the automatic pick IS the two-wave kernel there
            w_auto, _, _ = native.posterior_batch(strat, k, N, 5.0, **kw)
            assert np.array_equal(w_auto, w_two) and dev.last_launch()["block"] in (128, 256)
    finally:
        dev.set_option("wave_kernel", -1)
    assert worst < 1e-10


@pytest.mark.parametrize("k,N", [(150, 200), (191, 260), (200, 250), (239, 300)])
def test_two_wave_kernel_layouts_shared_sums_and_singular_windows(native, k, N):
    """The two-wave kernel in every layout: rolling windows with shared Gram sums (400 windows), the same without
    sharing (bitwise the index layout's results with identity indices), ragged index-layout windows with gathered
    columns and a per-row risk-free adjustment against the oracle; a rank-deficient Jeffreys batch is flagged."""
    rng = np.random.default_rng(k)
    W = 400
    inp = synthetic.make_kernel_inputs(k, N, W, seed=4300 + k, hf_days=3)
    n_r, m = inp["n_r"], inp["m"]
    kw = _kw(inp, "conjugate")
    dev = native.default_device()
    b = native.Batch(dev, "conjugate", k, N, n_r, 5.0, W, m)
    try:
        b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
        assert b.shared_gram_blocks() > 0
        b.run()
        w_sh, s_sh, a_sh = b.download()
        assert dev.last_launch()["block"] in (128, 256)
    finally:
        b.close()
    w_no, s_no, a_no = native.posterior_batch("conjugate", k, N, 5.0, flags=native.FLAG_NO_SHARED_GRAM, **kw)
    ikw = dict(panel=inp["panel"], n_r=n_r, row_idx=(inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32),
               col_idx=np.tile(np.arange(k, dtype=np.int32), (W, 1)), rf_adj=np.zeros((W, n_r)), hf_panel=inp["hf_panel"], m=m,
               hf_row_idx=(inp["hf_start"][:, None] + np.arange(m)[None, :]).astype(np.int32), w0=inp["w0"], n0=inp["n0"])
    w_ix, s_ix, a_ix = native.posterior_batch("conjugate", k, N, 5.0, **ikw)
    assert (s_sh == 0).all() and (s_no == 0).all() and (s_ix == 0).all()
    assert np.array_equal(w_no, w_ix)                                   # same rows, same order, same arithmetic
    np.testing.assert_allclose(w_sh, w_no, rtol=0, atol=1e-12)
    sample = np.unique(rng.integers(0, W, 6))
    ref, rstat, raux = oracle.posterior_batch_c("conjugate", k, N, 5.0, **{key: (val[sample] if key in ("start", "hf_start", "w0", "n0") else val)
                                                                            for key, val in kw.items()})
    np.testing.assert_allclose(w_sh[sample], ref, **WTOL)
    np.testing.assert_allclose(a_sh[sample, :6], raux[:, :6], rtol=1e-11, atol=1e-14)
    # ragged general layout
    Wg = 10
    col_idx = np.stack([np.sort(rng.choice(k, k - 9, replace=False)) for _ in range(Wg)]).astype(np.int32)
    kg = k - 9
    row_idx = np.stack([inp["start"][w] + np.sort(rng.choice(n_r, n_r, replace=False)) for w in range(Wg)]).astype(np.int32)
    n_rows = rng.integers(n_r - 9, n_r + 1, size=Wg).astype(np.int32)
    rf_adj = rng.normal(0, 1e-4, size=(Wg, n_r))
    w0 = np.abs(rng.normal(size=(Wg, kg))); w0 /= w0.sum(axis=1, keepdims=True)
    gkw = dict(panel=inp["panel"], start=None, row_idx=row_idx, n_rows=n_rows, col_idx=col_idx, rf_adj=rf_adj, n_r=n_r,
               hf_panel=inp["hf_panel"], hf_start=inp["hf_start"][:Wg], m=m, hf_count=rng.integers(m - 20, m + 1, Wg).astype(np.int32),
               w0=w0, n0=inp["n0"][:Wg])
    refg, rstatg, _ = oracle.posterior_batch_c("conjugate", kg, N, 5.0, **gkw)
    wg, sg, _ = native.posterior_batch("conjugate", kg, N, 5.0, **gkw)
    assert (sg == rstatg).all()
    np.testing.assert_allclose(wg, refg, **WTOL)
    # singular: more assets than rows
    sing = synthetic.make_kernel_inputs(k, 60, 5, seed=1)
    _, s, _ = native.posterior_batch("jeffreys", k, 60, 5.0, panel=sing["panel"], start=sing["start"], n_r=sing["n_r"])
    assert (s != 0).all()


@pytest.mark.parametrize("k,N", [(260, 520), (383, 700), (448, 800)])
def test_tiled_jeffreys_rank_one_term_in_every_layout(native, k, N):
    """Large-k path, Jeffreys: J = T - t t'/N is applied inside the Gram kernel (posterior_tiled_wave.h, RANK1) from the
    border column of the shared table slots and the column sums of the rows a wave stages itself.  The border column sits
    in the first / the last / a middle 16-column group of its super-tile; contiguous windows with the shared sums, without
    them, ragged windows with a risk-free adjustment, gathered columns and explicit rows - against the oracle at 1e-10 and
    against the 4-wave kernels (separate rank-one pass, option tiled_wave = 0)."""
    rng = np.random.default_rng(k)
    W = 14
    width = k + 7
    inp = synthetic.make_kernel_inputs(width, N, W, seed=4100 + k)
    n_r = inp["n_r"]
    dense = np.ascontiguousarray(inp["panel"][:, :k])
    assert W * n_r >= 3 * dense.shape[0]
    kw = dict(panel=dense, start=inp["start"], n_r=n_r)
    w_sh, s_sh, _ = native.posterior_batch("jeffreys", k, N, 5.0, **kw)
    w_no, s_no, _ = native.posterior_batch("jeffreys", k, N, 5.0, flags=native.FLAG_NO_SHARED_GRAM, **kw)
    ref, rstat, _ = oracle.posterior_batch_c("jeffreys", k, N, 5.0, **kw)
    assert (s_sh == rstat).all() and (s_no == rstat).all() and (rstat == 0).all()
    np.testing.assert_allclose(w_sh, ref, **WTOL)
    np.testing.assert_allclose(w_no, ref, **WTOL)
    dev = native.default_device()
    dev.set_option("tiled_wave", 0)
    try:
        w_4w, s_4w, _ = native.posterior_batch("jeffreys", k, N, 5.0, **kw)
    finally:
        dev.set_option("tiled_wave", -1)
    np.testing.assert_allclose(w_sh, w_4w, rtol=0, atol=1e-11 * max(1.0, np.abs(w_4w).max()))
    # general layout: gathered columns, explicit ragged rows, per-row risk-free adjustment, a shift on some windows
    cols = np.stack([np.sort(rng.choice(width, k, replace=False)) for _ in range(W)]).astype(np.int32)
    rows = np.stack([inp["start"][w] + np.sort(rng.choice(n_r, n_r, replace=False)) for w in range(W)]).astype(np.int32)
    gkw = dict(panel=inp["panel"], start=None, row_idx=rows, col_idx=cols, n_r=n_r,
               n_rows=rng.integers(n_r - 9, n_r + 1, W).astype(np.int32), rf_adj=rng.normal(1e-4, 3e-5, size=(W, n_r)))
    refg, rstatg, _ = oracle.posterior_batch_c("jeffreys", k, N, 5.0, **gkw)
    wg, sg, _ = native.posterior_batch("jeffreys", k, N, 5.0, **gkw)
    assert (sg == rstatg).all() and (rstatg == 0).all()
    np.testing.assert_allclose(wg, refg, **WTOL)
    # contiguous windows with ragged row counts and an adjustment (no sharing: rf_adj), and with the shift d I + e 1 1'
    ckw = dict(panel=dense, start=inp["start"], n_r=n_r, n_rows=gkw["n_rows"], rf_adj=gkw["rf_adj"])
    refc, _, _ = oracle.posterior_batch_c("jeffreys", k, N, 5.0, **ckw)
    wc, sc, _ = native.posterior_batch("jeffreys", k, N, 5.0, **ckw)
    assert (sc == 0).all()
    np.testing.assert_allclose(wc, refc, **WTOL)
    shift = np.column_stack([rng.gamma(1.0, 5.0, W), rng.uniform(0, 20.0, W)])
    refs, _, _ = oracle.posterior_batch("jeffreys", k, N, 5.0, **kw, shift=shift)
    ws, ss, _ = native.posterior_batch("jeffreys", k, N, 5.0, **kw, shift=shift)
    assert (ss == 0).all()
    np.testing.assert_allclose(ws, refs, rtol=0, atol=1e-10 * max(1.0, np.abs(refs).max()))


@pytest.mark.parametrize("k,N,hf_days,W", [(260, 300, 3, 40), (383, 250, 5, 36), (500, 250, 5, 48), (1000, 500, 22, 40)])
def test_shared_intraday_sums_on_the_large_k_path(native, k, N, hf_days, W):
    """Conjugate windows whose intraday rows advance by one day per date: the whole days of every window come from block Grams
    the windows of a sub-batch share (posterior_tiled_wave.h, tiled_gram_wave_hfs_kernel), the centring is a rank-one term
    and c S0 w0 is assembled from the super-tiles' pieces.  Against the oracle (flat 1e-10, aux 1e-11), against the same
    batch with every row through the MFMAs (TP_FLAG_NO_SHARED_GRAM), and bit-identical for a sub-batch."""
    inp = synthetic.make_kernel_inputs(k, N, W, seed=5200 + k, hf_days=hf_days)
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"],
              m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    dev = native.default_device()
    dev.set_option("hf_share_min_blocks", 2)                # (default 6: below that the tables cost what they save)
    try:
        wts, status, aux = native.posterior_batch("conjugate", k, N, 5.0, **kw)
        part = {key: (val[W // 3:] if key in ("start", "hf_start", "w0", "n0") else val) for key, val in kw.items()}
        wp, _, _ = native.posterior_batch("conjugate", k, N, 5.0, **part)
    finally:
        dev.set_option("hf_share_min_blocks", 6)
    plain, pstat, paux = native.posterior_batch("conjugate", k, N, 5.0, flags=native.FLAG_NO_SHARED_GRAM, **kw)
    assert (status == 0).all() and (pstat == 0).all()
    np.testing.assert_allclose(wts, plain, rtol=0, atol=1e-12 * max(1.0, np.abs(plain).max()))
    np.testing.assert_allclose(aux[:, :6], paux[:, :6], rtol=1e-11, atol=1e-14)
    assert not np.array_equal(wts, plain)                   # (the two forms round differently: the shared path did run)
    sel = np.array([0, 1, W // 2, W - 1])
    sub = {key: (val[sel] if key in ("start", "hf_start", "w0", "n0") else val) for key, val in kw.items()}
    ref, rstat, raux = oracle.posterior_batch_c("conjugate", k, N, 5.0, **sub)
    np.testing.assert_allclose(wts[sel], ref, **WTOL)
    np.testing.assert_allclose(aux[sel, :6], raux[:, :6], rtol=1e-11, atol=1e-14)
    assert np.array_equal(wp, wts[W // 3:])


def test_a_non_finite_intraday_row_poisons_only_the_windows_that_contain_it(native):
    """Shared intraday sums are additions only: a NaN bar return makes the block Gram of ITS day NaN and with it the sums of
    the windows that contain that day - the other windows come out bit-identical to the clean run."""
    k, N, hf_days, W = 260, 300, 8, 30                      # 7 whole days per window: shared by default
    inp = synthetic.make_kernel_inputs(k, N, W, seed=6100, hf_days=hf_days)
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"],
              m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    clean, cstat, _ = native.posterior_batch("conjugate", k, N, 5.0, **kw)
    assert (cstat == 0).all()
    plain, _, _ = native.posterior_batch("conjugate", k, N, 5.0, flags=native.FLAG_NO_SHARED_GRAM, **kw)
    assert not np.array_equal(clean, plain)                 # the shared path ran
    bad_row = 78 * 14 + 40
    hf = inp["hf_panel"].copy()
    hf[bad_row, 17] = np.nan
    got, status, _ = native.posterior_batch("conjugate", k, N, 5.0, **dict(kw, hf_panel=hf))
    inside = (inp["hf_start"] <= bad_row) & (bad_row < inp["hf_start"] + inp["m"])
    assert inside.any() and (~inside).any()
    assert (status[inside] != 0).all()
    assert (status[~inside] == 0).all()
    assert np.array_equal(got[~inside], clean[~inside])


def test_shared_intraday_sums_with_a_large_common_offset(native):
    """The shared sums are raw second moments made central by a rank-one term; every row is taken relative to ONE reference
    row of the panel first, so an offset common to all returns (here 1.0 against a spread of 1e-3: a factor 1e6 between the
    raw and the central moments) costs no digits.  Flat 1e-10 against the oracle's two-pass form."""
    k, N, hf_days, W = 260, 300, 8, 24
    inp = synthetic.make_kernel_inputs(k, N, W, seed=6300, hf_days=hf_days)
    hf = inp["hf_panel"] + 1.0
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"], hf_panel=hf, hf_start=inp["hf_start"],
              m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    wts, status, aux = native.posterior_batch("conjugate", k, N, 5.0, **kw)
    plain, pstat, paux = native.posterior_batch("conjugate", k, N, 5.0, flags=native.FLAG_NO_SHARED_GRAM, **kw)
    assert (status == 0).all() and (pstat == 0).all() and not np.array_equal(wts, plain)
    sel = np.array([0, 5, W - 1])
    sub = {key: (val[sel] if key in ("start", "hf_start", "w0", "n0") else val) for key, val in kw.items()}
    ref, rstat, raux = oracle.posterior_batch_c("conjugate", k, N, 5.0, **sub)
    np.testing.assert_allclose(plain[sel], ref, **WTOL)
    np.testing.assert_allclose(wts[sel], ref, **WTOL)
    np.testing.assert_allclose(aux[sel, :6], raux[:, :6], rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("strat,hf_days", [("conjugate", 8), ("conjugate", 2), ("jeffreys", 1)])
def test_large_k_tables_per_sub_batch_do_not_depend_on_the_cut(native, strat, hf_days):
    """The large-k path builds its shared tables (daily block-window sums, intraday block Grams) for the blocks of the
    sub-batch in flight.  A run cut into many small sub-batches (a 48 MiB arena: ~50 windows each) must give bit for bit what
    one sub-batch gives: block Grams depend on the panel only and the sums' groups are cut in absolute block positions."""
    k, N, W = 300, 700 if strat == "jeffreys" else 320, 230
    inp = synthetic.make_kernel_inputs(k, N, W, seed=6400 + hf_days, hf_days=hf_days)
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
    if strat == "conjugate":
        kw.update(hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    dev = native.default_device()
    one, s1, a1 = native.posterior_batch(strat, k, N, 5.0, **kw)
    dev.set_option("tiled_arena_mib", 48)
    try:
        b = dev.batch(strat, k, N, inp["n_r"], 5.0, W, inp["m"] if strat == "conjugate" else 0)
        try:
            b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
            b.run()
            cut, s2, a2 = b.download()
            assert dev.last_launch()["grid"] < W // 3           # several sub-batches
        finally:
            b.close()
    finally:
        dev.set_option("tiled_arena_mib", 0)
    assert (s1 == 0).all() and (s2 == 0).all()
    assert np.array_equal(one, cut) and np.array_equal(a1, a2)
    plain, _, _ = native.posterior_batch(strat, k, N, 5.0, flags=native.FLAG_NO_SHARED_GRAM, **kw)
    assert not np.array_equal(one, plain)                       # the shared tables were in use
    np.testing.assert_allclose(one, plain, rtol=0, atol=1e-12 * max(1.0, np.abs(plain).max()))
