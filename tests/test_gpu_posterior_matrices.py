"""Kept posterior scale matrices (tp_batch_keep_posterior / Batch.keep_posterior): S1 (ref:358) or J (ref:600-601) of
every window, stored by the run's own kernels.  Checked against the oracle's per-window functions on every kernel
family, against the reference's goldens, and for the contract (symmetry, ranges, no change to anything else).  -m gpu."""
import os

import numpy as np
import pytest

from incorporating_different_sources_amd import _native, synthetic
from oracle import oracle

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 1e-11


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


@pytest.fixture
def opts(dev):
    names = []

    def set_(name, value):
        names.append(name)
        dev.set_option(name, int(value))
    yield set_
    for n in names:
        dev.set_option(n, 0 if n in ("tiled_arena_mib", "no_shared_gram") else -1)


def _kw(inp):
    return dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"],
                m=inp["m"], w0=inp["w0"], n0=inp["n0"])


def oracle_mats(strategy, k, N, panel, start=None, n_r=None, hf_panel=None, hf_start=None, m=None, w0=None, n0=None,
                row_idx=None, n_rows=None, col_idx=None, rf_adj=None, windows=None, shift=None, ret_pairs=None,
                hf_ret_pairs=None, **_):
    """S1 / J of each window, sliced the way oracle.posterior_batch slices them (price panels through its front-end)."""
    W = len(start) if start is not None else len(row_idx)
    if ret_pairs is not None:
        panel = oracle.log_return_rows(panel, *ret_pairs)
    if hf_ret_pairs is not None:
        hf_panel = oracle.log_return_rows(hf_panel, *hf_ret_pairs)
    out = []
    for w in (range(W) if windows is None else windows):
        nr = int(n_rows[w]) if n_rows is not None else n_r
        rows = np.asarray(row_idx[w][:nr], dtype=np.int64) if row_idx is not None else np.arange(start[w], start[w] + nr)
        cols = np.asarray(col_idx[w], dtype=np.int64) if col_idx is not None else np.arange(k)
        X = panel[np.ix_(rows, cols)]
        if rf_adj is not None:
            X = X - np.asarray(rf_adj[w][:nr])[:, None]
        with np.errstate(all="ignore"):
            if strategy == "conjugate":
                Y = hf_panel[np.ix_(np.arange(hf_start[w], hf_start[w] + m), cols)]
                out.append(oracle.conjugate_window(X, Y, w0[w], float(n0[w]), N, k, 1.0, return_aux=True)[1]["S1"])
            else:
                try:
                    J = oracle.jeffreys_window(X, N, 1.0, return_aux=True)[1]["J"]
                except np.linalg.LinAlgError:        # exactly singular (the solve, not J, fails)
                    t = oracle.canonical_statistics_t(X)
                    J = oracle.canonical_statistics_T(X) - 1 / N * np.outer(t, t)
                if shift is not None:
                    J = J + shift[w][0] * np.eye(k) + shift[w][1] * np.ones((k, k))
                out.append(J)
    return np.stack(out)


def run_keep(dev, strategy, inp, begin=0, count=None, flags=0, upload_kw=None):
    k, N = inp["k"], inp["N"]
    b = dev.batch(strategy, k, N, inp["n_r"], 5.0, inp["W"], inp["m"], flags)
    b.upload(inp["panel"], **(upload_kw or dict(start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"],
                                                w0=inp["w0"], n0=inp["n0"])))
    b.keep_posterior(begin, count)
    b.run()
    M = b.download_posterior()
    res = b.download()
    return b, M, res


def assert_close(M, ref):
    scale = np.abs(ref).max()
    err = np.abs(M - ref).max()
    assert err <= TOL * scale, f"max|kept - oracle| = {err:.3e} > {TOL} x {scale:.3e}"


# ---- 1. goldens of the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["single_k3_n12", "single_k10_n60", "single_k16_n40", "single_k33_n80", "single_k100_n250"])
@pytest.mark.parametrize("strat", ["conjugate_hf_vix_vw", "conjugate_hf_vix_ew"])
def test_kept_S1_matches_reference_goldens(dev, name, strat):
    """The reference's own S1 of each window (X, Y and the asset order as the reference saw them)."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    k, N, W = int(g["k"]), int(g["N"]), int(g["W"])
    n_r = N - 1
    m = g["w0_Y"].shape[0]
    b = dev.batch("conjugate", k, N, n_r, 5.0, W, m)
    b.upload(np.concatenate([g[f"w{w}_X"] for w in range(W)], axis=0), start=np.arange(W, dtype=np.int64) * n_r,
             hf_panel=np.concatenate([g[f"w{w}_Y"] for w in range(W)], axis=0), hf_start=np.arange(W, dtype=np.int64) * m,
             w0=np.stack([g[f"w{w}_{strat}_w0"] for w in range(W)]),
             n0=np.array([float(g[f"w{w}_{strat}_n0"]) for w in range(W)]),
             col_idx=np.stack([g[f"w{w}_{strat}_order"] for w in range(W)]).astype(np.int32))
    M = b.keep_posterior().run().download_posterior()
    b.close()
    for w in range(W):
        np.testing.assert_allclose(M[w], g[f"w{w}_{strat}_S1"], rtol=1e-11, atol=1e-16)


# ---- 2. every kernel family against the oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("k", [1, 15, 16, 17, 100, 143, 144, 191, 192, 239, 240, 300, 500, 1000])
def test_every_kernel_family_matches_oracle(dev, opts, strategy, k):
    W = 12 if k <= 239 else (5 if k <= 500 else 3)
    N = max(2 * k // 3, 30) if k > 100 else 60
    inp = synthetic.make_kernel_inputs(k, N, W, seed=7100 + k)
    ref = oracle_mats(strategy, **{**_kw(inp), "k": k, "N": N})
    if k <= 239:
        variants = [("wave_kernel", v) for v in (-1, 0, 1, 2)]
    else:
        variants = [("tiled_wave", -1), ("tiled_wave", 0), ("tiled_fuse", 0), ("tiled_fuse", 1), ("tiled_arena_mib", 1)]
    for name, value in variants:
        opts(name, value)
        b, M, _ = run_keep(dev, strategy, inp)
        b.close()
        assert_close(M, ref)
        opts(name, 0 if name == "tiled_arena_mib" else -1)


# ---- 3. layouts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("k", [100, 191])
def test_layouts(dev, strategy, k):
    W, N = 40, 120
    inp = synthetic.make_kernel_inputs(k, N, W, seed=7300 + k)
    kw = _kw(inp)
    ref = oracle_mats(strategy, **{**kw, "k": k, "N": N})
    b, M, _ = run_keep(dev, strategy, inp)
    assert b.shared_gram_blocks() > 0
    b.close()
    assert_close(M, ref)
    b, M, _ = run_keep(dev, strategy, inp, flags=_native.FLAG_NO_SHARED_GRAM)
    assert b.shared_gram_blocks() == 0
    b.close()
    assert_close(M, ref)
    # index layout: shuffled columns, row subsets, risk-free adjustment (8 more panel columns to choose from)
    rng = np.random.default_rng(k)
    n_r = inp["n_r"]
    P = np.concatenate([inp["panel"], rng.normal(0.0, 0.01, size=(inp["panel"].shape[0], 8))], axis=1)
    col_idx = np.stack([rng.permutation(P.shape[1])[:k] for _ in range(W)]).astype(np.int32)
    row_idx = np.stack([inp["start"][w] + np.sort(rng.choice(n_r, n_r, replace=False)) for w in range(W)]).astype(np.int32)
    n_rows = rng.integers(n_r - 5, n_r + 1, size=W).astype(np.int32)
    rf_adj = rng.normal(0, 1e-4, size=(W, n_r))
    up = dict(row_idx=row_idx, n_rows=n_rows, col_idx=col_idx, rf_adj=rf_adj, hf_panel=np.concatenate(
        [inp["hf_panel"], rng.normal(0.0, 0.001, size=(inp["hf_panel"].shape[0], 8))], axis=1), hf_start=inp["hf_start"],
        w0=inp["w0"], n0=inp["n0"])
    ref = oracle_mats(strategy, k, N, P, n_r=n_r, hf_panel=up["hf_panel"], hf_start=inp["hf_start"], m=inp["m"],
                      w0=inp["w0"], n0=inp["n0"], row_idx=row_idx, n_rows=n_rows, col_idx=col_idx, rf_adj=rf_adj)
    b = dev.batch(strategy, k, N, n_r, 5.0, W, inp["m"])
    b.upload(P, **up).keep_posterior().run()
    M = b.download_posterior()
    b.close()
    assert_close(M, ref)


def test_large_k_shared_intraday_blocks(dev):
    k, N, W = 500, 250, 48
    inp = synthetic.make_kernel_inputs(k, N, W, seed=7400, hf_days=8)
    b, M, _ = run_keep(dev, "conjugate", inp, begin=W - 4)
    assert b.shared_intraday_blocks() > 0
    b.close()
    assert_close(M, oracle_mats("conjugate", **{**_kw(inp), "k": k, "N": N}, windows=range(W - 4, W)))


# ---- 4. nothing else changes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("k,wave", [(100, -1), (191, -1), (100, 0), (500, -1)])
def test_keep_changes_nothing_else(dev, opts, strategy, k, wave):
    opts("wave_kernel", wave)
    inp = synthetic.make_kernel_inputs(k, 250 if k == 500 else 120, 16, seed=7500 + k)
    b = dev.batch(strategy, k, inp["N"], inp["n_r"], 5.0, inp["W"], inp["m"])
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    off = b.run().download()
    launch_off = dev.last_launch()
    b.keep_posterior().run()
    on = b.download()
    launch_on = dev.last_launch()
    b.keep_posterior(0, 0).run()
    off2 = b.download()
    b.close()
    for x, y, z in zip(off, on, off2):
        assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True)
    assert launch_on == launch_off


# ---- 5. contract ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 100, 191, 300])
def test_symmetry_and_middle_range(dev, k):
    W = 24
    inp = synthetic.make_kernel_inputs(k, max(120, k // 2), W, seed=7600 + k)
    b, M_all, _ = run_keep(dev, "conjugate", inp)
    b.close()
    assert np.array_equal(M_all, np.swapaxes(M_all, 1, 2))
    b, M, _ = run_keep(dev, "conjugate", inp, begin=7, count=5)
    assert M.shape == (5, k, k)
    assert np.array_equal(M, M_all[7:12])
    if k <= 239:
        for i, w in enumerate(range(7, 12)):
            S1, _ = b.download_matrix(w, "posterior")
            assert np.abs(M[i] - S1).max() <= 1e-12 * np.abs(S1).max()
    b.close()


def test_shifted_jeffreys_matches_readback(dev):
    k, N, W = 60, 120, 10
    inp = synthetic.make_kernel_inputs(k, N, W, seed=7700)
    shift = np.stack([np.linspace(0.0, 1e-3, W), np.linspace(1e-4, 0.0, W)], axis=1)
    b = dev.batch("jeffreys", k, N, inp["n_r"], 5.0, W)
    b.set_shift(shift)
    b.upload(inp["panel"], start=inp["start"]).keep_posterior().run()
    M = b.download_posterior()
    for w in range(W):
        J, _ = b.download_matrix(w, "posterior")
        assert np.abs(M[w] - J).max() <= 1e-12 * np.abs(J).max()
    b.close()
    assert_close(M, oracle_mats("jeffreys", k, N, inp["panel"], start=inp["start"], n_r=inp["n_r"], shift=shift))


@pytest.mark.parametrize("k", [40, 300])
def test_rank_deficient_and_nan_rows(dev, k):
    N = 30 if k == 40 else 200
    W = 12
    inp = synthetic.make_kernel_inputs(k, N, W, seed=7800 + k)
    b, M_clean, _ = run_keep(dev, "jeffreys", inp)
    b.close()
    # rank-deficient: fewer rows than assets (29 < 40, 199 < 300)
    b, M, (w, status, aux) = run_keep(dev, "jeffreys", inp)
    b.close()
    assert (status == _native.STATUS_NOT_PD).any()
    assert_close(M, oracle_mats("jeffreys", **{**_kw(inp), "k": k, "N": N}))
    # a NaN row changes only the windows that contain it
    r = inp["n_r"] + 3
    panel = inp["panel"].copy()
    panel[r, 2] = np.nan
    b, M_nan, _ = run_keep(dev, "jeffreys", dict(inp, panel=panel))
    b.close()
    hit = (inp["start"] <= r) & (r < inp["start"] + inp["n_r"])
    assert hit.any() and not hit.all()
    assert np.array_equal(M_nan[~hit], M_clean[~hit])
    assert np.isnan(M_nan[hit]).any(axis=(1, 2)).all()


def test_keep_zero_stops_and_errors(dev):
    k, N, W = 20, 60, 8
    inp = synthetic.make_kernel_inputs(k, N, W, seed=7900)
    b = dev.batch("conjugate", k, N, inp["n_r"], 5.0, W, inp["m"])
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    with pytest.raises(_native.TangencyError) as e:            # no keep
        b.download_posterior()
    assert e.value.code == _native.TP_ERR_INVALID
    b.keep_posterior()
    with pytest.raises(_native.TangencyError) as e:            # keep, but no run after it
        b.download_posterior()
    assert e.value.code == _native.TP_ERR_INVALID
    for begin, count in ((-1, 2), (0, W + 1), (W, 1), (3, -1)):
        with pytest.raises(_native.TangencyError) as e:
            b.keep_posterior(begin, count)
        assert e.value.code == _native.TP_ERR_INVALID
    b.keep_posterior(2, 3).run()
    with pytest.raises(ValueError):
        b.download_posterior(out=np.empty((3, k, k + 1)))
    with pytest.raises(ValueError):
        b.download_posterior(out=np.empty((3, k, k), dtype=np.float32))
    pinned = _native.pinned_empty((3, k, k))
    assert b.download_posterior(out=pinned) is pinned
    b.keep_posterior(0, 0).run()
    with pytest.raises(_native.TangencyError) as e:
        b.download_posterior()
    assert e.value.code == _native.TP_ERR_INVALID
    b.close()


def test_posterior_batch_want_posterior(dev):
    k, N, W = 30, 60, 6
    inp = synthetic.make_kernel_inputs(k, N, W, seed=7950)
    kw = _kw(inp)
    out = _native.posterior_batch("conjugate", k, N, 5.0, device=dev, want_posterior=True, **kw)
    assert len(out) == 4 and out[3].shape == (W, k, k)
    assert len(_native.posterior_batch("conjugate", k, N, 5.0, device=dev, **kw)) == 3
    assert_close(out[3], oracle_mats("conjugate", **{**kw, "k": k, "N": N}))


# ---- 6. boundary: the reference's call surface ----------------------------------------------------------------------
def _spec(strat, size, N, window_freq, rebal):
    return {"weighting_strategy": strat, "size": size, "risk_aversion": 5, "turnover_cost": 15,
            "rebalancing_frequency": rebal, "rolling_window": N, "rolling_window_frequency": window_freq,
            "mcm_scaling": None if strat == "jeffreys" else 1, "display_name": strat}


@pytest.mark.parametrize("name", ["backtest_k10_n60_daily", "backtest_shipped_k50_n250_weekly_monthly"])
def test_batch_matrices_match_per_date_helpers(name):
    from incorporating_different_sources_amd import batch, portfolio_calculations as pc
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    md, _ = synthetic.make_market_data(n_tickers=int(g["n_tickers"]), n_days=int(g["n_days"]), seed=int(g["seed"]),
                                       rf_nan_every=int(g["rf_nan_every"]))
    days = md["stock_prices_df"].index
    dates = list(days[int(g["start_idx"])::max(1, (len(days) - int(g["start_idx"])) // 6)])[:6]
    size, N = int(g["size"]), int(g["N"])
    spec = _spec("conjugate_hf_vix_vw", size, N, str(g["window_freq"]), str(g["rebal"]))
    frames = pc.calculate_posterior_scale_matrices_batch(dates, spec, md)
    weights = pc.calculate_portfolio_weights_batch(dates, spec, md)
    assert len(frames) == len(dates)
    for d, F, wdf in zip(dates, frames, weights):
        assert list(F.index) == list(wdf.index) and list(F.columns) == list(wdf.index)
        uni = pc._Universe(d, spec, md)
        ref = pc.calculate_conjugate_posterior_S(spec, d, uni.prices, uni.intraday, pc._mcm_frame(spec, d, md),
                                                 md["risk_free_rate_df"])
        ref = ref.loc[F.index, F.columns].to_numpy()
        assert np.abs(F.to_numpy() - ref).max() <= TOL * np.abs(ref).max()
    jspec = _spec("jeffreys", size, N, str(g["window_freq"]), str(g["rebal"]))
    frames = pc.calculate_posterior_scale_matrices_batch(dates, jspec, md)
    kw, labels = batch.pack_windows(dates, jspec, md, members_of=pc._members_provider(md))
    ref = oracle_mats("jeffreys", size, N, **kw)
    for i, F in enumerate(frames):
        assert list(F.index) == list(labels[i])
        assert np.abs(F.to_numpy() - ref[i]).max() <= TOL * np.abs(ref[i]).max()
