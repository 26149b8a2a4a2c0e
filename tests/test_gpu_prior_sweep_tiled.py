"""Prior sweeps above sweep_max_assets() (tp_batch_prior_sweep_tiled / Batch.prior_sweep_tiled): P conjugate priors (n0, w0) per
window from one pair of Grams, factorised by the large-k tiled pipeline.  Checked against the oracle (oracle.posterior_batch
once per prior), against the run kernels, for independence of W / P / the prior's slot / the sub-ranges / the size of the tiled
workspace, statuses, that the batch is left alone, the contract, and the product path
(calculate_weights_for_specs(share_grams="any")).  -m gpu.

Shapes: k = 144 is the first size above the LDS solve core, 239 / 240 the two sides of the kernel-family boundary, NS = 3, 4, 5
super-tiles per side, and k = 191 puts the border column into a super-tile of its own (k + 1 = 192 = 3 x 64: NS = 4, NSB = 3).
Synthetic return panels: on them the raw-moment centring of the sweep's C moves the weights by less than 1e-3 of the tolerance
against the two-pass form (tools/prior_sweep_tiled_centring.py, profiles/r09_prior_sweep_tiled_centring.txt)."""
import numpy as np
import pandas as pd
import pytest

from incorporating_different_sources_amd import _native, synthetic
from oracle import oracle

from _tiled_sweep_cases import SCALINGS, layouts, make_priors

pytestmark = pytest.mark.gpu

GAMMA = 5.0
# the bound the project holds such solves to (tests/test_gpu_solve_sweep.py): atol = 1e-10 max(1, |ref|.max()), rtol = 0
TOL = 1e-10
SHAPES = [(144, 200), (191, 250), (239, 300), (240, 300), (300, 360)]


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


def assert_close(x, ref, tol=TOL, what=""):
    bound = tol * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(x - ref).max())
    print(f"{what}: max|sweep - ref| = {err:.3e} (bound {bound:.3e}, |ref|.max() = {np.abs(ref).max():.3e})")
    assert np.isfinite(x).all()
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def oracle_sweep(k, N, panel, okw, n0, w0):
    """oracle.posterior_batch once per prior -> (weights [W, P, k], aux [W, P, 8])."""
    W, P = n0.shape
    ref = np.empty((W, P, k))
    raux = np.zeros((W, P, 8))
    kw = {key: val for key, val in okw.items() if key not in ("w0", "n0")}
    for p in range(P):
        wts, status, aux = oracle.posterior_batch("conjugate", k, N, GAMMA, panel, w0=np.ascontiguousarray(w0[:, p]),
                                                  n0=np.ascontiguousarray(n0[:, p]), **kw)
        assert (status == 0).all()
        ref[:, p] = wts
        raux[:, p, :min(8, aux.shape[1])] = aux[:, :8]
    return ref, raux


def check_against_oracle(dev, k, N, W, P, seed, which, hf_index=False):
    inp = synthetic.make_kernel_inputs(k, N, W, seed=seed)
    n0, w0 = make_priors(np.random.default_rng(seed), W, P, k, N)
    seen = []
    for name, panel, ukw, okw in layouts(inp, seed, hf_index):
        if name not in which:
            continue
        seen.append(name)
        b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
        b.upload(panel, **ukw)
        wts, status, aux = b.prior_sweep_tiled(n0, w0)
        b.close()
        assert wts.shape == (W, P, k) and status.shape == (W, P) and aux.shape == (W, P, 8)
        assert (status == _native.STATUS_OK).all()
        ref, raux = oracle_sweep(k, N, panel, okw, n0, w0)
        assert_close(wts, ref, what=f"k={k} {name}")
        # aux: n0, n1, c, q0, q1, n1 - q1 at the tolerance of the run kernels' aux against the oracle (tests/test_gpu_parity.py)
        np.testing.assert_allclose(aux[..., :6], raux[..., :6], rtol=1e-11, atol=1e-14)
        assert np.array_equal(aux[..., 0], n0)
    assert seen == list(which)


# ---- 1. against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,N", SHAPES)
def test_tiled_prior_sweep_matches_oracle(dev, k, N):
    check_against_oracle(dev, k, N, 2, 4, 890000 + k, ("contiguous", "index"))


# ---- 2. per-window intraday row count --------------------------------------------------------------------------------
def test_tiled_prior_sweep_per_window_intraday_row_count(dev):
    """hf_row_idx with a different hf_count per window: m/(m-1) and the centring are the window's own."""
    check_against_oracle(dev, 150, 200, 2, 4, 890000 + 150, ("index+hf",), hf_index=True)


# ---- 3. against the run kernels ------------------------------------------------------------------------------------
def test_tiled_prior_sweep_agrees_with_run(dev):
    k, N, W, P = 240, 300, 3, 3
    inp = synthetic.make_kernel_inputs(k, N, W, seed=892000 + k)
    n0, w0 = make_priors(np.random.default_rng(892000 + k), W, P, k, N)
    n0[:, 1], w0[:, 1, :] = inp["n0"], inp["w0"]
    b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"], _native.FLAG_NO_SHARED_GRAM)
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    ref, rstat, raux = b.run().download()
    wts, status, aux = b.prior_sweep_tiled(n0, w0)
    b.close()
    assert (rstat == 0).all() and (status == 0).all()
    assert_close(wts[:, 1], ref, what=f"k={k} sweep vs run")
    np.testing.assert_allclose(aux[:, 1, :6], raux[:, :6], rtol=1e-11, atol=1e-14)


# ---- 4. independence ------------------------------------------------------------------------------------------------
def test_tiled_prior_sweep_is_independent_of_W_P_slot_and_chunking(dev):
    k, N, W, P = 160, 200, 5, 3
    inp = synthetic.make_kernel_inputs(k, N, W, seed=893000)
    n0, w0 = make_priors(np.random.default_rng(893000), W, P, k, N)
    up = dict(hf_panel=inp["hf_panel"])

    def sweep(windows, priors, chunk=0):
        dev.set_option("sweep_chunk_windows", chunk)
        try:
            ws = np.asarray(windows)
            b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, len(ws), inp["m"])
            b.upload(inp["panel"], start=inp["start"][ws], hf_start=inp["hf_start"][ws], w0=inp["w0"][ws], n0=inp["n0"][ws], **up)
            out = b.prior_sweep_tiled(n0[np.ix_(ws, priors)], w0[np.ix_(ws, priors)])
            b.close()
            return out
        finally:
            dev.set_option("sweep_chunk_windows", 0)

    full = sweep(range(W), list(range(P)))
    assert (full[1] == 0).all()
    one = sweep([3], list(range(P)))                       # W = 1 against 5
    for a, f in zip(one, full):
        assert np.array_equal(a[0], f[3])
    single = sweep(range(W), [2])                          # P = 1 against 3
    for a, f in zip(single, full):
        assert np.array_equal(a[:, 0], f[:, 2])
    moved = sweep(range(W), [2, 1, 0])                     # every prior but the middle one in another slot
    for a, f in zip(moved, full):
        assert np.array_equal(a[:, ::-1], f)
    cut = sweep(range(W), list(range(P)), chunk=1)         # sub-ranges of 1 window against automatic
    for a, f in zip(cut, full):
        assert np.array_equal(a, f)


# ---- 5. a tiled workspace smaller than the sub-range's (window, prior) pairs ------------------------------------------
def test_tiled_prior_sweep_is_independent_of_the_arena(dev):
    k, N, W, P = 300, 360, 3, 4
    inp = synthetic.make_kernel_inputs(k, N, W, seed=893500)
    n0, w0 = make_priors(np.random.default_rng(893500), W, P, k, N)

    def sweep(arena_mib):
        dev.set_option("tiled_arena_mib", arena_mib)
        try:
            b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
            b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
            out = b.prior_sweep_tiled(n0, w0)
            b.close()
            return out
        finally:
            dev.set_option("tiled_arena_mib", 0)

    full = sweep(0)                                        # all 12 pairs in the arena at once
    assert (full[1] == 0).all()
    for mib in (1, 5):                                     # one slot (about 1 MB each at k = 300); five: groups of 5, 5, 2
        cut = sweep(mib)
        for a, f in zip(cut, full):
            assert np.array_equal(a, f)


# ---- 6. statuses ----------------------------------------------------------------------------------------------------
def test_tiled_nan_row_flags_every_prior_of_its_window_only(dev):
    k, N, W, P = 150, 200, 3, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=894000)
    n0, w0 = make_priors(np.random.default_rng(894000), W, P, k, N)
    panel = inp["panel"].copy()
    row_idx = (inp["start"][:, None] + np.arange(inp["n_r"])[None, :]).astype(np.int32)
    row_idx[2, 7] = panel.shape[0]                         # window 2 alone reads the extra row
    panel = np.concatenate([panel, np.full((1, k), np.nan)], axis=0)
    b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
    b.upload(panel, row_idx=row_idx, hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    _, rstat, _ = b.run().download()
    wts, status, _ = b.prior_sweep_tiled(n0, w0)
    b.close()
    assert (status[2] != _native.STATUS_OK).all() and (status[2] == rstat[2]).all()     # as the tiled run reports it
    assert (np.delete(status, 2, axis=0) == _native.STATUS_OK).all() and np.isfinite(np.delete(wts, 2, axis=0)).all()


def test_tiled_duplicate_column_is_not_pd(dev):
    k, N, W, P = 150, 200, 3, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=894100)
    n0, w0 = make_priors(np.random.default_rng(894100), W, P, k, N)
    n0[:] = 1e-3
    col_idx = np.tile(np.arange(k, dtype=np.int32), (W, 1))
    col_idx[1, 70] = col_idx[1, 4]                         # window 1: a duplicate column in both panels -> singular S1
    b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
    b.upload(inp["panel"], row_idx=(inp["start"][:, None] + np.arange(inp["n_r"])[None, :]).astype(np.int32), col_idx=col_idx,
             hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    wts, status, _ = b.prior_sweep_tiled(n0, w0)
    b.close()
    assert (status[1] == _native.STATUS_NOT_PD).all(), status
    assert (status[[0, 2]] == _native.STATUS_OK).all()


# ---- 7. the batch is left alone -------------------------------------------------------------------------------------
def test_tiled_prior_sweep_leaves_the_batch_alone(dev):
    k, N, W, P = 150, 200, 3, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=895000)
    n0, w0 = make_priors(np.random.default_rng(895000), W, P, k, N)
    up = dict(start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
    b.upload(inp["panel"], **up)
    b.keep_rhs().keep_posterior()
    before = (*b.run().download(), b.download_rhs(), b.download_posterior(), dev.last_launch())
    swept = b.prior_sweep_tiled(n0, w0)
    after = (*b.download(), b.download_rhs(), b.download_posterior(), dev.last_launch())
    for x, y in zip(before[:5], after[:5]):
        assert np.array_equal(x, y)
    assert before[5] == after[5]
    rerun = (*b.run().download(), b.download_rhs(), b.download_posterior(), dev.last_launch())
    for x, y in zip(before[:5], rerun[:5]):
        assert np.array_equal(x, y)
    assert before[5] == rerun[5]
    again = b.prior_sweep_tiled(n0, w0)
    b.close()
    assert (swept[1] == 0).all()
    for x, y in zip(swept, again):
        assert np.array_equal(x, y)


def test_tiled_prior_sweep_is_one_timed_step(dev):
    k, N, W, P = 150, 200, 3, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=896100)
    n0, w0 = make_priors(np.random.default_rng(896100), W, P, k, N)
    b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    dev.set_option("sweep_chunk_windows", 2)               # two sub-ranges, still one step
    try:
        dev.region_begin()
        b.prior_sweep_tiled(n0, w0)
        dev.region_end()
    finally:
        dev.set_option("sweep_chunk_windows", 0)
    steps = dev.region_steps()
    b.close()
    assert len(steps) == 1 and steps[0] > 0 and dev.last_timing()["kernel_ms"] > 0


# ---- 8. the contract ------------------------------------------------------------------------------------------------
def test_tiled_prior_sweep_contract(dev):
    import ctypes
    k, N, W, P = 150, 200, 3, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=896000)
    n0, w0 = make_priors(np.random.default_rng(896000), W, P, k, N)
    lib = _native.lib
    pd_ = ctypes.POINTER(ctypes.c_double)
    ptr = lambda a: a.ctypes.data_as(pd_)

    def code(b, fn):
        with pytest.raises(_native.TangencyError) as e:
            fn(b)
        return e.value.code

    b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
    assert code(b, lambda b: b.prior_sweep_tiled(n0, w0)) == _native.TP_ERR_INVALID         # not uploaded
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    out = np.empty((W, P, k))
    assert lib.tp_batch_download_prior_sweep(b._b, ptr(out), None, None) == _native.TP_ERR_INVALID      # no sweep before it
    assert lib.tp_batch_prior_sweep_tiled(b._b, 0, ptr(n0), ptr(w0)) == _native.TP_ERR_INVALID          # n_prior < 1
    assert lib.tp_batch_prior_sweep_tiled(b._b, P, None, ptr(w0)) == _native.TP_ERR_INVALID             # NULL arrays
    assert lib.tp_batch_prior_sweep_tiled(b._b, P, ptr(n0), None) == _native.TP_ERR_INVALID
    for bad in (0.0, -1.0, np.nan, np.inf):
        n0b = n0.copy()
        n0b[1, 1] = bad
        assert code(b, lambda b: b.prior_sweep_tiled(n0b, w0)) == _native.TP_ERR_INVALID
    for bad in (np.nan, -np.inf):
        w0b = w0.copy()
        w0b[2, 0, 3] = bad
        assert code(b, lambda b: b.prior_sweep_tiled(n0, w0b)) == _native.TP_ERR_INVALID
    assert lib.tp_batch_download_prior_sweep(b._b, ptr(out), None, None) == _native.TP_ERR_INVALID      # still none that ran
    wts, status, _ = b.prior_sweep_tiled(n0, w0)                                            # the batch still works
    assert (status == 0).all()
    assert lib.tp_batch_download_prior_sweep(b._b, ptr(out), None, None) == 0 and np.array_equal(out, wts)
    b.close()

    j = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W, 0)
    j.upload(inp["panel"], start=inp["start"])
    assert code(j, lambda b: b.prior_sweep_tiled(n0, w0)) == _native.TP_ERR_INVALID         # a Jeffreys batch
    j.close()

    ks = 100                                                                                # tp_batch_prior_sweep's range
    assert ks <= _native.sweep_max_assets()
    small = synthetic.make_kernel_inputs(ks, ks + 20, 1, seed=896001)
    g = dev.batch("conjugate", ks, ks + 20, small["n_r"], GAMMA, 1, small["m"])
    g.upload(small["panel"], start=small["start"], hf_panel=small["hf_panel"], hf_start=small["hf_start"], w0=small["w0"], n0=small["n0"])
    assert code(g, lambda b: b.prior_sweep_tiled(small["n0"][:, None], small["w0"][:, None, :])) == _native.TP_ERR_UNSUPPORTED
    g.close()


# ---- 9. the product path --------------------------------------------------------------------------------------------
def _conj(strat, k, N, scaling, gamma):
    return {"weighting_strategy": strat, "size": k, "risk_aversion": gamma, "turnover_cost": 15,
            "rebalancing_frequency": "daily", "rolling_window": N, "rolling_window_frequency": "daily",
            "mcm_scaling": scaling, "display_name": f"{strat}_{scaling}"}


def test_share_grams_any_takes_the_tiled_sweep(monkeypatch):
    from incorporating_different_sources_amd import batch, portfolio_calculations as pc
    k, N = 150, 170
    assert k > _native.sweep_max_assets()
    md, _ = synthetic.make_market_data(n_tickers=k + 4, n_days=N + 30, seed=20240089)
    days = md["stock_prices_df"].index
    dates = [pd.Timestamp(d) for d in days[N + 5:N + 13]]
    names = ("conjugate_hf_vix_vw", "conjugate_hf_vix_ew", "conjugate_hf_epu_vw", "conjugate_hf_epu_ew")
    specs = [_conj(name, k, N, sc, 10 if (i + j) % 3 == 0 else 5) for i, name in enumerate(names) for j, sc in enumerate(SCALINGS[1:3])]
    assert len(dates) == 8 and len(specs) == 8
    batch.clear_panel_cache()
    plain = pc.calculate_weights_for_specs(dates, specs, md)
    tiled, small = [], []
    real_t, real_s = _native.Batch.prior_sweep_tiled, _native.Batch.prior_sweep
    monkeypatch.setattr(_native.Batch, "prior_sweep_tiled", lambda self, n0, w0, **kw: (tiled.append(n0.shape), real_t(self, n0, w0, **kw))[1])
    monkeypatch.setattr(_native.Batch, "prior_sweep", lambda self, n0, w0, **kw: (small.append(n0.shape), real_s(self, n0, w0, **kw))[1])
    batch.clear_panel_cache()
    same = pc.calculate_weights_for_specs(dates, specs, md, share_grams=True)
    assert tiled == [] and small == []                     # True above sweep_max_assets(): still the replicated batch
    for a, b in zip(plain, same):
        assert np.array_equal(a[0], b[0])
    batch.clear_panel_cache()
    shared = pc.calculate_weights_for_specs(dates, specs, md, share_grams="any")
    assert tiled == [(len(dates), len(specs))] and small == []     # ONE tiled sweep with P = len(specs)
    for sp, a, b in zip(specs, plain, shared):
        assert_close(b[0], a[0], what=f"k={k} {sp['display_name']} gamma={sp['risk_aversion']}")
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    batch.clear_panel_cache()
