"""Solve sweeps (tp_batch_solve_sweep / Batch.solve_sweep): S shifts x R right-hand sides per window from one Gram pass,
    x[w, s, r] = (M_w + d_ws I + e_ws 1 1')^-1 rhs_wr / gamma.
Checked against the oracle (Jeffreys: oracle.posterior_batch once per (s, r); conjugate: numpy.linalg.solve on the oracle's
S1), against the existing set_rhs + set_shift + run path, for independence of W / chunking / S, statuses, that the batch is
left alone, the contract, and the two strategies that use it.  -m gpu."""
import numpy as np
import pytest

from incorporating_different_sources_amd import _native, synthetic
from oracle import oracle

pytestmark = pytest.mark.gpu

GAMMA = 5.0
# the bound the project holds shifted solves to (tests/test_gpu_parity.py): atol = 1e-10 max(1, |ref|.max()), rtol = 0
TOL = 1e-10
SHAPES = [(3, 12), (10, 60), (33, 80), (50, 250), (100, 250), (143, 300)]


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


def make_shift(rng, W, S):
    """[W x S x 2]: shift 0 all-zero, d ~ Gamma(1, 10)/2, e ~ U(0, 50)."""
    sh = np.stack([rng.gamma(1.0, 10.0, size=(W, S)) / 2, rng.uniform(0.0, 50.0, size=(W, S))], axis=2)
    sh[:, 0, :] = 0.0
    return sh


def layouts(inp, seed):
    """(name, panel, upload kwargs, oracle kwargs) of the contiguous layout and of one with row_idx / n_rows / col_idx /
    rf_adj over a panel with 8 more columns to choose from."""
    k, W, n_r = inp["k"], inp["W"], inp["n_r"]
    cont = dict(start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    yield "contiguous", inp["panel"], cont, dict(cont, n_r=n_r, m=inp["m"])
    rng = np.random.default_rng(seed)
    P = np.concatenate([inp["panel"], rng.normal(0.0, 0.01, size=(inp["panel"].shape[0], 8))], axis=1)
    H = np.concatenate([inp["hf_panel"], rng.normal(0.0, 0.001, size=(inp["hf_panel"].shape[0], 8))], axis=1)
    col_idx = np.stack([rng.permutation(P.shape[1])[:k] for _ in range(W)]).astype(np.int32)
    row_idx = np.stack([inp["start"][w] + np.sort(rng.choice(n_r, n_r, replace=False)) for w in range(W)]).astype(np.int32)
    n_rows = rng.integers(max(k, n_r - 5), n_r + 1, size=W).astype(np.int32)
    rf_adj = rng.normal(0, 1e-4, size=(W, n_r))
    idx = dict(row_idx=row_idx, n_rows=n_rows, col_idx=col_idx, rf_adj=rf_adj, hf_panel=H, hf_start=inp["hf_start"],
               w0=inp["w0"], n0=inp["n0"])
    yield "index", P, idx, dict(idx, start=None, n_r=n_r, m=inp["m"])


def window_rows(panel, okw, k, w):
    """X of window w, sliced the way oracle.posterior_batch slices it."""
    nr = int(okw["n_rows"][w]) if okw.get("n_rows") is not None else okw["n_r"]
    rows = (np.asarray(okw["row_idx"][w][:nr], dtype=np.int64) if okw.get("row_idx") is not None
            else np.arange(okw["start"][w], okw["start"][w] + nr))
    cols = np.asarray(okw["col_idx"][w], dtype=np.int64) if okw.get("col_idx") is not None else np.arange(k)
    X = panel[np.ix_(rows, cols)]
    if okw.get("rf_adj") is not None:
        X = X - np.asarray(okw["rf_adj"][w][:nr])[:, None]
    return X, cols


def jeffreys_upload_kw(ukw):
    return {key: val for key, val in ukw.items() if key not in ("hf_panel", "hf_start", "w0", "n0")}


def jeffreys_reference(k, N, panel, okw, shift, rhs, no_center, default_rhs=True):
    """oracle.posterior_batch once per (s, r)."""
    W, S = shift.shape[:2]
    cols_rhs = ([None] if default_rhs else []) + [rhs[:, j, :] for j in range(rhs.shape[1])]
    ref = np.empty((W, S, len(cols_rhs), k))
    jkw = {key: val for key, val in okw.items() if key not in ("hf_panel", "hf_start", "w0", "n0", "m")}
    for s in range(S):
        for r, col in enumerate(cols_rhs):
            wts, status, _ = oracle.posterior_batch("jeffreys", k, N, GAMMA, panel, rhs=col, shift=shift[:, s, :],
                                                    no_center=no_center, **jkw)
            assert (status == 0).all()
            ref[:, s, r, :] = wts
    return ref


# ---- 1. against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,N", SHAPES)
@pytest.mark.parametrize("no_center", [True, False])
def test_jeffreys_sweep_matches_oracle(dev, k, N, no_center):
    W, S = 3, 5
    inp = synthetic.make_kernel_inputs(k, N, W, seed=770000 + k)
    rng = np.random.default_rng(770000 + k)
    shift = make_shift(rng, W, S)
    rhs = rng.normal(size=(W, 2, k))
    for name, panel, ukw, okw in layouts(inp, 770000 + k):
        b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W, 0, _native.FLAG_NO_CENTER if no_center else 0)
        b.upload(panel, **jeffreys_upload_kw(ukw))
        x, status = b.solve_sweep(shift=shift, rhs=rhs)
        b.close()
        assert x.shape == (W, S, 3, k) and status.shape == (W, S)
        assert (status == _native.STATUS_OK).all()
        assert_close(x, jeffreys_reference(k, N, panel, okw, shift, rhs, no_center), what=f"jeffreys k={k} {name}")


@pytest.mark.parametrize("k,N", SHAPES)
def test_conjugate_sweep_matches_numpy_solve_of_oracle_S1(dev, k, N):
    W = 3
    inp = synthetic.make_kernel_inputs(k, N, W, seed=770000 + k)
    rng = np.random.default_rng(770000 + k)
    rhs = rng.normal(size=(W, 2, k))
    for name, panel, ukw, okw in layouts(inp, 770000 + k):
        b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
        b.upload(panel, **ukw)
        x, status = b.solve_sweep(rhs=rhs)
        rhs0 = b.download_sweep_rhs()
        b.close()
        assert x.shape == (W, 1, 3, k) and (status == _native.STATUS_OK).all()
        ref = np.empty_like(x)
        for w in range(W):
            X, cols = window_rows(panel, okw, k, w)
            Y = okw["hf_panel"][np.ix_(np.arange(okw["hf_start"][w], okw["hf_start"][w] + inp["m"]), cols)]
            a = oracle.conjugate_window(X, Y, inp["w0"][w], float(inp["n0"][w]), N, k, GAMMA, return_aux=True)[1]
            b0 = a["c"] * (a["S0"] @ inp["w0"][w]) + a["t"]
            assert np.abs(rhs0[w] - b0).max() <= 1e-12 * max(1.0, np.abs(b0).max())
            for r, col in enumerate([b0, rhs[w, 0], rhs[w, 1]]):
                ref[w, 0, r] = np.linalg.solve(a["S1"], col) / GAMMA
        assert_close(x, ref, what=f"conjugate k={k} {name}")


# ---- 1b. the sizes it claims ----------------------------------------------------------------------------------------
def check_against_numpy_solve(dev, k, S, n_rhs, default_rhs, seed):
    """Jeffreys (default centring), N = 2 k + 24 rows, W = 2, shift 0 all-zero: x against numpy.linalg.solve of
    (T - t t'/N + d I + e 1 1') X = [t |] rhs, all columns at once, T and t from the oracle's statistics."""
    W, N = 2, max(2 * k + 24, 13)                          # (at least 12 rows per window)
    inp = synthetic.make_kernel_inputs(k, N, W, seed=seed)
    rng = np.random.default_rng(seed)
    shift = make_shift(rng, W, S)
    rhs = rng.normal(size=(W, n_rhs, k))
    b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W)
    b.upload(inp["panel"], start=inp["start"])
    x, status = b.solve_sweep(shift=shift, rhs=rhs, default_rhs=default_rhs)
    b.close()
    R = n_rhs + (1 if default_rhs else 0)
    assert x.shape == (W, S, R, k) and (status == _native.STATUS_OK).all(), status
    ref = np.empty_like(x)
    for w in range(W):
        X = inp["panel"][inp["start"][w]:inp["start"][w] + inp["n_r"]]
        T, t = oracle.canonical_statistics_T(X), oracle.canonical_statistics_t(X)
        B = np.column_stack(([t] if default_rhs else []) + [rhs[w, j] for j in range(n_rhs)])
        for s in range(S):
            M = T - np.outer(t, t) / N + shift[w, s, 0] * np.eye(k) + shift[w, s, 1] * np.ones((k, k))
            ref[w, s] = np.linalg.solve(M, B).T / GAMMA
    assert_close(x, ref, what=f"k={k} S={S} R={R}")


@pytest.mark.parametrize("k", [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 143])
def test_solve_sweep_edge_sizes(dev, k):
    """One and two assets, the tile edges of the Gram pass, the largest universe, and both sides of the sizes at which a lane
    of sweep_back_substitute takes another solution register (row i of lane i % 64 is register i / 64: k = 64 / 65, 128 / 129)."""
    check_against_numpy_solve(dev, k, 3, 2, True, 777000 + k)


@pytest.mark.parametrize("default_rhs", [True, False], ids=["default+15", "16"])
def test_solve_sweep_largest_launch(dev, default_rhs):
    """k = 143 with R = 16: the documented maximum, the largest packed triangle and the largest LDS image (98.3 KiB)."""
    check_against_numpy_solve(dev, _native.sweep_max_assets(), 2, 15 if default_rhs else 16, default_rhs, 778000)


# ---- 2. against the existing device path ----------------------------------------------------------------------------
@pytest.mark.parametrize("k,N", [(10, 60), (100, 250), (143, 300)])
def test_single_solve_equals_set_rhs_set_shift_run(dev, k, N):
    W = 6
    inp = synthetic.make_kernel_inputs(k, N, W, seed=771000 + k)
    rng = np.random.default_rng(771000 + k)
    shift = make_shift(rng, W, 2)[:, 1:, :]
    rhs = rng.normal(size=(W, 1, k))
    b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W, 0, _native.FLAG_NO_CENTER)
    b.upload(inp["panel"], start=inp["start"])
    x, status = b.solve_sweep(shift=shift, rhs=rhs, default_rhs=False)
    b.set_rhs(rhs[:, 0, :]).set_shift(shift[:, 0, :])
    wts, wstatus, _ = b.run().download(want_aux=False)
    b.close()
    assert x.shape == (W, 1, 1, k)
    assert (status[:, 0] == wstatus).all()
    assert_close(x[:, 0, 0, :], wts, tol=2e-10, what=f"sweep vs run k={k}")


# ---- 3. independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,N", [(20, 60), (100, 120)])
def test_results_do_not_depend_on_W_chunking_or_S(dev, k, N):
    W, S = 7, 5
    inp = synthetic.make_kernel_inputs(k, N, W, seed=772000 + k)
    rng = np.random.default_rng(772000 + k)
    shift = make_shift(rng, W, S)
    rhs = rng.normal(size=(W, 2, k))

    def sweep(windows, sh, chunk=0):
        dev.set_option("sweep_chunk_windows", chunk)
        try:
            b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, len(windows), 0, _native.FLAG_NO_CENTER)
            b.upload(inp["panel"], start=inp["start"][windows])
            out = b.solve_sweep(shift=sh[windows], rhs=rhs[windows])
            b.close()
            return out
        finally:
            dev.set_option("sweep_chunk_windows", 0)

    every = np.arange(W)
    x7, s7 = sweep(every, shift)
    x7c, s7c = sweep(every, shift, chunk=2)
    assert np.array_equal(x7, x7c) and np.array_equal(s7, s7c)
    for w in range(W):
        x1, s1 = sweep(np.array([w]), shift)
        assert np.array_equal(x1[0], x7[w]) and np.array_equal(s1[0], s7[w])
    for s in (0, 3):
        xs, ss = sweep(every, shift[:, s:s + 1, :])
        assert np.array_equal(xs[:, 0], x7[:, s]) and np.array_equal(ss[:, 0], s7[:, s])


# ---- 4. status ------------------------------------------------------------------------------------------------------
def test_zero_column_is_not_pd_unshifted_and_solved_when_shifted(dev):
    k, N, W = 24, 60, 4
    inp = synthetic.make_kernel_inputs(k, N, W, seed=773000)
    panel = inp["panel"].copy()
    panel[:, 5] = 0.0                                   # T has a zero row and column: the pivot is exactly 0
    shift = np.tile(np.array([[0.0, 0.0], [0.5, 0.0], [0.0, 3.0]]), (W, 1, 1))
    rhs = np.random.default_rng(773000).normal(size=(W, 1, k))
    b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W, 0, _native.FLAG_NO_CENTER)
    b.upload(panel, start=inp["start"])
    x, status = b.solve_sweep(shift=shift, rhs=rhs)
    b.close()
    assert (status[:, 0] == _native.STATUS_NOT_PD).all()
    assert (status[:, 1:] == _native.STATUS_OK).all()
    ref = np.empty((W, 2, 2, k))
    for w in range(W):
        X = panel[inp["start"][w]:inp["start"][w] + inp["n_r"]]
        T, t = X.T @ X, X.sum(axis=0)
        for s in (1, 2):
            M = T + shift[w, s, 0] * np.eye(k) + shift[w, s, 1] * np.ones((k, k))
            ref[w, s - 1, 0] = np.linalg.solve(M, t) / GAMMA
            ref[w, s - 1, 1] = np.linalg.solve(M, rhs[w, 0]) / GAMMA
    assert_close(x[:, 1:], ref, what="zero column, shifted")


def test_nan_row_marks_exactly_the_windows_that_contain_it(dev):
    k, N, W, S = 30, 40, 12, 3
    inp = synthetic.make_kernel_inputs(k, N, W, seed=773100)
    rng = np.random.default_rng(773100)
    shift = make_shift(rng, W, S)
    rhs = rng.normal(size=(W, 1, k))

    def sweep(panel):
        b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W, 0, _native.FLAG_NO_CENTER)
        b.upload(panel, start=inp["start"])
        out = b.solve_sweep(shift=shift, rhs=rhs)
        b.close()
        return out

    x_clean, s_clean = sweep(inp["panel"])
    assert (s_clean == _native.STATUS_OK).all()
    r = inp["n_r"] + 3
    panel = inp["panel"].copy()
    panel[r, 2] = np.nan
    x, status = sweep(panel)
    hit = (inp["start"] <= r) & (r < inp["start"] + inp["n_r"])
    assert hit.any() and not hit.all()
    assert (status[hit] == _native.STATUS_NONFINITE).all()
    assert not np.isfinite(x[hit]).all(axis=3).any()            # every (s, r) of those windows
    assert np.array_equal(status[~hit], s_clean[~hit]) and np.array_equal(x[~hit], x_clean[~hit])


# ---- 5. the batch is left alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_sweep_leaves_the_batch_alone(dev, strategy):
    k, N, W = 40, 120, 9
    inp = synthetic.make_kernel_inputs(k, N, W, seed=774000)
    rng = np.random.default_rng(774000)
    b = dev.batch(strategy, k, N, inp["n_r"], GAMMA, W, inp["m"])
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    b.set_rhs(rng.normal(size=(W, k)))
    if strategy == "jeffreys":
        b.set_shift(make_shift(rng, W, 2)[:, 1, :])
    b.keep_posterior(2, 5).keep_rhs().run()
    before = (*b.download(), b.download_posterior(), b.download_rhs())
    launch = dev.last_launch()
    b.solve_sweep(shift=make_shift(rng, W, 3) if strategy == "jeffreys" else None, rhs=rng.normal(size=(W, 2, k)))
    after = (*b.download(), b.download_posterior(), b.download_rhs())
    for x, y in zip(before, after):
        assert np.array_equal(x, y, equal_nan=True)
    b.run()
    assert dev.last_launch() == launch
    again = (*b.download(), b.download_posterior(), b.download_rhs())
    for x, y in zip(before, again):
        assert np.array_equal(x, y, equal_nan=True)
    b.close()


def test_kernel_ms_covers_the_sweep(dev):
    """kernel_ms spans the Gram pass AND the solves: it exceeds the time of the Gram pass alone - a plain run of the same
    batch on the same kernel (kept right-hand side and matrices, no shared sums) - whose work the sweep contains, next
    to 64 x 200 factorisations.  Inside a region the sweep is one step."""
    k, N, W, S = 50, 250, 64, 200
    inp = synthetic.make_kernel_inputs(k, N, W, seed=774100)
    b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W, 0, _native.FLAG_NO_CENTER | _native.FLAG_NO_SHARED_GRAM)
    b.upload(inp["panel"], start=inp["start"])
    shift = make_shift(np.random.default_rng(1), W, S)
    run_ms, sweep_ms = [], []
    b.keep_rhs().keep_posterior()
    for _ in range(3):
        b.run().download()
        run_ms.append(dev.last_timing()["kernel_ms"])
        b.solve_sweep(shift=shift, rhs=np.ones((W, 1, k)))
        sweep_ms.append(dev.last_timing()["kernel_ms"])
    print(f"run {run_ms} ms, sweep {sweep_ms} ms")
    assert min(run_ms) > 0.0 and min(sweep_ms) > min(run_ms)
    dev.region_begin()
    b.solve_sweep(shift=shift, rhs=np.ones((W, 1, k)))
    dev.region_end()
    steps = dev.region_steps()
    assert len(steps) == 1 and steps[0] > min(run_ms)
    b.close()


def test_greyserman_date_groups_do_not_change_results(monkeypatch):
    size, N = 10, 60
    pc, kw = _packed(size, N)
    rng = np.random.default_rng(776100)
    draws = (rng.uniform(-1000, 1000, size=(5, 40)), rng.gamma(1.0, 10.0, size=(5, 40)))
    whole = pc._greyserman_batch(kw, 5.0, size, N, draws=draws)
    monkeypatch.setattr(pc, "_GREYSERMAN_SWEEP_BYTES", 2 * 40 * 2 * size * 8)          # two dates per sweep
    assert np.array_equal(pc._greyserman_batch(kw, 5.0, size, N, draws=draws), whole)


# ---- 6. contract ----------------------------------------------------------------------------------------------------
def test_contract(dev):
    k, N, W = 12, 60, 4
    inp = synthetic.make_kernel_inputs(k, N, W, seed=775000)
    rng = np.random.default_rng(775000)

    def code(fn):
        with pytest.raises(_native.TangencyError) as e:
            fn()
        return e.value.code

    lib, c_double, c_int32 = _native.lib, _native.c_double, _native.c_int32
    b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W)
    x_buf, s_buf = np.empty((W, 1, 1, k)), np.empty((W, 1), dtype=np.int32)
    # not uploaded; download before any sweep
    assert code(lambda: b.solve_sweep()) == _native.TP_ERR_INVALID
    assert lib.tp_batch_download_sweep(b._b, _native._ptr(x_buf, c_double), _native._ptr(s_buf, c_int32)) == _native.TP_ERR_INVALID
    b.upload(inp["panel"], start=inp["start"])
    assert lib.tp_batch_download_sweep(b._b, _native._ptr(x_buf, c_double), _native._ptr(s_buf, c_int32)) == _native.TP_ERR_INVALID
    assert code(lambda: b.download_sweep_rhs()) == _native.TP_ERR_INVALID
    # negative shift values, n_shift < 0, R outside [1, 16]
    for bad in (-1e-3, np.nan):
        sh = make_shift(rng, W, 3)
        sh[2, 1, 1] = bad
        assert code(lambda: b.solve_sweep(shift=sh)) == _native.TP_ERR_INVALID
    sh = make_shift(rng, W, 3)
    assert lib.tp_batch_solve_sweep(b._b, -1, _native._ptr(sh, c_double), 0, None, 1) == _native.TP_ERR_INVALID
    assert lib.tp_batch_solve_sweep(b._b, 0, None, 0, None, 0) == _native.TP_ERR_INVALID           # R = 0
    r17 = rng.normal(size=(W, 17, k))
    assert lib.tp_batch_solve_sweep(b._b, 0, None, 17, _native._ptr(r17, c_double), 0) == _native.TP_ERR_INVALID
    assert lib.tp_batch_solve_sweep(b._b, 0, None, 16, _native._ptr(r17, c_double), 1) == _native.TP_ERR_INVALID
    assert lib.tp_batch_solve_sweep(b._b, 0, None, 2, None, 1) == _native.TP_ERR_INVALID           # n_rhs without rhs
    assert lib.tp_batch_solve_sweep(None, 0, None, 0, None, 1) == _native.TP_ERR_INVALID
    assert lib.tp_batch_download_sweep(None, None, None) == _native.TP_ERR_INVALID
    with pytest.raises(ValueError):
        b.solve_sweep(rhs=r17, default_rhs=False)
    with pytest.raises(ValueError):
        b.solve_sweep(rhs=rng.normal(size=(W, 2, k + 1)))
    with pytest.raises(ValueError):
        b.solve_sweep(shift=np.zeros((W, 3)))
    with pytest.raises(ValueError):
        b.solve_sweep(shift=np.zeros((W + 1, 3, 2)))
    with pytest.raises(ValueError):
        b.solve_sweep(out=(np.empty((W, 1, 2, k)), np.empty((W, 1), dtype=np.int32)))
    # R = 16 works (15 columns behind the default, and 16 without it), into pinned arrays
    r16 = rng.normal(size=(W, 16, k))
    out = (_native.pinned_empty((W, 3, 16, k)), _native.pinned_empty((W, 3), np.int32))
    x, status = b.solve_sweep(shift=sh, rhs=r16[:, :15], out=out)
    assert x is out[0] and status is out[1] and (status == 0).all()
    x2, _ = b.solve_sweep(shift=sh, rhs=r16, default_rhs=False)
    assert np.array_equal(x2[:, :, :15], x[:, :, 1:])
    X = inp["panel"][inp["start"][1]:inp["start"][1] + inp["n_r"]]
    t = X.sum(axis=0)
    M = X.T @ X - np.outer(t, t) / N + sh[1, 2, 0] * np.eye(k) + sh[1, 2, 1] * np.ones((k, k))
    assert_close(x2[1, 2], np.linalg.solve(M, r16[1].T).T / GAMMA, what="R = 16")
    assert np.abs(b.download_sweep_rhs()[1] - t).max() <= 1e-13
    b.close()
    # a shift on a conjugate batch
    c = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
    c.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    with pytest.raises(_native.TangencyError) as e:
        c.solve_sweep(shift=np.zeros((W, 1, 2)))
    assert e.value.code == _native.TP_ERR_INVALID and "Jeffreys strategy only" in str(e.value)
    c.close()
    # k above the sweep kernel's range
    kmax = _native.sweep_max_assets()
    assert 143 <= kmax <= _native.max_assets()
    if kmax < _native.max_assets():
        big = synthetic.make_kernel_inputs(kmax + 1, 200, 2, seed=775001)
        g = dev.batch("jeffreys", kmax + 1, 200, big["n_r"], GAMMA, 2)
        g.upload(big["panel"], start=big["start"])
        assert code(lambda: g.solve_sweep()) == _native.TP_ERR_UNSUPPORTED
        g.close()
    with pytest.raises(_native.TangencyError):
        dev.set_option("sweep_chunk_windows", -1)


# ---- 7. strategies --------------------------------------------------------------------------------------------------
def _spec(strat, size, N):
    return {"weighting_strategy": strat, "size": size, "risk_aversion": 5, "turnover_cost": 15,
            "rebalancing_frequency": "daily", "rolling_window": N, "rolling_window_frequency": "daily",
            "mcm_scaling": None, "display_name": strat}


def _packed(size, N):
    from incorporating_different_sources_amd import batch, portfolio_calculations as pc
    md, _ = synthetic.make_market_data(n_tickers=size + 4, n_days=N + 40, seed=20240077)
    days = md["stock_prices_df"].index
    dates = list(days[N + 5::7])[:5]
    assert len(dates) == 5
    kw, _ = batch.pack_windows(dates, _spec("jeffreys", size, N), md, members_of=pc._members_provider(md))
    return pc, kw


def _one_date(kw, i):
    per_window = ("start", "row_idx", "n_rows", "col_idx", "rf_adj")
    return {key: (np.asarray(val)[i:i + 1] if key in per_window and val is not None else val) for key, val in kw.items()}


def test_greyserman_batch_equals_single_dates():
    size, N = 10, 60
    pc, kw = _packed(size, N)
    rng = np.random.default_rng(776000)
    draws = (rng.uniform(-1000, 1000, size=(5, 40)), rng.gamma(1.0, 10.0, size=(5, 40)))
    both = pc._greyserman_batch(kw, 5.0, size, N, draws=draws)
    assert both.shape == (5, size) and np.isfinite(both).all()
    for i in range(5):
        one = pc._greyserman_batch(_one_date(kw, i), 5.0, size, N, draws=(draws[0][i:i + 1], draws[1][i:i + 1]))
        assert np.array_equal(one[0], both[i])


def test_jorion_batch_equals_single_dates():
    size, N = 10, 60
    pc, kw = _packed(size, N)
    kw.pop("start", None)
    both = pc._jorion_batch(kw, 5.0, size, N)
    assert both.shape == (5, size) and np.isfinite(both).all()
    for i in range(5):
        one = pc._jorion_batch(_one_date(kw, i), 5.0, size, N)
        assert np.array_equal(one[0], both[i])
