"""HIP path (through the C-ABI) against the CPU oracle and the reference's golden vectors.  -m gpu."""
import os

import numpy as np
import pytest

from oracle import oracle
from incorporating_different_sources_amd import synthetic

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# north_star: 1e-10 on the weights (fp64) - a FLAT absolute bound, no relative slack.  Observed on MI355X
# (tools/parity_report.py, 58 shapes, k = 1 .. 2047, both strategies): max |hip - oracle| = 6.1e-12 at k = 2047,
# <= 3.4e-13 everywhere else, 2.7e-14 at k = 100.
WTOL = dict(rtol=0, atol=1e-10)


@pytest.fixture(scope="module")
def native():
    from incorporating_different_sources_amd import _native
    return _native


def _golden_batch(name, strat):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    k, N, W = int(g["k"]), int(g["N"]), int(g["W"])
    n_r = N - 1
    kw = dict(panel=np.concatenate([g[f"w{w}_X"] for w in range(W)], axis=0),
              start=np.arange(W, dtype=np.int64) * n_r, n_r=n_r)
    if strat != "jeffreys":
        m = g["w0_Y"].shape[0]
        kw.update(hf_panel=np.concatenate([g[f"w{w}_Y"] for w in range(W)], axis=0),
                  hf_start=np.arange(W, dtype=np.int64) * m, m=m,
                  w0=np.stack([g[f"w{w}_{strat}_w0"] for w in range(W)]),
                  n0=np.array([float(g[f"w{w}_{strat}_n0"]) for w in range(W)]),
                  col_idx=np.stack([g[f"w{w}_{strat}_order"] for w in range(W)]).astype(np.int32))
    ref = np.stack([g[f"w{w}_{strat}_weights"] for w in range(W)])
    return g, k, N, kw, ref


SMALL = ["single_k3_n12", "single_k10_n60", "single_k16_n40", "single_k33_n80", "single_k100_n250"]


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("strat", ["conjugate_hf_vix_vw", "conjugate_hf_vix_ew", "jeffreys"])
def test_hip_matches_reference_golden(native, name, strat):
    g, k, N, kw, ref = _golden_batch(name, strat)
    s = "jeffreys" if strat == "jeffreys" else "conjugate"
    wts, status, aux = native.posterior_batch(s, k, N, 5.0, **kw)
    assert (status == 0).all(), status
    np.testing.assert_allclose(wts, ref, **WTOL)
    if s == "conjugate":
        W = len(ref)
        np.testing.assert_allclose(aux[:, 2], [float(g[f"w{w}_{strat}_c"]) for w in range(W)], rtol=1e-12)
        np.testing.assert_allclose(aux[:, 3], [float(g[f"w{w}_{strat}_q0"]) for w in range(W)], rtol=1e-11)
        np.testing.assert_allclose(aux[:, 4], [float(g[f"w{w}_{strat}_q1"]) for w in range(W)], rtol=1e-9)


@pytest.mark.parametrize("name", ["single_k10_n60", "single_k100_n250"])
def test_hip_S1_matches_reference(native, name):
    strat = "conjugate_hf_vix_vw"
    g, k, N, kw, ref = _golden_batch(name, strat)
    dev = native.default_device()
    n_r = kw.pop("n_r"); m = kw.pop("m")
    b = native.Batch(dev, "conjugate", k, N, n_r, 5.0, len(ref), m)
    b.upload(**kw)
    for w in range(len(ref)):
        S1 = b.download_S1(w)
        np.testing.assert_allclose(S1, g[f"w{w}_{strat}_S1"], rtol=1e-11, atol=1e-16)
    b.close()


@pytest.mark.parametrize("k,N,hf_days", [(1, 8, 1), (2, 9, 1), (7, 20, 1), (15, 40, 1), (16, 40, 1), (17, 60, 1),
                                          (31, 70, 1), (32, 70, 1), (47, 100, 1), (48, 120, 1), (64, 150, 1),
                                          (95, 200, 1), (96, 250, 1), (100, 250, 1), (111, 250, 1), (112, 250, 2),
                                          (128, 300, 2), (150, 320, 2), (191, 400, 3), (192, 400, 3), (200, 420, 3),
                                          (224, 460, 3), (239, 500, 4)])
@pytest.mark.parametrize("strat", ["conjugate", "jeffreys"])
def test_hip_matches_oracle_all_tile_shapes(native, k, N, hf_days, strat):
    """Every tile count 1..16 of the register-tile kernel, k on / next to tile edges."""
    W = 5
    inp = synthetic.make_kernel_inputs(k, N, W, seed=777000 + k, hf_days=hf_days)
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
    if strat == "conjugate":
        kw.update(hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    ref, rstat, raux = oracle.posterior_batch_c(strat, k, N, 5.0, **kw)
    wts, status, aux = native.posterior_batch(strat, k, N, 5.0, **kw)
    assert (status == rstat).all()
    scale = np.abs(ref).max()
    np.testing.assert_allclose(wts, ref, **WTOL)
    if strat == "conjugate":
        np.testing.assert_allclose(aux[:, :6], raux[:, :6], rtol=1e-11, atol=1e-14)


def test_rccl_gather_world_1(native):
    """The RCCL leg of the multi-GPU path with a one-rank communicator: ncclCommInitRank, the grouped
    gather of weights and statuses on the kernel's stream, and the host copy-out."""
    inp = synthetic.make_kernel_inputs(20, 50, 33, seed=99)
    dev = native.Device(0)
    try:
        dev.comm_init(native.Device.comm_unique_id(), 0, 1)
        b = dev.batch("conjugate", 20, 50, inp["n_r"], 5.0, 33, inp["m"])
        b.upload(panel=inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"],
                 w0=inp["w0"], n0=inp["n0"])
        b.run()
        wall, sall = b.gather(root=0)
        w, s, _ = b.download()
        assert wall.shape == (1, 33, 20) and np.array_equal(wall[0], w) and np.array_equal(sall[0], s)
        assert dev.last_timing()["gather_ms"] > 0
        b.close()
        dev.comm_destroy()
    finally:
        dev.close()


def test_rccl_gather_async_overlaps_and_orders(native):
    """tp_batch_gather_async on a one-rank communicator: several run + gather pairs queued without a host
    wait; each gather sees the snapshot of ITS run even though the next run rewrites the weights (the
    right-hand side changes between runs), and the last one is what download_gathered returns."""
    k, N, W = 20, 50, 200
    inp = synthetic.make_kernel_inputs(k, N, W, seed=98)
    dev = native.Device(0)
    try:
        dev.comm_init(native.Device.comm_unique_id(), 0, 1)
        b = dev.batch("jeffreys", k, N, inp["n_r"], 5.0, W, 0)
        b.upload(panel=inp["panel"], start=inp["start"])
        expect = None
        for i in range(4):
            b.set_rhs(np.full((W, k), float(i + 1)))
            b.run()
            b.gather_async(root=0)
        dev.synchronize()
        wall, sall = b.download_gathered()
        w, s, _ = b.download()
        assert np.array_equal(wall[0], w) and np.array_equal(sall[0], s)
        assert dev.last_timing()["gather_ms"] > 0
        # queued back to back WITHOUT set_rhs' host synchronisation in between: run(i+1) overwrites the weights
        # while gather(i) may still be in flight; linearity in the right-hand side identifies the snapshot
        b.set_rhs(np.full((W, k), 1.0)); b.run(); b.gather_async(root=0)
        first, _ = b.download_gathered()
        b.set_rhs(np.full((W, k), 3.0))
        b.run(); b.gather_async(root=0); b.run(); b.gather_async(root=0)
        last, _ = b.download_gathered()
        np.testing.assert_allclose(last[0], 3.0 * first[0], rtol=1e-11, atol=1e-12)   # 3x, not 1x: linear up to rounding
        b.close()
        dev.comm_destroy()
    finally:
        dev.close()


def test_status_codes(native):
    """Rank-deficient windows are flagged, not returned as garbage (Appendix B-Q8): Jeffreys with
    k > n_r - 1 has a singular J; a conjugate window with too few intraday returns likewise."""
    k, N = 40, 20          # n_r = 19 < k
    inp = synthetic.make_kernel_inputs(k, N, 3, seed=5)
    w, status, _ = native.posterior_batch("jeffreys", k, N, 5.0, panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
    assert (status != 0).all()
    # conjugate: rank(S1) <= (n_r) + (m - 1) = 19 + 9 < 40
    w, status, _ = native.posterior_batch("conjugate", k, N, 5.0, panel=inp["panel"], start=inp["start"], n_r=inp["n_r"],
                                          hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=10, w0=inp["w0"], n0=inp["n0"])
    assert (status != 0).all()


def test_invalid_inputs_are_rejected_on_the_host(native):
    inp = synthetic.make_kernel_inputs(8, 20, 4, seed=1)
    bad = inp["start"].copy(); bad[-1] = inp["panel"].shape[0]          # window runs off the panel
    with pytest.raises(native.TangencyError) as e:
        native.posterior_batch("jeffreys", 8, 20, 5.0, panel=inp["panel"], start=bad, n_r=inp["n_r"])
    assert e.value.code == native.TP_ERR_INVALID
    with pytest.raises(native.TangencyError) as e:                        # k beyond the largest supported universe
        native.posterior_batch("jeffreys", 2100, 30, 5.0, panel=np.zeros((30, 2100)), start=np.zeros(1, np.int64), n_r=29)
    assert e.value.code == native.TP_ERR_UNSUPPORTED
    col = np.tile(np.arange(8, dtype=np.int32), (4, 1)); col[0, 0] = 99
    with pytest.raises(native.TangencyError):
        native.posterior_batch("jeffreys", 8, 20, 5.0, panel=inp["panel"], start=inp["start"], n_r=inp["n_r"], col_idx=col)


def test_row_and_column_index_modes(native):
    """Explicit row lists (resampled / NaN-dropped windows), per-window row counts, column gathers and
    the per-row risk-free subtraction give what the dense equivalent gives."""
    rng = np.random.default_rng(3)
    k, N, W, Kall = 12, 30, 6, 20
    inp = synthetic.make_kernel_inputs(Kall, N, W, seed=8)
    n_r, m = inp["n_r"], inp["m"]
    cols = np.stack([rng.permutation(Kall)[:k] for _ in range(W)]).astype(np.int32)
    n_rows = rng.integers(n_r - 5, n_r + 1, size=W).astype(np.int32)
    rows = np.stack([np.sort(rng.choice(inp["panel"].shape[0], n_r, replace=False)) for _ in range(W)]).astype(np.int32)
    hf_count = rng.integers(m - 7, m + 1, size=W).astype(np.int32)
    hf_rows = np.stack([np.sort(rng.choice(inp["hf_panel"].shape[0], m, replace=False)) for _ in range(W)]).astype(np.int32)
    rf = rng.normal(0, 1e-4, size=(W, n_r))
    w0 = rng.uniform(0.5, 1.5, size=(W, k)); w0 /= w0.sum(axis=1, keepdims=True)
    kw = dict(panel=inp["panel"], start=None, n_r=n_r, row_idx=rows, n_rows=n_rows, col_idx=cols, rf_adj=rf,
              hf_panel=inp["hf_panel"], hf_start=None, hf_row_idx=hf_rows, hf_count=hf_count, m=m, w0=w0, n0=inp["n0"])
    ref, rstat, raux = oracle.posterior_batch("conjugate", k, N, 5.0, **kw)
    wts, status, aux = native.posterior_batch("conjugate", k, N, 5.0, **kw)
    assert (status == rstat).all()
    np.testing.assert_allclose(wts, ref, **WTOL)
    kwj = dict(panel=inp["panel"], start=None, n_r=n_r, row_idx=rows, n_rows=n_rows, col_idx=cols, rf_adj=rf)
    refj, _, _ = oracle.posterior_batch("jeffreys", k, N, 5.0, **kwj)
    wj, sj, _ = native.posterior_batch("jeffreys", k, N, 5.0, **kwj)
    np.testing.assert_allclose(wj, refj, **WTOL)


# ---------------------------------------------------------------------------------------------------
# large-k path (tiled pipeline, k >= 240): BASELINE configs[2] (k=500) and configs[4] (k=1000)
@pytest.mark.parametrize("name", ["single_k500_n250", "single_k1000_n500"])
@pytest.mark.parametrize("strat", ["conjugate_hf_vix_vw", "conjugate_hf_vix_ew"])
def test_tiled_path_matches_reference_golden(native, name, strat):
    """Outputs-only goldens of the unmodified reference at S&P500-sized universes; inputs regenerated
    from the seed and pushed through the same price round trip the reference saw."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    k, N, hf_days, seed = int(g["k"]), int(g["N"]), int(g["hf_days"]), int(g["seed"])
    inp = synthetic.make_kernel_inputs(k, N, 1, seed, hf_days=hf_days)
    n_r, m = inp["n_r"], inp["m"]
    P = 100.0 * np.exp(np.concatenate([np.zeros((1, k)), np.cumsum(inp["panel"][:n_r], axis=0)]))
    X = oracle.excess_log_returns_from_prices(P)
    H = 50.0 * np.exp(np.concatenate([np.zeros((1, k)), np.cumsum(inp["hf_panel"][:m], axis=0)]))
    Y = oracle.excess_log_returns_from_prices(H)
    order = g[f"w0_{strat}_order"].astype(np.int32)
    wts, status, aux = native.posterior_batch(
        "conjugate", k, N, 5.0, panel=X, start=np.zeros(1, np.int64), n_r=n_r, hf_panel=Y,
        hf_start=np.zeros(1, np.int64), m=m, w0=g[f"w0_{strat}_w0"][None, :],
        n0=np.array([float(g[f"w0_{strat}_n0"])]), col_idx=order[None, :])
    assert status[0] == 0
    np.testing.assert_allclose(wts[0], g[f"w0_{strat}_weights"], **WTOL)
    assert aux[0, 2] == pytest.approx(float(g[f"w0_{strat}_c"]), rel=1e-11)
    assert aux[0, 4] == pytest.approx(float(g[f"w0_{strat}_q1"]), rel=1e-8)


@pytest.mark.parametrize("k,N,hf_days,strat", [
    (240, 300, 2, "conjugate"), (255, 300, 2, "conjugate"), (256, 300, 2, "conjugate"), (300, 700, 1, "jeffreys"),
    (319, 250, 3, "conjugate"), (320, 250, 3, "conjugate"), (500, 250, 5, "conjugate"), (511, 260, 5, "conjugate"),
    (512, 1100, 1, "jeffreys"), (640, 400, 6, "conjugate"), (1000, 500, 22, "conjugate"),
    (2047, 300, 24, "conjugate")])      # tp_max_assets()
def test_tiled_path_matches_oracle(native, k, N, hf_days, strat):
    W = 3
    inp = synthetic.make_kernel_inputs(k, N, W, seed=880000 + k, hf_days=hf_days)
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
    if strat == "conjugate":
        kw.update(hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    ref, rstat, raux = oracle.posterior_batch_c(strat, k, N, 5.0, **kw)
    wts, status, aux = native.posterior_batch(strat, k, N, 5.0, **kw)
    assert (status == rstat).all()
    scale = max(1.0, np.abs(ref).max())
    np.testing.assert_allclose(wts, ref, **WTOL)
    if strat == "conjugate":
        np.testing.assert_allclose(aux[:, :6], raux[:, :6], rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("k,N", [(3, 12), (10, 60), (33, 80), (100, 250), (239, 300), (300, 400)])
def test_shift_and_plain_gram_match_oracle(native, k, N):
    """tp_batch_set_shift / TP_FLAG_NO_CENTER (the Greyserman scale matrix, ref:924): (T + d I + e 1 1')^-1 rhs
    and (T - t t'/N + d I + e 1 1')^-1 t on both the fused (k <= 239) and the tiled path."""
    W = 4
    inp = synthetic.make_kernel_inputs(k, N, W, seed=770000 + k)
    rng = np.random.default_rng(k)
    shift = np.column_stack([rng.gamma(1.0, 10.0, W) / 2, rng.uniform(0, 50.0, W)])
    shift[0] = (0.0, 0.0)
    rhs = rng.normal(size=(W, k))
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
    # plain Gram + shift, caller's right-hand side
    ref, rstat, _ = oracle.posterior_batch("jeffreys", k, N, 1.0, **kw, rhs=rhs, shift=shift, no_center=True)
    got, status, _ = native.posterior_batch("jeffreys", k, N, 1.0, **kw, rhs=rhs, shift=shift,
                                            flags=native.FLAG_NO_CENTER)
    assert (status == 0).all()
    # Not weights: solutions of (T + shift)^-1 rhs with a random right-hand side; window 0 has NO shift and T is close to
    # singular at k = 239 on 299 rows, so |x| reaches ~7e2 there.  The bound is the flat 1e-10 relative to the largest
    # entry (observed: 1.7e-13 relative, 1.1e-10 absolute at k = 239).
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * max(1.0, np.abs(ref).max()))
    # Jeffreys scatter + shift, default right-hand side t
    ref, rstat, _ = oracle.posterior_batch("jeffreys", k, N, 5.0, **kw, shift=shift)
    got, status, _ = native.posterior_batch("jeffreys", k, N, 5.0, **kw, shift=shift)
    assert (status == 0).all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * max(1.0, np.abs(ref).max()))


def test_shift_is_rejected_where_it_does_not_apply(native):
    inp = synthetic.make_kernel_inputs(5, 20, 2, seed=3)
    dev = native.default_device()
    b = native.Batch(dev, "conjugate", 5, 20, inp["n_r"], 5.0, 2, inp["m"])
    with pytest.raises(Exception, match="Jeffreys"):
        b.set_shift(np.ones((2, 2)))
    b.close()
    b = native.Batch(dev, "jeffreys", 5, 20, inp["n_r"], 5.0, 2, 0)
    with pytest.raises(Exception, match=">= 0"):
        b.set_shift(np.array([[1.0, -1.0], [0.0, 0.0]]))
    b.close()


def test_log_return_kernel_matches_numpy(native):
    """F4: the price front-end on its own (tp_log_returns) against numpy's log on the same row pairs, NaN /
    zero / negative prices included.  Both logarithms are within an ulp of the true value, not bit-equal."""
    rng = np.random.default_rng(42)
    rows, cols = 700, 133
    P = 100.0 * np.exp(np.cumsum(rng.normal(3e-4, 0.01, size=(rows, cols)), axis=0))
    P[5, 7] = np.nan; P[100:110, 0] = np.nan; P[300, 3] = 0.0; P[301, 4] = -1.0
    num = np.concatenate([np.arange(rows), rng.integers(0, rows, 500)]).astype(np.int32)
    den = np.concatenate([np.maximum(np.arange(rows) - 1, 0), rng.integers(0, rows, 500)]).astype(np.int32)
    got = native.default_device().log_returns(P, num, den)
    ref = oracle.log_return_rows(P, num, den)
    assert got.shape == ref.shape == (rows + 500, cols)
    assert np.array_equal(got == 0.0, ref == 0.0)                 # NaN -> 0 in the same places; exact zeros (p/p)
    assert np.array_equal(np.abs(got) > 1e300, np.abs(ref) > 1e300)   # +-inf -> +-DBL_MAX in the same places
    fin = np.abs(ref) < 1e300
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-15, atol=1e-18)
    with pytest.raises(Exception, match="outside the price panel"):
        native.default_device().log_returns(P, np.array([rows], np.int32), np.array([0], np.int32))


def _log_return_prices(rng, rows, cols):
    """A price panel with a NaN, a zero and a negative price (and a run of NaNs in the last column)."""
    P = 100.0 * np.exp(np.cumsum(rng.normal(3e-4, 0.01, size=(rows, cols)), axis=0))
    P[5, cols - 2] = np.nan; P[100:110, cols - 1] = np.nan; P[300, 3] = 0.0; P[301, 4] = -1.0
    return P


def _assert_log_returns_match_numpy(native, P, num, den):
    """The assertions of test_log_return_kernel_matches_numpy."""
    got = native.default_device().log_returns(P, num, den)
    ref = oracle.log_return_rows(P, num, den)
    assert got.shape == ref.shape == (len(num), P.shape[1])
    assert np.array_equal(got == 0.0, ref == 0.0)                 # NaN -> 0 in the same places; exact zeros (p/p)
    assert np.array_equal(np.abs(got) > 1e300, np.abs(ref) > 1e300)   # +-inf -> +-DBL_MAX in the same places
    fin = np.abs(ref) < 1e300
    assert (ref == 0.0).any() and (~fin).any()                    # the NaN, zero and negative prices are among the rows
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-15, atol=1e-18)


@pytest.mark.parametrize("cols", [1030, 1029])
def test_log_return_kernel_over_several_column_blocks(native, cols):
    """More than one x-block of 512 columns (three; the last one partly outside the panel, its idle lanes leave through the
    c >= ld guard): 1030 columns take the double2 form, 1029 the scalar form with the odd last column."""
    rng = np.random.default_rng(43 + cols)
    rows = 700
    P = _log_return_prices(rng, rows, cols)
    num = np.concatenate([np.arange(rows), rng.integers(0, rows, 100)]).astype(np.int32)
    den = np.concatenate([np.maximum(np.arange(rows) - 1, 0), rng.integers(0, rows, 100)]).astype(np.int32)
    _assert_log_returns_match_numpy(native, P, num, den)


def test_log_return_kernel_strides_over_more_rows_than_its_grid(native):
    """32,768 + 5 output rows from 700 price rows through repeated num / den: the grid holds 32,768 rows, the last five
    come from the second trip of the grid-stride loop."""
    rng = np.random.default_rng(44)
    rows, cols, n_out = 700, 6, 32768 + 5
    P = _log_return_prices(rng, rows, cols)
    num = np.concatenate([np.arange(rows), rng.integers(0, rows, n_out - rows)]).astype(np.int32)
    den = np.concatenate([np.maximum(np.arange(rows) - 1, 0), rng.integers(0, rows, n_out - rows)]).astype(np.int32)
    num[-5:], den[-5:] = [301, 300, 6, 5, 699], [300, 299, 5, 4, 0]      # the special prices in the second trip, too
    _assert_log_returns_match_numpy(native, P, num, den)


@pytest.mark.parametrize("k,N", [(10, 60), (100, 250), (300, 400)])
def test_price_front_end_matches_return_panels(native, k, N):
    """F4: prices + (numerator, denominator) rows into tp_batch_upload give the weights of the same windows
    fed as log-return panels (fused and tiled path), and the oracle's."""
    W = 6
    hf_days = 1 if k < 240 else 5
    inp = synthetic.make_kernel_inputs(k, N, W, seed=660000 + k, hf_days=hf_days)
    # prices whose consecutive log-returns are the synthetic panels (up to the rounding of exp / log)
    P = 100.0 * np.exp(np.concatenate([np.zeros((1, k)), np.cumsum(inp["panel"], axis=0)]))
    H = 50.0 * np.exp(np.concatenate([np.zeros((1, k)), np.cumsum(inp["hf_panel"], axis=0)]))
    pairs = lambda n: (np.arange(1, n, dtype=np.int32), np.arange(0, n - 1, dtype=np.int32))   # return row i: price i+1 / i
    common = dict(start=inp["start"], n_r=inp["n_r"], hf_start=inp["hf_start"], m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    got, status, aux = native.posterior_batch("conjugate", k, N, 5.0, panel=P, hf_panel=H, ret_pairs=pairs(len(P)),
                                              hf_ret_pairs=pairs(len(H)), **common)
    assert (status == 0).all()
    Lp, Lh = oracle.log_return_rows(P, *pairs(len(P))), oracle.log_return_rows(H, *pairs(len(H)))
    same, _, _ = native.posterior_batch("conjugate", k, N, 5.0, panel=Lp, hf_panel=Lh, **common)
    np.testing.assert_allclose(got, same, rtol=1e-9, atol=1e-11 * max(1.0, np.abs(same).max()))
    ref, _, _ = oracle.posterior_batch_c("conjugate", k, N, 5.0, panel=Lp, hf_panel=Lh, **common)
    np.testing.assert_allclose(got, ref, **WTOL)
    with pytest.raises(Exception, match="outside the panel"):      # windows are checked against the RETURN rows
        native.posterior_batch("conjugate", k, N, 5.0, panel=P, hf_panel=H, ret_pairs=(pairs(len(P))[0][:-3], pairs(len(P))[1][:-3]),
                               hf_ret_pairs=pairs(len(H)), **common)


@pytest.mark.parametrize("k,N", [(5, 20), (33, 80), (100, 250), (150, 200)])
@pytest.mark.parametrize("strat", ["conjugate", "jeffreys"])
def test_contiguous_layout_with_ragged_rows_and_risk_free_adjustment(native, k, N, strat):
    """The lean kernel (contiguous rows, ungathered columns) with everything that is optional in that layout:
    per-window row counts below n_r / m (ragged last chunk), and the per-row risk-free subtraction of ref:57."""
    W = 9
    inp = synthetic.make_kernel_inputs(k, N, W, seed=550000 + k)
    rng = np.random.default_rng(k)
    n_r, m = inp["n_r"], inp["m"]
    lo = max(k + 3, n_r - 20)            # Jeffreys needs more rows than assets (rank of T - t t'/N)
    n_rows = rng.integers(lo, n_r + 1, W).astype(np.int32); n_rows[0] = n_r; n_rows[1] = max(lo, n_r - 17)
    rf_adj = rng.normal(1e-4, 2e-5, size=(W, n_r))
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=n_r, n_rows=n_rows, rf_adj=rf_adj)
    if strat == "conjugate":
        hf_count = rng.integers(max(2, m - 30), m + 1, W).astype(np.int32); hf_count[0] = m
        kw.update(hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=m, hf_count=hf_count, w0=inp["w0"], n0=inp["n0"])
    ref, rstat, raux = oracle.posterior_batch(strat, k, N, 5.0, **kw)
    got, status, aux = native.posterior_batch(strat, k, N, 5.0, **kw)
    assert (status == rstat).all()
    np.testing.assert_allclose(got, ref, **WTOL)
    if strat == "conjugate":
        np.testing.assert_allclose(aux[:, :6], raux[:, :6], rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("k,N,hf_days", [(7, 30, 1), (31, 70, 1), (100, 250, 1), (130, 200, 2), (200, 250, 3), (239, 260, 4),
                                         (300, 320, 5)])
def test_layouts_are_bitwise_equivalent(native, k, N, hf_days):
    """The same windows through the contiguous layout (lean kernel) and through identity row / column index arrays
    plus a zero risk-free adjustment (generic kernel) give bit-identical weights: the two instantiations (and the
    tiled path's two Gram kernels) differ in addressing only, never in arithmetic or summation order - with the
    shared Gram prefixes of the contiguous layout switched off (TP_FLAG_NO_SHARED_GRAM).  With them on (the
    default for rolling windows over one panel) the daily Gram is summed block-wise: same numbers to a few ulps."""
    W = 24
    inp = synthetic.make_kernel_inputs(k, N, W, seed=440000 + k, hf_days=hf_days)
    n_r, m = inp["n_r"], inp["m"]
    base = dict(panel=inp["panel"], start=inp["start"], n_r=n_r, hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=m,
                w0=inp["w0"], n0=inp["n0"])
    rows = (inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32)
    hrows = (inp["hf_start"][:, None] + np.arange(m)[None, :]).astype(np.int32)
    idx = dict(panel=inp["panel"], start=None, n_r=n_r, row_idx=rows, col_idx=np.tile(np.arange(k, dtype=np.int32), (W, 1)),
               rf_adj=np.zeros((W, n_r)), hf_panel=inp["hf_panel"], hf_start=None, hf_row_idx=hrows, m=m, w0=inp["w0"], n0=inp["n0"])
    plain = native.FLAG_NO_SHARED_GRAM
    w1, s1, a1 = native.posterior_batch("conjugate", k, N, 5.0, flags=plain, **base)
    w2, s2, a2 = native.posterior_batch("conjugate", k, N, 5.0, **idx)
    assert (s1 == 0).all() and np.array_equal(s1, s2)
    assert np.array_equal(w1, w2) and np.array_equal(a1, a2)
    w3, s3, a3 = native.posterior_batch("conjugate", k, N, 5.0, **base)              # shared Gram prefixes (W n_r >= 3 rows)
    assert np.array_equal(s3, s1)
    np.testing.assert_allclose(w3, w1, rtol=0, atol=1e-12)
    np.testing.assert_allclose(a3, a1, rtol=1e-12, atol=1e-15)
    if k < n_r - 2:
        jkw = dict(panel=inp["panel"], start=inp["start"], n_r=n_r)
        j1, _, _ = native.posterior_batch("jeffreys", k, N, 5.0, flags=plain, **jkw)
        j2, _, _ = native.posterior_batch("jeffreys", k, N, 5.0, panel=inp["panel"], start=None, n_r=n_r, row_idx=rows,
                                          col_idx=idx["col_idx"], rf_adj=idx["rf_adj"])
        assert np.array_equal(j1, j2)
        j3, _, _ = native.posterior_batch("jeffreys", k, N, 5.0, **jkw)
        np.testing.assert_allclose(j3, j1, rtol=0, atol=1e-11 * max(1.0, np.abs(j1).max()))


@pytest.mark.parametrize("k,N,hf_days,strat,W", [(7, 600, 1, "conjugate", 450), (100, 250, 1, "conjugate", 300),
                                                 (130, 700, 2, "jeffreys", 50), (200, 1200, 3, "conjugate", 20),
                                                 (240, 300, 2, "conjugate", 40), (300, 700, 1, "jeffreys", 30),
                                                 (500, 250, 5, "conjugate", 48), (1000, 500, 22, "conjugate", 20),
                                                 # Jeffreys on the tiled path: the rank-one term is fused into the Gram kernel
                                                 # (border column at the last / the first column of its super-tile)
                                                 (447, 900, 1, "jeffreys", 12), (512, 1100, 1, "jeffreys", 12)])
def test_shared_gram_prefixes(native, k, N, hf_days, strat, W):
    """Rolling windows over one panel (register-tile path and tiled path; windows that span several restarts of the running sums): the whole aligned 16-row blocks of every window come from the
    shared running sums (W n_r >= 3 panel rows switches them on) - against the oracle at the flat 1e-10 bound, against
    the same batch with TP_FLAG_NO_SHARED_GRAM to a few ulps, and bit-identical for any sub-batch (the sums depend
    on the panel only)."""
    inp = synthetic.make_kernel_inputs(k, N, W, seed=990000 + k, hf_days=hf_days, hf_period=8)
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
    if strat == "conjugate":
        kw.update(hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    assert W * inp["n_r"] >= 3 * inp["panel"].shape[0]
    wts, status, aux = native.posterior_batch(strat, k, N, 5.0, **kw)
    plain, pstat, paux = native.posterior_batch(strat, k, N, 5.0, flags=native.FLAG_NO_SHARED_GRAM, **kw)
    assert (status == 0).all() and (pstat == 0).all()
    np.testing.assert_allclose(wts, plain, rtol=0, atol=1e-12 * max(1.0, np.abs(plain).max()))
    sel = np.array([0, 1, W // 2, W - 1])
    sub = {key: (val[sel] if key in ("start", "hf_start", "w0", "n0") else val) for key, val in kw.items()}
    ref, rstat, _ = oracle.posterior_batch_c(strat, k, N, 5.0, **sub)
    np.testing.assert_allclose(wts[sel], ref, **WTOL)
    half = {key: (val[W // 3:] if key in ("start", "hf_start", "w0", "n0") else val) for key, val in kw.items()}
    assert (W - W // 3) * inp["n_r"] >= 3 * inp["panel"].shape[0]
    wh, _, _ = native.posterior_batch(strat, k, N, 5.0, **half)
    assert np.array_equal(wh, wts[W // 3:])
