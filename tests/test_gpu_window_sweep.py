"""Window sweeps (tp_batch_window_sweep / Batch.window_sweep): L nested window lengths per window - the last rows[w][l] daily
rows - from one pass over the rows of the longest.  Checked against the oracle called once per length on the suffix rows with
that length's risk-free offsets and N_l (the table of tests/_window_sweep_cases.py, vouched for on the CPU by
tests/test_host_window_sweep_cases.py), against the prior sweep and the run kernels on the whole window, that the delta
correction is really applied, for bitwise independence of W / the slot / P / the sub-ranges, for isolation of a length from
older rows, the contract, that the batch is left alone, and the product path (calculate_weights_for_windows).  -m gpu."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from incorporating_different_sources_amd import _native, synthetic
from oracle import oracle

import _window_sweep_cases as cases
from _window_sweep_cases import GAMMA, TOL

pytestmark = pytest.mark.gpu


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


def upload(dev, pr, flags=0):
    inp, conj = pr["inp"], pr["strategy"] == "conjugate"
    b = dev.batch(pr["strategy"], pr["k"], inp["N"], inp["n_r"], GAMMA, cases.W, inp["m"] if conj else 0, flags)
    ukw = pr["upload"] if conj else {key: val for key, val in pr["upload"].items() if not key.startswith("hf_") and key not in ("w0", "n0")}
    b.upload(pr["panel"], **ukw)
    return b


# ---- 1. against the oracle --------------------------------------------------------------------------------------------
CONJ = list(cases.problems("conjugate"))
JEFF = list(cases.problems("jeffreys"))


@pytest.mark.parametrize("pr", CONJ, ids=[pr["id"] for pr in CONJ])
def test_window_sweep_matches_oracle_conjugate(dev, pr):
    L, k = len(pr["N"]), pr["k"]
    b = upload(dev, pr)
    wts, status, aux = b.window_sweep(pr["N"], pr["rows"], pr["n0"], pr["w0"], delta=pr["delta"])
    b.close()
    assert wts.shape == (cases.W, cases.P, L, k) and status.shape == (cases.W, cases.P, L) and aux.shape == (cases.W, cases.P, L, 8)
    assert (status == _native.STATUS_OK).all(), status
    ref, _, raux = cases.reference(pr)
    for l in range(L):
        assert_close(wts[:, :, l], ref[:, :, l], what=f"{pr['id']} rows={pr['rows'][:, l].tolist()}")
    np.testing.assert_allclose(aux[..., :6], raux[..., :6], rtol=cases.AUX_RTOL, atol=cases.AUX_ATOL)
    assert np.array_equal(aux[..., 0], pr["n0"])


@pytest.mark.parametrize("flags", [0, _native.FLAG_CENTER_BY_ROWS, _native.FLAG_NO_CENTER])
@pytest.mark.parametrize("pr", JEFF, ids=[pr["id"] for pr in JEFF])
def test_window_sweep_matches_oracle_jeffreys(dev, pr, flags):
    L, k = len(pr["N"]), pr["k"]
    b = upload(dev, pr, flags)
    wts, status, aux = b.window_sweep(pr["N"], pr["rows"], delta=pr["delta"])
    b.close()
    assert wts.shape == (cases.W, 1, L, k) and status.shape == (cases.W, 1, L) and aux.shape == (cases.W, 1, L, 8)
    assert (status == _native.STATUS_OK).all(), status
    ref, _, _ = cases.reference(pr, flags)
    for l in range(L):
        assert_close(wts[:, :, l], ref[:, :, l], what=f"{pr['id']} flags={flags} rows={pr['rows'][:, l].tolist()}")
    # aux: what tp_batch_download gives a Jeffreys window - zeros except q1 = t'M^-1 t = gamma t'(the weights)
    assert not aux[..., [0, 1, 2, 3, 5, 6, 7]].any()
    assert np.array_equal(aux[..., 0], np.zeros((cases.W, 1, L)))      # "n0" of a Jeffreys batch
    # The oracle has no q1 for Jeffreys: gamma t'(its weights) stands in, as in tests/test_gpu_size_sweep.py, at the project's
    # tolerance for aux (the CPU test holds the stand-in to a quarter of it against an extended-precision t'M^-1 t).
    for w in range(cases.W):
        for l in range(L):
            X, _ = cases.window_rows(pr, w, l)
            q1 = GAMMA * X.sum(axis=0) @ ref[w, 0, l]
            print(f"{pr['id']} flags={flags} w={w} rows={pr['rows'][w, l]}: rel |q1 - ref| = {abs(aux[w, 0, l, 4] / q1 - 1):.3e}")
            np.testing.assert_allclose(aux[w, 0, l, 4], q1, rtol=cases.AUX_RTOL, atol=cases.AUX_ATOL)


# ---- 2. against the existing paths on the whole window; the correction is really applied ------------------------------
def test_whole_window_without_delta_equals_prior_sweep_and_run(dev):
    k, N, W, P = 33, 130, 3, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=921000)
    n_r = inp["n_r"]
    rng = np.random.default_rng(921000)
    Nl = np.array([20, 64, N], dtype=np.int32)
    rows = np.tile(np.array([19, 63, n_r], dtype=np.int32), (W, 1))
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(W, P, 3))
    w0 = np.stack([inp["w0"], np.full((W, k), 1.0 / k)], axis=1)
    zero = np.zeros((W, 3, n_r))
    b = dev.batch("conjugate", k, N, n_r, GAMMA, W, inp["m"])
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    pw, pstat, paux = b.prior_sweep(np.ascontiguousarray(n0[:, :, 2]), w0)
    plain = b.window_sweep(Nl, rows, n0, w0)
    zeroed = b.window_sweep(Nl, rows, n0, w0, delta=zero)
    b.close()
    assert (pstat == 0).all() and (plain[1] == 0).all()
    assert_close(plain[0][:, :, 2], pw, what="conjugate, whole window vs prior_sweep")
    np.testing.assert_allclose(plain[2][:, :, 2, :6], paux[..., :6], rtol=1e-11, atol=1e-14)
    for x, y in zip(plain, zeroed):                                    # an all-zero delta reproduces G and g exactly
        assert np.array_equal(x, y)
    Nj = np.array([41, 64, N], dtype=np.int32)                         # (more rows than columns at every length)
    rows_j = np.tile(np.array([40, 63, n_r], dtype=np.int32), (W, 1))
    for flags in (0, _native.FLAG_CENTER_BY_ROWS, _native.FLAG_NO_CENTER):
        j = dev.batch("jeffreys", k, N, n_r, GAMMA, W, 0, flags)
        j.upload(inp["panel"], start=inp["start"])
        full, fstat, faux = j.run().download()
        wts, status, aux = j.window_sweep(Nj, rows_j)
        j.close()
        assert (fstat == 0).all() and (status == 0).all()
        assert_close(wts[:, 0, 2], full, what=f"jeffreys flags={flags}, whole window vs run")
        np.testing.assert_allclose(aux[:, 0, 2, 4], faux[:, 4], rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_delta_changes_the_result_by_more_than_the_bound(dev, strategy):
    pr = next(p for p in cases.problems(strategy, ks=[33]) if p["layout"] == "index" and p["delta"] is not None)
    pri = (pr["n0"], pr["w0"]) if strategy == "conjugate" else ()
    b = upload(dev, pr)
    with_delta = b.window_sweep(pr["N"], pr["rows"], *pri, delta=pr["delta"])[0]
    without = b.window_sweep(pr["N"], pr["rows"], *pri)[0]
    b.close()
    ref, _, _ = cases.reference(pr)
    for l in range(len(pr["N"])):
        assert_close(with_delta[:, :, l], ref[:, :, l], what=f"{strategy} with delta, rows={pr['rows'][:, l].tolist()}")
        moved = float(np.abs(with_delta[:, :, l] - without[:, :, l]).max())
        print(f"{strategy} rows={pr['rows'][:, l].tolist()}: delta moves the weights by {moved:.3e} (bound {cases.bound(ref[:, :, l]):.3e})")
        assert moved > cases.bound(ref[:, :, l])


# ---- 3. independence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_window_sweep_is_bitwise_independent_of_W_slot_P_and_chunking(dev, strategy):
    k, N, W, P = 50, 100, 7, 3
    conj = strategy == "conjugate"
    inp = synthetic.make_kernel_inputs(k, N, W, seed=922000)
    n_r = inp["n_r"]
    rng = np.random.default_rng(922000)
    Nl = np.array([61, 70, 73, 80, 100], dtype=np.int32)
    rows = np.stack([np.array([60, 69, 72, 79, 99], dtype=np.int32) - (w % 3) for w in range(W)])
    L = len(Nl)
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(W, P, L))
    w0 = rng.dirichlet(np.ones(k), size=(W, P))
    delta = rng.normal(0.0, 1e-6, size=(W, L, n_r))

    def sweep(windows, priors, lengths=None, chunk=0):
        dev.set_option("sweep_chunk_windows", chunk)
        try:
            ws = np.asarray(windows)
            ls = np.arange(L) if lengths is None else np.asarray(lengths)
            b = dev.batch(strategy, k, N, n_r, GAMMA, len(ws), inp["m"] if conj else 0)
            if conj:
                b.upload(inp["panel"], start=inp["start"][ws], hf_start=inp["hf_start"][ws], w0=inp["w0"][ws], n0=inp["n0"][ws],
                         hf_panel=inp["hf_panel"])
            else:
                b.upload(inp["panel"], start=inp["start"][ws])
            pri = (n0[np.ix_(ws, priors, ls)], w0[np.ix_(ws, priors)]) if conj else ()
            out = b.window_sweep(Nl[ls], rows[np.ix_(ws, ls)], *pri, delta=delta[np.ix_(ws, ls)])
            b.close()
            return out
        finally:
            dev.set_option("sweep_chunk_windows", 0)

    allp = list(range(P)) if conj else [0]
    full = sweep(range(W), allp)
    assert (full[1] == 0).all()
    one = sweep([3], allp)                                 # W = 1 against 7
    for a, f in zip(one, full):
        assert np.array_equal(a[0], f[3])
    rev = sweep(list(range(W))[::-1], allp)                # every window in another slot
    for a, f in zip(rev, full):
        assert np.array_equal(a[::-1], f)
    if conj:
        single = sweep(range(W), [1])                      # P = 1 against 3
        for a, f in zip(single, full):
            assert np.array_equal(a[:, 0], f[:, 1])
        swapped = sweep(range(W), allp[::-1])              # every prior in another slot
        for a, f in zip(swapped, full):
            assert np.array_equal(a[:, ::-1], f)
    for chunk in (1, 2):                                   # sub-ranges of 1 and 2 windows against automatic
        cut = sweep(range(W), allp, chunk=chunk)
        for a, f in zip(cut, full):
            assert np.array_equal(a, f)
    # another list of lengths cuts the partial sums elsewhere: the shared lengths agree within the bound
    some = sweep(range(W), allp, lengths=[1, 4])
    assert_close(some[0], full[0][:, :, [1, 4]], what=f"{strategy}: lengths [1, 4] alone vs the list of 5")
    assert np.array_equal(some[1], full[1][:, :, [1, 4]])


# ---- 4. isolation -----------------------------------------------------------------------------------------------------
ISO_K, ISO_N, ISO_W = 20, 90, 3
ISO_ROWS = [30, 40, 60, 89]


def _iso_sweep(dev, strategy, panel, row_idx, inp, rng_seed=923000):
    conj = strategy == "conjugate"
    rng = np.random.default_rng(rng_seed)
    Nl = np.asarray(ISO_ROWS, dtype=np.int32) + 1
    rows = np.tile(np.asarray(ISO_ROWS, dtype=np.int32), (ISO_W, 1))
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(ISO_W, 2, len(ISO_ROWS)))
    w0 = rng.dirichlet(np.ones(ISO_K), size=(ISO_W, 2))
    delta = rng.normal(0.0, 1e-6, size=(ISO_W, len(ISO_ROWS), inp["n_r"]))
    b = dev.batch(strategy, ISO_K, ISO_N, inp["n_r"], GAMMA, ISO_W, inp["m"] if conj else 0)
    if conj:
        b.upload(panel, row_idx=row_idx, hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
        out = b.window_sweep(Nl, rows, n0, w0, delta=delta)
    else:
        b.upload(panel, row_idx=row_idx)
        out = b.window_sweep(Nl, rows, delta=delta)
    b.close()
    return out


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("damage", [np.nan, 1e6])
def test_a_row_older_than_a_suffix_never_reaches_it(dev, strategy, damage):
    """Window 1 reads a damaged row at position n_r - 50: inside segment 2 (the rows of length 60 that length 40 does not
    have).  Lengths 30 and 40 are bit for bit those of the clean run; lengths 60 and 89 are flagged (NaN) or changed (outlier)."""
    inp = synthetic.make_kernel_inputs(ISO_K, ISO_N, ISO_W, seed=923000)
    n_r = inp["n_r"]
    row_idx = (inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32)
    clean = _iso_sweep(dev, strategy, inp["panel"], row_idx, inp)
    assert (clean[1] == 0).all()
    pos = n_r - 50
    extra = inp["panel"][row_idx[1, pos]].copy()
    extra[7] = damage
    bad_idx = row_idx.copy()
    bad_idx[1, pos] = inp["panel"].shape[0]                # window 1 alone reads the extra row
    hit = _iso_sweep(dev, strategy, np.concatenate([inp["panel"], extra[None, :]], axis=0), bad_idx, inp)
    for c, h in zip(clean, hit):
        assert np.array_equal(c[[0, 2]], h[[0, 2]])        # the other windows
        assert np.array_equal(c[1][:, :2], h[1][:, :2])    # lengths 30 and 40 of the damaged window: bit for bit
    assert (hit[1][1][:, :2] == _native.STATUS_OK).all()
    if np.isnan(damage):
        assert (hit[1][1][:, 2:] != _native.STATUS_OK).all(), hit[1]
    else:
        assert (np.abs(hit[0][1][:, 2:] - clean[0][1][:, 2:]).max(axis=-1) > 0).all()


def test_jeffreys_length_of_fewer_rows_than_columns_is_not_pd_for_that_length_only(dev):
    k, N, W = 33, 130, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=923100)
    Nl = np.array([6, 61, 130], dtype=np.int32)
    rows = np.tile(np.array([5, 60, 129], dtype=np.int32), (W, 1))
    b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W, 0)
    b.upload(inp["panel"], start=inp["start"])
    wts, status, _ = b.window_sweep(Nl, rows)
    b.close()
    assert (status[:, 0, 0] == _native.STATUS_NOT_PD).all() and (status[:, 0, 1:] == _native.STATUS_OK).all(), status
    for l in (1, 2):
        ref = np.stack([oracle.jeffreys_window(inp["panel"][inp["start"][w] + inp["n_r"] - rows[w, l]:inp["start"][w] + inp["n_r"]],
                                               int(Nl[l]), GAMMA) for w in range(W)])
        assert_close(wts[:, 0, l], ref, what=f"rows={rows[0, l]} next to a singular length")


# ---- 5. the contract ----------------------------------------------------------------------------------------------------
def test_window_sweep_contract(dev):
    k, N, W, P = 10, 60, 3, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=924000)
    n_r = inp["n_r"]
    rng = np.random.default_rng(924000)
    Nl = np.array([20, 40, 60], dtype=np.int32)
    rows = np.tile(np.array([19, 39, 59], dtype=np.int32), (W, 1))
    L = 3
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(W, P, L))
    w0 = rng.dirichlet(np.ones(k), size=(W, P))
    delta = rng.normal(0.0, 1e-6, size=(W, L, n_r))
    lib = _native.lib
    pd_, pi_ = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ptr = lambda a: a.ctypes.data_as(pd_)
    keep = []

    def iptr(a):
        keep.append(np.ascontiguousarray(a, dtype=np.int32))
        return keep[-1].ctypes.data_as(pi_)

    def code(b, fn):
        with pytest.raises(_native.TangencyError) as e:
            fn(b)
        return e.value.code

    INV = _native.TP_ERR_INVALID
    b = dev.batch("conjugate", k, N, n_r, GAMMA, W, inp["m"])
    assert code(b, lambda b: b.window_sweep(Nl, rows, n0, w0)) == INV                                  # not uploaded
    n_rows = np.array([n_r, n_r - 2, n_r], dtype=np.int32)
    b.upload(inp["panel"], start=inp["start"], n_rows=n_rows, hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    rows_ok = np.minimum(rows, n_rows[:, None]).astype(np.int32)
    out = np.empty((W, P, L, k))
    assert lib.tp_batch_download_window_sweep(b._b, ptr(out), None, None) == INV                       # no sweep before it
    call = lambda n_len, Np, rp, dp, npri, n0p, w0p: lib.tp_batch_window_sweep(b._b, n_len, Np, rp, dp, npri, n0p, w0p)
    assert call(0, iptr(Nl), iptr(rows_ok), None, P, ptr(n0), ptr(w0)) == INV                          # n_len < 1
    big = np.arange(1, 18, dtype=np.int32)
    assert call(17, iptr(big), iptr(np.tile(big, (W, 1))), None, P, ptr(np.ones((W, P, 17))), ptr(w0)) == INV   # n_len > 16
    assert call(L, None, iptr(rows_ok), None, P, ptr(n0), ptr(w0)) == INV                              # N NULL
    for bad in ([0, 40, 60], [20, 20, 60], [40, 20, 60]):                                              # < 1, not strictly increasing
        assert call(L, iptr(bad), iptr(rows_ok), None, P, ptr(n0), ptr(w0)) == INV
    assert call(L, iptr(Nl), None, None, P, ptr(n0), ptr(w0)) == INV                                   # rows NULL
    for w, l, bad in ((0, 0, 0), (2, 2, n_r + 1), (1, 2, n_r - 1), (0, 1, 18)):                        # < 1, > n_w (twice), decreasing
        rb = rows_ok.copy()
        rb[w, l] = bad
        assert code(b, lambda b: b.window_sweep(Nl, rb, n0, w0)) == INV, (w, l, bad)
    tie = rows_ok.copy()
    tie[0, 1] = tie[0, 0]                                                                              # a tie is allowed
    tied = b.window_sweep(Nl, tie, n0, w0)
    assert (tied[1] == 0).all()
    for bad in (np.nan, np.inf):                                                                       # a delta some length reads
        db = delta.copy()
        db[1, 0, n_rows[1] - 1] = bad
        assert code(b, lambda b: b.window_sweep(Nl, rows_ok, n0, w0, delta=db)) == INV
    junk = delta.copy()                                    # positions no length reads may hold anything: older rows, the unused tail
    junk[:, 0, :n_r - 2 - 19] = np.nan
    junk[1, :, n_rows[1]:] = np.inf
    a1 = b.window_sweep(Nl, rows_ok, n0, w0, delta=delta)
    a2 = b.window_sweep(Nl, rows_ok, n0, w0, delta=junk)
    for x, y in zip(a1, a2):
        assert np.array_equal(x, y)
    assert call(L, iptr(Nl), iptr(rows_ok), None, 0, ptr(n0), ptr(w0)) == INV                          # n_prior < 1
    assert call(L, iptr(Nl), iptr(rows_ok), None, P, None, ptr(w0)) == INV                             # NULL priors
    assert call(L, iptr(Nl), iptr(rows_ok), None, P, ptr(n0), None) == INV
    for bad in (0.0, -1.0, np.nan, np.inf):
        n0b = n0.copy()
        n0b[1, 1, 2] = bad
        assert code(b, lambda b: b.window_sweep(Nl, rows_ok, n0b, w0)) == INV
    w0b = w0.copy()
    w0b[2, 0, 6] = np.nan
    assert code(b, lambda b: b.window_sweep(Nl, rows_ok, n0, w0b)) == INV
    wts, status, aux = b.window_sweep(Nl, rows_ok, n0, w0)                                             # the batch still works
    assert (status == 0).all()
    assert lib.tp_batch_download_window_sweep(b._b, ptr(out), None, None) == 0 and np.array_equal(out, wts)
    assert lib.tp_batch_download_window_sweep(b._b, None, None, None) == 0                             # each may be NULL
    # a call refused for its arguments - rows and delta are checked last - keeps the results of the last sweep
    rb, db = rows_ok.copy(), delta.copy()
    rb[2, 1] = 0
    db[0, 2, n_r - 1] = np.nan
    assert code(b, lambda b: b.window_sweep(Nl, rb, n0, w0)) == INV
    assert code(b, lambda b: b.window_sweep(Nl, rows_ok, n0, w0, delta=db)) == INV
    out[:] = 0
    assert lib.tp_batch_download_window_sweep(b._b, ptr(out), None, None) == 0 and np.array_equal(out, wts)
    b.close()

    j = dev.batch("jeffreys", k, N, n_r, GAMMA, W, 0)
    j.upload(inp["panel"], start=inp["start"])
    assert code(j, lambda b: b.window_sweep(Nl, rows, n0, w0)) == INV                                  # Jeffreys with priors
    jcall = lambda npri, n0p, w0p: lib.tp_batch_window_sweep(j._b, L, iptr(Nl), iptr(rows), None, npri, n0p, w0p)
    assert jcall(1, None, None) == INV and jcall(0, ptr(n0), None) == INV and jcall(0, None, ptr(w0)) == INV
    assert (j.window_sweep(Nl, rows)[1] == 0).all()
    j.close()

    kb = _native.sweep_max_assets() + 1
    bigk = synthetic.make_kernel_inputs(kb, kb + 20, 1, seed=924001)
    g = dev.batch("conjugate", kb, kb + 20, bigk["n_r"], GAMMA, 1, bigk["m"])
    g.upload(bigk["panel"], start=bigk["start"], hf_panel=bigk["hf_panel"], hf_start=bigk["hf_start"], w0=bigk["w0"], n0=bigk["n0"])
    assert code(g, lambda b: b.window_sweep([kb + 20], np.full((1, 1), bigk["n_r"], dtype=np.int32), bigk["n0"][:, None, None],
                                            bigk["w0"][:, None, :])) == _native.TP_ERR_UNSUPPORTED
    g.close()


def test_window_sweep_refuses_index_layout_windows_too_long_for_the_gram_pass(dev):
    """The Gram pass stages the row indices and risk-free adjustments of a pass in LDS, 12 bytes per row inside 128 KiB (the
    prior sweep's rule): TP_ERR_UNSUPPORTED before any kernel is launched, no result to download, the device goes on working."""
    k, W, n_r, m = 3, 1, 11_000, 20
    rng = np.random.default_rng(924100)
    panel = rng.normal(0.0, 0.01, size=(64, k))
    hf = rng.normal(0.0, 0.001, size=(m, k))
    b = dev.batch("conjugate", k, n_r + 1, n_r, GAMMA, W, m)
    b.upload(panel, row_idx=rng.integers(0, 64, size=(W, n_r)).astype(np.int32), hf_panel=hf, hf_start=np.zeros(W, dtype=np.int64),
             w0=np.full((W, k), 1.0 / k), n0=np.full(W, 100.0))
    with pytest.raises(_native.TangencyError) as e:
        b.window_sweep([100, n_r + 1], np.array([[99, n_r]], dtype=np.int32), np.full((W, 1, 2), 100.0), np.full((W, 1, k), 1.0 / k))
    assert e.value.code == _native.TP_ERR_UNSUPPORTED
    out = np.empty((W, 1, 2, k))
    assert _native.lib.tp_batch_download_window_sweep(b._b, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None) == _native.TP_ERR_INVALID
    b.close()
    pr = next(p for p in cases.problems("conjugate", ks=[5]) if p["layout"] == "index")
    b = upload(dev, pr)
    wts, status, _ = b.window_sweep(pr["N"], pr["rows"], pr["n0"], pr["w0"])
    b.close()
    assert (status == 0).all()
    assert_close(wts, cases.reference(pr)[0], what="after the refused call")


def test_window_sweep_leaves_the_batch_alone(dev):
    k, N, W, P = 33, 80, 5, 2
    sizes = [4, 20, 33]
    inp = synthetic.make_kernel_inputs(k, N, W, seed=925000)
    rng = np.random.default_rng(925000)
    Nl = np.array([40, 80], dtype=np.int32)
    rows = np.tile(np.array([39, 79], dtype=np.int32), (W, 1))
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(W, P, 2))
    w0 = rng.dirichlet(np.ones(k), size=(W, P))
    w0s = np.repeat(w0[:, :, None, :], len(sizes), axis=2)
    rhs = rng.normal(size=(W, 2, k))
    b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    b.keep_rhs().keep_posterior()
    b.run()
    solved = b.solve_sweep(rhs=rhs)
    priored = b.prior_sweep(n0[:, :, 1].copy(), w0)
    sized = b.size_sweep(sizes, n0[:, :, 1].copy(), w0s)
    lib = _native.lib
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def earlier():
        x, pw, sw = np.empty_like(solved[0]), np.empty_like(priored[0]), np.empty_like(sized[0])
        assert lib.tp_batch_download_sweep(b._b, ptr(x), None) == 0 and lib.tp_batch_download_prior_sweep(b._b, ptr(pw), None, None) == 0
        assert lib.tp_batch_download_size_sweep(b._b, ptr(sw), None, None) == 0
        return (*b.download(), b.download_rhs(), b.download_posterior(), b.download_sweep_rhs(), x, pw, sw, dev.last_launch())

    before = earlier()
    swept = b.window_sweep(Nl, rows, n0, w0)
    after = earlier()
    for x, y in zip(before[:-1], after[:-1]):
        assert np.array_equal(x, y)
    assert before[-1] == after[-1]
    assert np.array_equal(before[6], solved[0]) and np.array_equal(before[7], priored[0]) and np.array_equal(before[8], sized[0])
    # the other sweeps and a window sweep on the same batch, in either order, return what they return alone
    priored2 = b.prior_sweep(n0[:, :, 1].copy(), w0)
    sized2 = b.size_sweep(sizes, n0[:, :, 1].copy(), w0s)
    again = b.window_sweep(Nl, rows, n0, w0)
    b.close()
    for x, y in zip(swept + priored + sized, again + priored2 + sized2):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_window_sweep_is_one_timed_step(dev, strategy):
    k, N, W, P = 10, 60, 6, 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=925100)
    conj = strategy == "conjugate"
    Nl = np.array([30, 60], dtype=np.int32)
    rows = np.tile(np.array([29, 59], dtype=np.int32), (W, 1))
    b = dev.batch(strategy, k, N, inp["n_r"], GAMMA, W, inp["m"] if conj else 0)
    if conj:
        b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    else:
        b.upload(inp["panel"], start=inp["start"])
    pri = (np.full((W, P, 2), 80.0), np.full((W, P, k), 1.0 / k)) if conj else ()
    dev.set_option("sweep_chunk_windows", 2)               # three sub-ranges, still one step
    try:
        dev.region_begin()
        b.window_sweep(Nl, rows, *pri, delta=np.full((W, 2, inp["n_r"]), 1e-6))
        dev.region_end()
    finally:
        dev.set_option("sweep_chunk_windows", 0)
    steps = dev.region_steps()
    b.close()
    assert len(steps) == 1 and steps[0] > 0 and dev.last_timing()["kernel_ms"] > 0


# ---- 6. the product path ----------------------------------------------------------------------------------------------
def _spec(strat, k, N, freq, scaling=1):
    return {"weighting_strategy": strat, "size": k, "risk_aversion": 5, "turnover_cost": 15,
            "rebalancing_frequency": "daily", "rolling_window": N, "rolling_window_frequency": freq,
            "mcm_scaling": scaling, "display_name": f"{strat}_{N}_{scaling}"}


@pytest.mark.parametrize("freq,k,windows,first", [("daily", 8, [20, 30, 60], 25), ("weekly", 6, [12, 14, 16], 62)])
@pytest.mark.parametrize("names", [("conjugate_hf_vix_vw", "conjugate_hf_epu_ew"), ("jeffreys",)])
def test_calculate_weights_for_windows_equals_spec_by_spec(names, freq, k, windows, first, monkeypatch):
    """Business days at rf = 0.02: the daily lengths have different mean calendar gaps, so the sweep must be given a delta.  The
    first dates are early enough that the longer windows are cut by the start of the data (ties in `rows`)."""
    from incorporating_different_sources_amd import batch, portfolio_calculations as pc
    md, _ = synthetic.make_market_data(n_tickers=14, n_days=130, seed=20240094)
    days = md["stock_prices_df"].index
    dates = [pd.Timestamp(d) for d in days[first:first + 40:4]]
    specs = [_spec(name, k, N, freq, 5 if name.endswith("ew") else 1) for name in names for N in windows]
    batch.clear_panel_cache()
    plain = [pc._weights_for_dates(dates, sp, md) for sp in specs]
    batch.clear_panel_cache()
    packs, sweeps = [], []
    real_pack, real_sweep = batch.pack_windows_lengths, _native.Batch.window_sweep

    def pack(d, sp, wins, m, **kw):
        packs.append(real_pack(d, sp, wins, m, **kw))
        return packs[-1]

    def sweep(self, N, rows, n0=None, w0=None, delta=None, **kw):
        sweeps.append((list(N), None if n0 is None else n0.shape, None if w0 is None else w0.shape, delta is not None))
        return real_sweep(self, N, rows, n0, w0, delta=delta, **kw)

    monkeypatch.setattr(batch, "pack_windows_lengths", pack)
    monkeypatch.setattr(_native.Batch, "window_sweep", sweep)
    shared = pc.calculate_weights_for_windows(dates, specs, md)
    W = len(dates)
    assert len(packs) == 1 and packs[0][5].all()
    rows, delta = packs[0][3], packs[0][4]
    assert (rows[:, :-1] == rows[:, 1:]).any() and (rows[:, :-1] < rows[:, 1:]).any()      # truncated at the first dates only
    assert bool(delta.any()) == (freq == "daily")
    conj = names[0] != "jeffreys"
    assert sweeps == [(windows, (W, 2, 3) if conj else None, (W, 2, k) if conj else None, freq == "daily")]
    for sp, a, b in zip(specs, plain, shared):
        assert b[0].shape == (W, k)
        assert_close(b[0], a[0], what=sp["display_name"] + " " + freq)
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    if conj:           # the backtest calls that follow find the cache filled: no device batch of their own
        monkeypatch.setattr(_native, "posterior_batch", lambda *a, **kw: pytest.fail("the cache was not filled"))
        for sp, res in zip(specs, shared):
            assert pc._weights_for_dates(dates, sp, md)[0] is res[0]
    batch.clear_panel_cache()


def test_calculate_weights_for_windows_serves_masked_pairs_spec_by_spec():
    """A late-listed large cap: at one date the shortest window has another universe than the pack.  That (date, length) comes
    from `_weights_for_dates` - labels and columns included - and everything else from the sweep."""
    from incorporating_different_sources_amd import batch, portfolio_calculations as pc
    md, _ = synthetic.make_market_data(n_tickers=12, n_days=70, seed=20240093)
    days = md["stock_prices_df"].index
    prices = md["stock_prices_df"].copy()
    big = md["stock_market_caps_df"].loc[days[45]].idxmax()
    prices.loc[prices.index < days[30], big] = np.nan
    md = dict(md, stock_prices_df=prices)
    dates = [pd.Timestamp(d) for d in (days[38], days[45], days[62])]
    specs = [_spec("jeffreys", 8, N, "daily") for N in (12, 20, 30)]
    batch.clear_panel_cache()
    assert batch.pack_windows_lengths(dates, specs[0], [12, 20, 30], md)[5].tolist() == [[True] * 3, [False, True, True], [True] * 3]
    plain = [pc._weights_for_dates(dates, sp, md) for sp in specs]
    shared = pc.calculate_weights_for_windows(dates, specs, md)
    assert big in shared[0][1][1] and big not in shared[1][1][1]
    for sp, a, b in zip(specs, plain, shared):
        assert_close(b[0], a[0], what=sp["display_name"])
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    batch.clear_panel_cache()
