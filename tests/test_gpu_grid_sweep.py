"""Grid sweeps (tp_batch_grid_sweep / Batch.grid_sweep): S nested universes x L nested window lengths per window from one pass
over the rows and ONE factorisation per (window, prior, length).  Checked against the oracle called once per (prior, length,
size) on the suffix rows and prefix columns (the table of tests/_grid_sweep_cases.py, vouched for on the CPU by
tests/test_host_grid_sweep_cases.py), against the window sweep and the size sweep on the same batch, for bitwise independence of
W / the slot / P / the sub-ranges / the other sizes, for isolation of a prefix from later columns and of a suffix from older
rows, the contract, that the batch and the other sweeps are left alone, and the product path (calculate_weights_for_grid).
-m gpu."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from incorporating_different_sources_amd import _native, synthetic
from oracle import oracle

import _grid_sweep_cases as cases
from _grid_sweep_cases import GAMMA, TOL
from test_gpu_sweeps_coexist import again, same

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


def conjugate_batch(dev, inp, k, N, W, windows=None):
    ws = np.arange(W) if windows is None else np.asarray(windows)
    b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, len(ws), inp["m"])
    b.upload(inp["panel"], start=inp["start"][ws], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"][ws], w0=inp["w0"][ws], n0=inp["n0"][ws])
    return b


def jeffreys_batch(dev, inp, k, N, W, windows=None, flags=0):
    ws = np.arange(W) if windows is None else np.asarray(windows)
    b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, len(ws), 0, flags)
    b.upload(inp["panel"], start=inp["start"][ws])
    return b


def prefix_priors(rng, W, P, sizes, k):
    """w0 [W x P x S x k]: a Dirichlet vector over each prefix, zeros beyond."""
    w0 = np.zeros((W, P, len(sizes), k))
    for s, ks in enumerate(sizes):
        w0[:, :, s, :ks] = rng.dirichlet(np.ones(ks), size=(W, P))
    return w0


# ---- 1. against the oracle --------------------------------------------------------------------------------------------
CONJ = cases.problems("conjugate")
JEFF = cases.problems("jeffreys")


@pytest.mark.parametrize("pr", CONJ, ids=[pr["id"] for pr in CONJ])
def test_grid_sweep_matches_oracle_conjugate(dev, pr):
    L, S, k, P = len(pr["N"]), len(pr["sizes"]), pr["k"], pr["P"]
    b = upload(dev, pr)
    wts, status, aux = b.grid_sweep(pr["sizes"], pr["N"], pr["rows"], pr["n0"], pr["w0g"], delta=pr["delta"])
    b.close()
    assert wts.shape == (cases.W, P, L, S, k) and status.shape == (cases.W, P, L, S) and aux.shape == (cases.W, P, L, S, 8)
    assert (status == _native.STATUS_OK).all(), status
    ref, _, raux = cases.reference(pr)
    for l in range(L):
        for s, ks in enumerate(pr["sizes"]):
            assert_close(wts[:, :, l, s], ref[:, :, l, s], what=f"{pr['id']} rows={pr['rows'][:, l].tolist()} k_s={ks}")
            assert not wts[:, :, l, s, ks:].any()              # exactly zero beyond the prefix
    np.testing.assert_allclose(aux[..., :6], raux[..., :6], rtol=cases.AUX_RTOL, atol=cases.AUX_ATOL)
    assert np.array_equal(aux[..., 0], np.broadcast_to(pr["n0"][..., None], aux.shape[:4]))


@pytest.mark.parametrize("flags", [0, _native.FLAG_CENTER_BY_ROWS, _native.FLAG_NO_CENTER])
@pytest.mark.parametrize("pr", JEFF, ids=[pr["id"] for pr in JEFF])
def test_grid_sweep_matches_oracle_jeffreys(dev, pr, flags):
    L, S, k = len(pr["N"]), len(pr["sizes"]), pr["k"]
    b = upload(dev, pr, flags)
    wts, status, aux = b.grid_sweep(pr["sizes"], pr["N"], pr["rows"], delta=pr["delta"])
    b.close()
    assert wts.shape == (cases.W, 1, L, S, k) and status.shape == (cases.W, 1, L, S) and aux.shape == (cases.W, 1, L, S, 8)
    assert (status == _native.STATUS_OK).all(), status
    ref, _, _ = cases.reference(pr, flags)
    for l in range(L):
        for s, ks in enumerate(pr["sizes"]):
            assert_close(wts[:, :, l, s], ref[:, :, l, s], what=f"{pr['id']} flags={flags} rows={pr['rows'][:, l].tolist()} k_s={ks}")
            assert not wts[:, :, l, s, ks:].any()
    # aux: zeros except q1 = t'M^-1 t over the prefix; the oracle has no q1 for Jeffreys: gamma t'(its weights) stands in (the CPU
    # test holds the stand-in to a quarter of the tolerance against an extended-precision value)
    assert not aux[..., [0, 1, 2, 3, 5, 6, 7]].any()
    for w in range(cases.W):
        for l in range(L):
            X, _ = cases.window_rows(pr, w, l)
            for s, ks in enumerate(pr["sizes"]):
                q1 = GAMMA * X[:, :ks].sum(axis=0) @ ref[w, 0, l, s, :ks]
                np.testing.assert_allclose(aux[w, 0, l, s, 4], q1, rtol=cases.AUX_RTOL, atol=cases.AUX_ATOL)


# ---- 2. consistency with the parents, on the same batch ----------------------------------------------------------------
def _bits(a, b):
    return "bit-identical" if all(np.array_equal(x, y) for x, y in zip(a, b)) else "equal to rounding"


def test_grid_sweep_agrees_with_window_sweep_and_size_sweep_on_the_same_batch(dev):
    k, N, W, P = 33, 130, 3, 2
    sizes = [5, 17, 32, 33]
    S = len(sizes)
    inp = synthetic.make_kernel_inputs(k, N, W, seed=931000)
    n_r = inp["n_r"]
    rng = np.random.default_rng(931000)
    Nl = np.array([45, 64, N], dtype=np.int32)
    rows = np.tile(np.array([44, 63, n_r], dtype=np.int32), (W, 1))
    L = 3
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(W, P, L))
    w0 = prefix_priors(rng, W, P, sizes, k)
    delta = rng.normal(0.0, 1e-6, size=(W, L, n_r))
    for strategy in ("conjugate", "jeffreys"):
        conj = strategy == "conjugate"
        b = conjugate_batch(dev, inp, k, N, W) if conj else jeffreys_batch(dev, inp, k, N, W)
        # sizes = [k] against the window sweep, with a delta
        pri = (n0, np.ascontiguousarray(w0[:, :, S - 1:])) if conj else ()
        wpri = (n0, np.ascontiguousarray(w0[:, :, S - 1])) if conj else ()
        g = b.grid_sweep([k], Nl, rows, *pri, delta=delta)
        ws = b.window_sweep(Nl, rows, *wpri, delta=delta)
        assert (g[1] == 0).all() and np.array_equal(g[1][..., 0], ws[1])
        assert_close(g[0][:, :, :, 0], ws[0], what=f"{strategy}: sizes = [k] vs window_sweep")
        np.testing.assert_allclose(g[2][:, :, :, 0, :6], ws[2][..., :6], rtol=cases.AUX_RTOL, atol=cases.AUX_ATOL)
        print(f"{strategy}: sizes = [k] vs window_sweep: {_bits((g[0][:, :, :, 0], g[2][:, :, :, 0]), (ws[0], ws[2]))}")
        # a single length with rows = n_w and no delta, against the size sweep
        whole = np.full((W, 1), n_r, dtype=np.int32)
        pri = (np.ascontiguousarray(n0[:, :, 2:]), w0) if conj else ()
        spri = (np.ascontiguousarray(n0[:, :, 2]), w0) if conj else ()
        g1 = b.grid_sweep(sizes, [N], whole, *pri)
        zs = b.size_sweep(sizes, *spri)
        assert (g1[1] == 0).all() and np.array_equal(g1[1][:, :, 0], zs[1])
        assert_close(g1[0][:, :, 0], zs[0], what=f"{strategy}: one whole length vs size_sweep")
        np.testing.assert_allclose(g1[2][:, :, 0, :, :6], zs[2][..., :6], rtol=cases.AUX_RTOL, atol=cases.AUX_ATOL)
        print(f"{strategy}: one whole length vs size_sweep: {_bits((g1[0][:, :, 0], g1[2][:, :, 0]), (zs[0], zs[2]))}")
        # an all-zero delta against delta = None: bit for bit
        pri = (n0, w0) if conj else ()
        plain = b.grid_sweep(sizes, Nl, rows, *pri)
        zeroed = b.grid_sweep(sizes, Nl, rows, *pri, delta=np.zeros((W, L, n_r)))
        b.close()
        for x, y in zip(plain, zeroed):
            assert np.array_equal(x, y)


# ---- 3. promises ------------------------------------------------------------------------------------------------------
SIZES16 = [3, 7, 8, 15, 16, 17, 24, 31, 32, 33, 40, 45, 47, 48, 49, 50]


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_grid_sweep_is_bitwise_independent_of_W_slot_P_chunking_and_the_other_sizes(dev, strategy):
    k, N, P = 50, 100, 3
    W = 2
    conj = strategy == "conjugate"
    inp = synthetic.make_kernel_inputs(k, N, W, seed=932000)
    n_r = inp["n_r"]
    rng = np.random.default_rng(932000)
    Nl = np.array([61, 70, 73, 100], dtype=np.int32)
    rows = np.stack([np.array([60, 69, 72, 99], dtype=np.int32) - w for w in range(W)])
    L = len(Nl)
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(W, P, L))
    w0 = prefix_priors(rng, W, P, SIZES16, k)
    delta = rng.normal(0.0, 1e-6, size=(W, L, n_r))
    base = [2, 5, 9]                                       # positions in SIZES16: the list of 3

    def sweep(windows, priors, spos=base, lengths=None, chunk=0):
        dev.set_option("sweep_chunk_windows", chunk)
        try:
            ws = np.asarray(windows)
            ls = np.arange(L) if lengths is None else np.asarray(lengths)
            b = conjugate_batch(dev, inp, k, N, W, ws) if conj else jeffreys_batch(dev, inp, k, N, W, ws)
            pri = (n0[np.ix_(ws, priors, ls)], w0[np.ix_(ws, priors, spos)]) if conj else ()
            out = b.grid_sweep([SIZES16[i] for i in spos], Nl[ls], rows[np.ix_(ws, ls)], *pri, delta=delta[np.ix_(ws, ls)])
            b.close()
            return out
        finally:
            dev.set_option("sweep_chunk_windows", 0)

    allp = list(range(P)) if conj else [0]
    full = sweep(range(W), allp)
    assert (full[1] == 0).all()
    one = sweep([1], allp)                                 # W = 1 against 2
    for a, f in zip(one, full):
        assert np.array_equal(a[0], f[1])
    rev = sweep([1, 0], allp)                              # every window in another slot
    for a, f in zip(rev, full):
        assert np.array_equal(a[::-1], f)
    if conj:
        single = sweep(range(W), [1])                      # P = 1 against 3
        for a, f in zip(single, full):
            assert np.array_equal(a[:, 0], f[:, 1])
        swapped = sweep(range(W), allp[::-1])              # every prior in another slot
        for a, f in zip(swapped, full):
            assert np.array_equal(a[:, ::-1], f)
    cut = sweep(range(W), allp, chunk=1)                   # sub-ranges of 1 window against automatic
    for a, f in zip(cut, full):
        assert np.array_equal(a, f)
    # the other sizes of the list: size 33 (position 9) alone and in lists of 3, 6, 10 and 16 - the four builds of the fill
    alone = sweep(range(W), allp, spos=[9])
    for spos in (base, [0, 2, 5, 9, 12, 15], [0, 1, 2, 4, 5, 8, 9, 11, 13, 15], list(range(16))):
        many = sweep(range(W), allp, spos=spos)
        assert (many[1] == 0).all()
        at = spos.index(9)
        for a, f in zip(alone, many):
            assert np.array_equal(a[:, :, :, 0], f[:, :, :, at]), len(spos)
    # another list of lengths cuts the partial sums elsewhere: the shared lengths agree within the bound
    some = sweep(range(W), allp, lengths=[1, 3])
    assert_close(some[0], full[0][:, :, [1, 3]], what=f"{strategy}: lengths [1, 3] alone vs the list of 4")
    assert np.array_equal(some[1], full[1][:, :, [1, 3]])


# ---- 4. isolation -----------------------------------------------------------------------------------------------------
ISO_K, ISO_N, ISO_W = 40, 130, 2
ISO_SIZES = [8, 20, 21, 40]
ISO_ROWS = [50, 60, 90, 129]


def _iso_inputs():
    inp = synthetic.make_kernel_inputs(ISO_K, ISO_N, ISO_W, seed=933000)
    rng = np.random.default_rng(933000)
    Nl = np.asarray(ISO_ROWS, dtype=np.int32) + 1
    rows = np.tile(np.asarray(ISO_ROWS, dtype=np.int32), (ISO_W, 1))
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(ISO_W, 2, len(ISO_ROWS)))
    w0 = prefix_priors(rng, ISO_W, 2, ISO_SIZES, ISO_K)
    delta = rng.normal(0.0, 1e-6, size=(ISO_W, len(ISO_ROWS), inp["n_r"]))
    return inp, Nl, rows, n0, w0, delta


def _iso_sweep(dev, strategy, panel, row_idx, hf_panel=None, with_delta=True):
    inp, Nl, rows, n0, w0, delta = _iso_inputs()
    delta = delta if with_delta else None
    conj = strategy == "conjugate"
    b = dev.batch(strategy, ISO_K, ISO_N, inp["n_r"], GAMMA, ISO_W, inp["m"] if conj else 0)
    if conj:
        b.upload(panel, row_idx=row_idx, hf_panel=inp["hf_panel"] if hf_panel is None else hf_panel, hf_start=inp["hf_start"],
                 w0=inp["w0"], n0=inp["n0"])
        out = b.grid_sweep(ISO_SIZES, Nl, rows, n0, w0, delta=delta)
    else:
        b.upload(panel, row_idx=row_idx)
        out = b.grid_sweep(ISO_SIZES, Nl, rows, delta=delta)
    b.close()
    return out


def _iso_reference(strategy, panel, row_idx, hf_panel, sizes, with_delta=True):
    """The oracle on the prefixes `sizes` of the isolation problem -> weights [W, P', L, len(sizes), k]."""
    inp, Nl, rows, n0, w0, delta = _iso_inputs()
    delta = delta if with_delta else np.zeros_like(delta)
    conj = strategy == "conjugate"
    n_r = inp["n_r"]
    Pn = 2 if conj else 1
    ref = np.zeros((ISO_W, Pn, len(ISO_ROWS), len(sizes), ISO_K))
    for l, r in enumerate(ISO_ROWS):
        ridx = np.zeros((ISO_W, n_r), dtype=np.int64)
        ridx[:, :r] = row_idx[:, n_r - r:]
        adj = np.zeros((ISO_W, n_r))
        adj[:, :r] = delta[:, l, n_r - r:]
        for si, ks in enumerate(sizes):
            s = ISO_SIZES.index(ks)
            cols = np.tile(np.arange(ks, dtype=np.int32), (ISO_W, 1))
            for p in range(Pn):
                kw = dict(start=None, n_r=n_r, row_idx=ridx, n_rows=np.full(ISO_W, r, dtype=np.int32), rf_adj=adj, col_idx=cols)
                if conj:
                    kw.update(hf_panel=hf_panel, hf_start=inp["hf_start"], m=inp["m"], w0=np.ascontiguousarray(w0[:, p, s, :ks]),
                              n0=np.ascontiguousarray(n0[:, p, l]))
                ref[:, p, l, si, :ks] = oracle.posterior_batch(strategy, ks, int(Nl[l]), GAMMA, panel, **kw)[0]
    return ref


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("damage", ["duplicate", "zero", "nan"])
def test_a_column_beyond_a_prefix_never_reaches_it(dev, strategy, damage):
    """Column 20 is in turn a duplicate of column 3, a zero column and a NaN column (daily and intraday panel): at every length
    sizes 8 and 20 stay OK and equal to the oracle on their prefix, sizes 21 and 40 are flagged.  The zero column runs without
    a delta: minus delta it is a small column, not a zero one, and its matrix is not singular."""
    inp = _iso_inputs()[0]
    n_r = inp["n_r"]
    row_idx = (inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32)
    panel, hf = inp["panel"].copy(), inp["hf_panel"].copy()
    for a in (panel, hf):
        a[:, 20] = a[:, 3] if damage == "duplicate" else (0.0 if damage == "zero" else np.nan)
    with_delta = damage != "zero"
    wts, status, _ = _iso_sweep(dev, strategy, panel, row_idx, hf, with_delta)
    assert (status[..., :2] == _native.STATUS_OK).all(), status
    assert (status[..., 2:] != _native.STATUS_OK).all(), status
    if damage != "nan":
        assert (status[..., 2:] == _native.STATUS_NOT_PD).all(), status
    ref = _iso_reference(strategy, panel, row_idx, hf, [8, 20], with_delta)
    for l in range(len(ISO_ROWS)):
        for si, ks in enumerate((8, 20)):
            assert_close(wts[:, :, l, si], ref[:, :, l, si], what=f"{strategy} {damage} rows={ISO_ROWS[l]} k_s={ks}")


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("damage", [np.nan, 1e6])
def test_a_row_older_than_a_suffix_never_reaches_it(dev, strategy, damage):
    """Window 1 reads a damaged row at position n_r - 70: inside segment 2 (the rows of length 90 that length 60 does not have).
    Lengths 50 and 60 are bit for bit those of the clean run at every size; lengths 90 and 129 are flagged (NaN, in the sizes that
    hold the damaged column 7) or changed (outlier)."""
    inp = _iso_inputs()[0]
    n_r = inp["n_r"]
    row_idx = (inp["start"][:, None] + np.arange(n_r)[None, :]).astype(np.int32)
    clean = _iso_sweep(dev, strategy, inp["panel"], row_idx)
    assert (clean[1] == 0).all()
    pos = n_r - 70
    extra = inp["panel"][row_idx[1, pos]].copy()
    extra[7] = damage
    bad_idx = row_idx.copy()
    bad_idx[1, pos] = inp["panel"].shape[0]                # window 1 alone reads the extra row
    hit = _iso_sweep(dev, strategy, np.concatenate([inp["panel"], extra[None, :]], axis=0), bad_idx)
    for c, h in zip(clean, hit):
        assert np.array_equal(c[0], h[0])                  # the other window
        assert np.array_equal(c[1][:, :2], h[1][:, :2])    # lengths 50 and 60 of the damaged window, every size: bit for bit
    assert (hit[1][1][:, :2] == _native.STATUS_OK).all()
    if np.isnan(damage):
        assert (hit[1][1][:, 2:] != _native.STATUS_OK).all(), hit[1]       # (column 7 lies inside every size of the list)
    else:
        assert (np.abs(hit[0][1][:, 2:] - clean[0][1][:, 2:]).max(axis=-1) > 0).all()


def test_jeffreys_entry_of_fewer_rows_than_its_size_is_not_pd_for_that_entry_only(dev):
    k, N, W = 33, 130, 2
    sizes = [3, 16, 33]
    inp = synthetic.make_kernel_inputs(k, N, W, seed=933100)
    Nl = np.array([6, 61, 130], dtype=np.int32)
    rows = np.tile(np.array([5, 60, 129], dtype=np.int32), (W, 1))
    b = jeffreys_batch(dev, inp, k, N, W)
    wts, status, _ = b.grid_sweep(sizes, Nl, rows)
    b.close()
    want = np.zeros((W, 1, 3, 3), dtype=np.int32)
    want[:, :, 0, 1:] = _native.STATUS_NOT_PD              # 5 rows: sizes 16 and 33 are singular, size 3 is not
    assert np.array_equal(status, want), status
    for l in range(3):
        for s, ks in enumerate(sizes):
            if status[0, 0, l, s] == 0:
                ref = np.stack([oracle.jeffreys_window(inp["panel"][inp["start"][w] + inp["n_r"] - rows[w, l]:inp["start"][w] + inp["n_r"], :ks],
                                                       int(Nl[l]), GAMMA) for w in range(W)])
                assert_close(wts[:, 0, l, s, :ks], ref, what=f"rows={rows[0, l]} k_s={ks} next to singular entries")


# ---- 5. the contract; the batch and the other sweeps are left alone -------------------------------------------------------
def test_grid_sweep_contract(dev):
    k, N, W, P = 10, 60, 3, 2
    sizes = [3, 10]
    S = 2
    inp = synthetic.make_kernel_inputs(k, N, W, seed=934000)
    n_r = inp["n_r"]
    rng = np.random.default_rng(934000)
    Nl = np.array([20, 40, 60], dtype=np.int32)
    rows = np.tile(np.array([19, 39, 59], dtype=np.int32), (W, 1))
    L = 3
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(W, P, L))
    w0 = prefix_priors(rng, W, P, sizes, k)
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
    assert code(b, lambda b: b.grid_sweep(sizes, Nl, rows, n0, w0)) == INV                             # not uploaded
    n_rows = np.array([n_r, n_r - 2, n_r], dtype=np.int32)
    b.upload(inp["panel"], start=inp["start"], n_rows=n_rows, hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    rows_ok = np.minimum(rows, n_rows[:, None]).astype(np.int32)
    out = np.empty((W, P, L, S, k))
    assert lib.tp_batch_download_grid_sweep(b._b, ptr(out), None, None) == INV                         # no sweep before it

    def call(n_size=S, sz=sizes, n_len=L, Np=Nl, rp=rows_ok, dp=None, npri=P, n0p=n0, w0p=w0):
        return lib.tp_batch_grid_sweep(b._b, n_size, None if sz is None else iptr(sz), n_len, None if Np is None else iptr(Np),
                                       None if rp is None else iptr(rp), None if dp is None else ptr(dp), npri,
                                       None if n0p is None else ptr(n0p), None if w0p is None else ptr(w0p))

    assert call(n_size=0) == INV and call(sz=None) == INV                                              # n_size < 1, sizes NULL
    big = np.arange(1, 18, dtype=np.int32)
    assert call(n_size=17, sz=big) == INV                                                              # n_size > 16
    for bad in ([0, 10], [3, 3], [10, 3], [3, 11]):                                                    # < 1, not increasing, > k
        assert call(sz=bad) == INV
    assert call(n_len=0) == INV and call(Np=None) == INV and call(rp=None) == INV
    assert call(n_len=17, Np=big, rp=np.tile(big, (W, 1)), n0p=np.ones((W, P, 17))) == INV             # n_len > 16
    for bad in ([0, 40, 60], [20, 20, 60], [40, 20, 60]):                                              # < 1, not strictly increasing
        assert call(Np=bad) == INV
    for w, l, bad in ((0, 0, 0), (2, 2, n_r + 1), (1, 2, n_r - 1), (0, 1, 18)):                        # < 1, > n_w (twice), decreasing
        rb = rows_ok.copy()
        rb[w, l] = bad
        assert call(rp=rb) == INV, (w, l, bad)
    for bad in (np.nan, np.inf):                                                                       # a delta some length reads
        db = delta.copy()
        db[1, 0, n_rows[1] - 1] = bad
        assert call(dp=db) == INV
    assert call(npri=0) == INV and call(n0p=None) == INV and call(w0p=None) == INV
    for bad in (0.0, -1.0, np.nan, np.inf):
        n0b = n0.copy()
        n0b[1, 1, 2] = bad
        assert call(n0p=n0b) == INV
    w0b = w0.copy()
    w0b[2, 0, 0, 2] = np.nan                                                                           # inside the prefix of size 3
    assert call(w0p=w0b) == INV
    # none of them got as far as a launch: there is still nothing to download
    assert lib.tp_batch_download_grid_sweep(b._b, ptr(out), None, None) == INV
    junk_w0 = w0.copy()
    junk_w0[:, :, 0, 3:] = np.nan                                                                      # beyond a prefix: never read
    junk = delta.copy()                                    # positions no length reads may hold anything
    junk[:, 0, :n_r - 2 - 19] = np.nan
    junk[1, :, n_rows[1]:] = np.inf
    a1 = b.grid_sweep(sizes, Nl, rows_ok, n0, w0, delta=delta)
    a2 = b.grid_sweep(sizes, Nl, rows_ok, n0, junk_w0, delta=junk)
    assert (a1[1] == 0).all()
    for x, y in zip(a1, a2):
        assert np.array_equal(x, y)
    tie = rows_ok.copy()
    tie[0, 1] = tie[0, 0]                                                                              # a tie is allowed
    assert (b.grid_sweep(sizes, Nl, tie, n0, w0)[1] == 0).all()
    wts, status, aux = b.grid_sweep(sizes, Nl, rows_ok, n0, w0)
    assert lib.tp_batch_download_grid_sweep(b._b, ptr(out), None, None) == 0 and np.array_equal(out, wts)
    assert lib.tp_batch_download_grid_sweep(b._b, None, None, None) == 0                               # each may be NULL
    # a refused call - sizes, priors, rows and delta, the last to be checked - keeps the results of the last sweep
    rb, db = rows_ok.copy(), delta.copy()
    rb[2, 1] = 0
    db[0, 2, n_r - 1] = np.nan
    assert call(sz=[3, 11]) == INV and call(w0p=w0b) == INV and call(rp=rb) == INV and call(dp=db) == INV
    out[:] = 0
    assert lib.tp_batch_download_grid_sweep(b._b, ptr(out), None, None) == 0 and np.array_equal(out, wts)
    b.close()

    j = dev.batch("jeffreys", k, N, n_r, GAMMA, W, 0)
    j.upload(inp["panel"], start=inp["start"])
    assert code(j, lambda b: b.grid_sweep(sizes, Nl, rows, n0, w0)) == INV                             # Jeffreys with priors
    jcall = lambda npri, n0p, w0p: lib.tp_batch_grid_sweep(j._b, S, iptr(sizes), L, iptr(Nl), iptr(rows), None, npri, n0p, w0p)
    assert jcall(1, None, None) == INV and jcall(0, ptr(n0), None) == INV and jcall(0, None, ptr(w0)) == INV
    assert (j.grid_sweep(sizes, Nl, rows)[1] == 0).all()
    j.close()

    kb = _native.sweep_max_assets() + 1
    bigk = synthetic.make_kernel_inputs(kb, kb + 20, 1, seed=934001)
    g = dev.batch("conjugate", kb, kb + 20, bigk["n_r"], GAMMA, 1, bigk["m"])
    g.upload(bigk["panel"], start=bigk["start"], hf_panel=bigk["hf_panel"], hf_start=bigk["hf_start"], w0=bigk["w0"], n0=bigk["n0"])
    assert code(g, lambda b: b.grid_sweep([kb], [kb + 20], np.full((1, 1), bigk["n_r"], dtype=np.int32), bigk["n0"][:, None, None],
                                          bigk["w0"][:, None, None, :])) == _native.TP_ERR_UNSUPPORTED
    g.close()


def test_grid_sweep_refuses_index_layout_windows_too_long_for_the_gram_pass(dev):
    k, W, n_r, m = 3, 1, 11_000, 20
    rng = np.random.default_rng(934100)
    panel = rng.normal(0.0, 0.01, size=(64, k))
    hf = rng.normal(0.0, 0.001, size=(m, k))
    b = dev.batch("conjugate", k, n_r + 1, n_r, GAMMA, W, m)
    b.upload(panel, row_idx=rng.integers(0, 64, size=(W, n_r)).astype(np.int32), hf_panel=hf, hf_start=np.zeros(W, dtype=np.int64),
             w0=np.full((W, k), 1.0 / k), n0=np.full(W, 100.0))
    with pytest.raises(_native.TangencyError) as e:
        b.grid_sweep([2, 3], [100, n_r + 1], np.array([[99, n_r]], dtype=np.int32), np.full((W, 1, 2), 100.0), np.full((W, 1, 2, k), 1.0 / k))
    assert e.value.code == _native.TP_ERR_UNSUPPORTED
    out = np.empty((W, 1, 2, 2, k))
    assert _native.lib.tp_batch_download_grid_sweep(b._b, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None) == _native.TP_ERR_INVALID
    b.close()


def test_grid_sweep_leaves_the_batch_and_the_other_sweeps_alone(dev):
    k, N, W, P = 20, 60, 4, 2
    sizes = [7, 20]
    inp = synthetic.make_kernel_inputs(k, N, W, seed=935000)
    rng = np.random.default_rng(935000)
    Nl = np.array([30, 60], dtype=np.int32)
    rows = np.tile(np.array([29, 59], dtype=np.int32), (W, 1))
    n0 = Nl[None, None, :] * rng.uniform(1.0, 1.6, size=(W, P, 2))
    w0s = prefix_priors(rng, W, P, sizes, k)
    w0 = np.ascontiguousarray(w0s[:, :, 1])
    b = conjugate_batch(dev, inp, k, N, W)
    b.keep_rhs().keep_posterior()
    first = b.run().download()
    prior = b.prior_sweep(n0[:, :, 1].copy(), w0)
    solve = b.solve_sweep(rhs=rng.normal(size=(W, 2, k)))
    rhs0 = b.download_sweep_rhs()
    size = b.size_sweep(sizes, n0[:, :, 1].copy(), w0s)
    window = b.window_sweep(Nl, rows, n0, w0)
    kept = (b.download_rhs(), b.download_posterior())
    launch = dev.last_launch()
    grid = b.grid_sweep(sizes, Nl, rows, n0, w0s, delta=rng.normal(0.0, 1e-6, size=(W, 2, inp["n_r"])))
    assert (grid[1] == 0).all()
    lib = _native.lib
    assert same(b.download(), first)
    assert same(again(b, lib.tp_batch_download_prior_sweep, *prior), prior)
    assert same(again(b, lib.tp_batch_download_size_sweep, *size), size)
    assert same(again(b, lib.tp_batch_download_window_sweep, *window), window)
    assert same(again(b, lib.tp_batch_download_sweep, *solve), solve)
    assert same(again(b, lib.tp_batch_download_sweep_rhs, rhs0), [rhs0])
    assert same((b.download_rhs(), b.download_posterior()), kept) and dev.last_launch() == launch
    # the other sweeps after it leave the grid sweep's results alone
    b.window_sweep(Nl, rows, n0, w0)
    b.size_sweep(sizes, n0[:, :, 0].copy(), w0s)
    b.run()
    assert same(again(b, lib.tp_batch_download_grid_sweep, *grid), grid)
    b.close()


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_grid_sweep_is_one_timed_step(dev, strategy):
    k, N, W, P = 10, 60, 6, 2
    sizes = [4, 10]
    inp = synthetic.make_kernel_inputs(k, N, W, seed=935100)
    conj = strategy == "conjugate"
    Nl = np.array([30, 60], dtype=np.int32)
    rows = np.tile(np.array([29, 59], dtype=np.int32), (W, 1))
    b = conjugate_batch(dev, inp, k, N, W) if conj else jeffreys_batch(dev, inp, k, N, W)
    pri = (np.full((W, P, 2), 80.0), np.full((W, P, 2, k), 1.0 / k)) if conj else ()
    dev.set_option("sweep_chunk_windows", 2)               # three sub-ranges, still one step
    try:
        dev.region_begin()
        b.grid_sweep(sizes, Nl, rows, *pri, delta=np.full((W, 2, inp["n_r"]), 1e-6))
        dev.region_end()
    finally:
        dev.set_option("sweep_chunk_windows", 0)
    steps = dev.region_steps()
    b.close()
    assert len(steps) == 1 and steps[0] > 0 and dev.last_timing()["kernel_ms"] > 0


# ---- 6. the product path ----------------------------------------------------------------------------------------------
def _spec(strat, k, N, scaling=1):
    return {"weighting_strategy": strat, "size": k, "risk_aversion": 5, "turnover_cost": 15,
            "rebalancing_frequency": "daily", "rolling_window": N, "rolling_window_frequency": "daily",
            "mcm_scaling": scaling, "display_name": f"{strat}_{k}_{N}_{scaling}"}


GRID_SIZES, GRID_WINDOWS = [5, 8, 12], [20, 30, 60]


@pytest.mark.parametrize("names", [("conjugate_hf_vix_vw", "conjugate_hf_epu_ew"), ("jeffreys",)])
def test_calculate_weights_for_grid_equals_spec_by_spec(names, monkeypatch):
    """Business days at rf = 0.02: the lengths have different mean calendar gaps, so the sweep must be given a delta.  The first
    dates are early enough that the longer windows are cut by the start of the data (ties in `rows`)."""
    from incorporating_different_sources_amd import batch, portfolio_calculations as pc
    md, _ = synthetic.make_market_data(n_tickers=14, n_days=130, seed=20240094)
    days = md["stock_prices_df"].index
    dates = [pd.Timestamp(d) for d in days[25:65:4]]
    specs = [_spec(name, k, N, 5 if name.endswith("ew") else 1) for name in names for k in GRID_SIZES for N in GRID_WINDOWS]
    batch.clear_panel_cache()
    plain = [pc._weights_for_dates(dates, sp, md) for sp in specs]
    batch.clear_panel_cache()
    packs, sweeps = [], []
    real_pack, real_sweep = batch.pack_windows_grid, _native.Batch.grid_sweep

    def pack(d, sp, sizes, wins, m, **kw):
        packs.append(real_pack(d, sp, sizes, wins, m, **kw))
        return packs[-1]

    def sweep(self, sizes, N, rows, n0=None, w0=None, delta=None, **kw):
        sweeps.append((list(sizes), list(N), None if n0 is None else n0.shape, None if w0 is None else w0.shape, delta is not None))
        return real_sweep(self, sizes, N, rows, n0, w0, delta=delta, **kw)

    monkeypatch.setattr(batch, "pack_windows_grid", pack)
    monkeypatch.setattr(_native.Batch, "grid_sweep", sweep)
    monkeypatch.setattr(_native.Batch, "window_sweep", lambda *a, **kw: pytest.fail("a window sweep was run"))
    monkeypatch.setattr(_native.Batch, "size_sweep", lambda *a, **kw: pytest.fail("a size sweep was run"))
    shared = pc.calculate_weights_for_grid(dates, specs, md)
    W = len(dates)
    assert len(packs) == 1 and packs[0][5].all()
    rows, delta = packs[0][3], packs[0][4]
    assert (rows[:, :-1] == rows[:, 1:]).any() and (rows[:, :-1] < rows[:, 1:]).any()      # truncated at the first dates only
    assert delta.any()
    conj = names[0] != "jeffreys"
    assert sweeps == [(GRID_SIZES, GRID_WINDOWS, (W, 2, 3) if conj else None, (W, 2, 3, 12) if conj else None, True)]
    for sp, a, b in zip(specs, plain, shared):
        assert b[0].shape == (W, sp["size"])
        assert_close(b[0], a[0], what=sp["display_name"])
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    if conj:           # the backtest calls that follow find the cache filled: no device batch of their own
        monkeypatch.setattr(_native, "posterior_batch", lambda *a, **kw: pytest.fail("the cache was not filled"))
        for sp, res in zip(specs, shared):
            assert pc._weights_for_dates(dates, sp, md)[0] is res[0]
    batch.clear_panel_cache()


def test_calculate_weights_for_grid_serves_masked_triples_spec_by_spec():
    """A late-listed large cap: at one date the shortest window has another universe than the pack, at every size.  Those (date,
    size, length) triples come from `_weights_for_dates` - labels and columns included - and everything else from the sweep."""
    from incorporating_different_sources_amd import batch, portfolio_calculations as pc
    md, _ = synthetic.make_market_data(n_tickers=12, n_days=70, seed=20240093)
    days = md["stock_prices_df"].index
    prices = md["stock_prices_df"].copy()
    big = md["stock_market_caps_df"].loc[days[45]].idxmax()
    prices.loc[prices.index < days[30], big] = np.nan
    md = dict(md, stock_prices_df=prices)
    dates = [pd.Timestamp(d) for d in (days[38], days[45], days[62])]
    sizes, windows = [5, 8], [12, 20, 30]
    specs = [_spec("jeffreys", k, N) for k in sizes for N in windows]
    batch.clear_panel_cache()
    mask = batch.pack_windows_grid(dates, specs[0], sizes, windows, md)[5]
    assert mask.tolist() == [[[True] * 3] * 2, [[False, True, True]] * 2, [[True] * 3] * 2]
    plain = [pc._weights_for_dates(dates, sp, md) for sp in specs]
    shared = pc.calculate_weights_for_grid(dates, specs, md)
    assert big in shared[0][1][1] and big not in shared[1][1][1] and big in shared[3][1][1] and big not in shared[4][1][1]
    for sp, a, b in zip(specs, plain, shared):
        assert_close(b[0], a[0], what=sp["display_name"])
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    batch.clear_panel_cache()
