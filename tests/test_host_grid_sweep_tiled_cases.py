"""Tiled grid sweep (tp_batch_grid_sweep_tiled), what can be checked without a GPU.  About the case table
(tests/_grid_sweep_tiled_cases.py): for every (case, window, prior, length, size) the GPU test compares, the oracle on the suffix
rows and prefix columns and an independent np.longdouble Cholesky solve of the same system agree within a QUARTER of the bound
the GPU test applies - so a miss on the GPU is the kernel's, not the reference's - and the table has the geometry it is there
for.  No entry is skipped; no case had to move.  The extended-precision matrix is factorised once per (window, prior, length) and
every size solved on its leading block.  About the binding: wrong arguments are rejected before any device call, the
symbol is listed and exported.  About calculate_weights_for_grid: its routing with the GRID_SWEEP_TILED switch off and on, with
no device."""
import ctypes

import numpy as np
import pytest

from incorporating_different_sources_amd import _native, batch
from oracle import oracle

import _grid_sweep_tiled_cases as cases
from test_host_window_sweep_cases import LD, conjugate_ld, jeffreys_ld

CONJ = cases.problems("conjugate")
JEFF = [(pr, f) for pr in cases.problems("jeffreys") for f in cases.jeffreys_flags(pr["k"])]


def quarter(got, ref, what):
    b = cases.bound(ref)
    err = float(np.abs(got - ref.astype(LD)).max())
    assert np.isfinite(ref).all() and err <= 0.25 * b, f"{what}: {err:.3e} > a quarter of {b:.3e}"
    return err / b


# The extended-precision solve of a prefix system.  The leading k_s x k_s block of S1 (of J) at the largest size IS the matrix of
# the universe of size k_s over the same rows, and the Cholesky factor of a leading block is the leading block of the factor: the
# matrix is formed and factorised ONCE per (window, prior, length) in np.longdouble and every size solved on its own leading
# block with its own right-hand side - the arithmetic per size is test_host_window_sweep_cases.conjugate_ld / jeffreys_ld's.
def chol_factor(A):
    n = A.shape[0]
    Lm = np.zeros((n, n), dtype=LD)
    A = A.copy()
    for j in range(n):
        d = np.sqrt(A[j, j])
        Lm[j:, j] = A[j:, j] / d
        A[j + 1:, j + 1:] -= np.outer(Lm[j + 1:, j], Lm[j + 1:, j])
    return Lm


def prefix_solve(Lm, b, ks):
    y = np.zeros(ks, dtype=LD)
    for i in range(ks):
        y[i] = (b[i] - Lm[i, :i] @ y[:i]) / Lm[i, i]
    x = np.zeros(ks, dtype=LD)
    for i in range(ks - 1, -1, -1):
        x[i] = (y[i] - Lm[i + 1:ks, i] @ x[i + 1:]) / Lm[i, i]
    return x


def test_the_shared_factor_solves_what_the_window_tests_solve():
    """One factorisation at k, prefix solves on its leading blocks: the numbers of conjugate_ld / jeffreys_ld on the prefix."""
    rng = np.random.default_rng(5)
    X, Y, w0 = rng.normal(size=(40, 9)), rng.normal(size=(30, 9)), rng.dirichlet(np.ones(6))
    ld, ald = conjugate_ld(X[:, :6], Y[:, :6], w0, 55.0, 41, 6, 5.0)
    C, T, t = _scatter(Y), X.astype(LD).T @ X.astype(LD), X.astype(LD).sum(axis=0)
    got, aux = _conjugate_prefix(C, 30, T, t, chol_factor(_s0(C, 30, LD(55.0)) + T), w0, LD(55.0), 41, 6, 5.0)
    assert float(np.abs(got - ld).max()) < 1e-17 and float(np.abs(aux - ald).max()) < 1e-15 * float(np.abs(ald).max())
    jl, q1 = jeffreys_ld(X[:, :6], 41, 5.0)
    J = T - np.outer(t, t) / LD(41)
    x = prefix_solve(chol_factor(J), t, 6)
    assert float(np.abs(x / LD(5.0) - jl).max()) < 1e-17 and abs(float(t[:6] @ x - q1)) < 1e-17


def _scatter(Y):
    Yc = Y.astype(LD) - Y.astype(LD).mean(axis=0)
    return Yc.T @ Yc


def _s0(C, m, n0):
    return n0 * (C / LD(m - 1) * LD(m))


def _conjugate_prefix(C, m, T, t, Lm, w0, n0, N, ks, gamma):
    """ref:819-836 in np.longdouble on the leading block -> (weights, aux[:6]); Lm: the factor of S0 + T at the largest size."""
    w0 = w0.astype(LD)
    S0 = _s0(C[:ks, :ks], m, n0)
    v = S0 @ w0
    q0 = w0 @ v
    a = n0 + ks + 2
    c = 2 * n0 / (a + np.sqrt(a * a + 4 * n0 * q0))
    w1 = prefix_solve(Lm, c * v + t[:ks], ks)
    n1 = n0 + N
    q1 = w1 @ ((S0 + T[:ks, :ks]) @ w1)
    return (n1 + ks + 2) * w1 / (n1 - q1) / LD(gamma), np.array([n0, n1, c, q0, q1, n1 - q1], dtype=LD)


# ---- well-posedness ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pr", CONJ, ids=[pr["id"] for pr in CONJ])
def test_conjugate_oracle_is_good_to_a_quarter_of_the_bound(pr):
    ref, rstat, raux = cases.reference(pr)
    assert (rstat == 0).all()
    worst, worst_aux = 0.0, 0.0
    for w in range(cases.W):
        C = None
        for l in range(len(pr["N"])):
            X, Y = cases.window_rows(pr, w, l)
            assert X.shape == (pr["rows"][w, l], pr["k"]) and Y.shape[0] > pr["k"]      # m > k: the prior alone is definite
            m = Y.shape[0]
            C = _scatter(Y) if C is None else C                        # the intraday rows do not depend on the length
            Xl = X.astype(LD)
            T, t = Xl.T @ Xl, Xl.sum(axis=0)
            for p in range(pr["P"]):
                n0, N = LD(float(pr["n0"][w, p, l])), int(pr["N"][l])
                Lm = chol_factor(_s0(C, m, n0) + T)
                for s, ks in enumerate(pr["sizes"]):
                    wt = ref[w, p, l, s, :ks]
                    assert not ref[w, p, l, s, ks:].any()
                    ld, ald = _conjugate_prefix(C, m, T, t, Lm, pr["w0g"][w, p, s, :ks], n0, N, ks, cases.GAMMA)
                    worst = max(worst, quarter(ld, wt, f"{pr['id']} w={w} p={p} rows={pr['rows'][w, l]} k_s={ks}"))
                    ra = np.abs(raux[w, p, l, s, :6].astype(LD) - ald) / (cases.AUX_TOL["atol"] + cases.AUX_TOL["rtol"] * np.abs(ald))
                    worst_aux = max(worst_aux, float(ra.max()))
                    assert raux[w, p, l, s, 5] > 0                     # no BAD_DENOM among the cases
    print(f"{pr['id']}: worst |oracle - longdouble| = {worst:.2e} of the bound, aux {worst_aux:.2e} of its tolerance")
    assert worst_aux <= 0.25


@pytest.mark.parametrize("pr,flag", JEFF, ids=[f"{pr['id']}-flag{f}" for pr, f in JEFF])
def test_jeffreys_oracle_is_good_to_a_quarter_of_the_bound(pr, flag):
    ref, rstat, _ = cases.reference(pr, flag)
    assert (rstat == 0).all()
    worst, worst_q1 = 0.0, 0.0
    for w in range(cases.W):
        for l in range(len(pr["N"])):
            X, _ = cases.window_rows(pr, w, l)
            assert X.shape[0] >= pr["k"] + 16 - w                     # (window w has w rows fewer than the list says)
            Nw = None if flag == 2 else (X.shape[0] if flag == 1 else int(pr["N"][l]))
            Xl = X.astype(LD)
            T, t = Xl.T @ Xl, Xl.sum(axis=0)
            Lm = chol_factor(T - np.outer(t, t) / LD(Nw) if Nw is not None else T)
            for s, ks in enumerate(pr["sizes"]):
                wt = ref[w, 0, l, s, :ks]
                assert not ref[w, 0, l, s, ks:].any()
                x = prefix_solve(Lm, t, ks)
                ld, q1_ld = x / LD(cases.GAMMA), t[:ks] @ x
                worst = max(worst, quarter(ld, wt, f"{pr['id']} flag={flag} w={w} rows={pr['rows'][w, l]} k_s={ks}"))
                # the GPU test's stand-in for q1, gamma t'(the oracle's weights), in units of its tolerance for aux
                q1 = cases.GAMMA * X[:, :ks].sum(axis=0) @ wt
                worst_q1 = max(worst_q1, float(abs(LD(q1) - q1_ld) / (cases.AUX_TOL["atol"] + cases.AUX_TOL["rtol"] * abs(q1_ld))))
    print(f"{pr['id']} flag={flag}: worst |oracle - longdouble| = {worst:.2e} of the bound, q1 stand-in {worst_q1:.2e} of its tolerance")
    assert worst_q1 <= 0.25


def test_the_reference_is_the_oracle_on_the_suffix_rows_and_prefix_columns():
    pr = next(p for p in cases.problems("conjugate", ks=[260]) if p["layout"] == "index" and p["delta"] is not None)
    ref, _, _ = cases.reference(pr)
    for w, p, l, s in ((0, 0, 0, 0), (1, 1, 3, 2), (1, 0, len(pr["N"]) - 1, len(pr["sizes"]) - 1)):
        X, Y = cases.window_rows(pr, w, l)
        ks = pr["sizes"][s]
        wt = oracle.conjugate_window(np.ascontiguousarray(X[:, :ks]), np.ascontiguousarray(Y[:, :ks]), pr["w0g"][w, p, s, :ks],
                                     float(pr["n0"][w, p, l]), int(pr["N"][l]), ks, cases.GAMMA)
        assert np.array_equal(wt, ref[w, p, l, s, :ks])


# ---- geometry ---------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_is_there_for():
    smax = _native.sweep_max_assets()
    assert min(cases.SIZES) == smax + 1 and sorted(cases.SIZES) == sorted(cases.wcases.CASES)
    # (KP, NS, NSB, super-tiles of the right-hand-side columns)
    assert cases.geometry(144, 7) == (192, 3, 3, [2])
    assert cases.geometry(144, 16) == (192, 3, 3, [2])
    assert cases.geometry(191, 1) == (192, 3, 3, [2]) and 191 == 192 - 1       # the arena's last column
    assert cases.geometry(191, 2) == (256, 4, 3, [2, 3])                       # the right-hand sides straddle two super-tiles
    assert cases.geometry(192, 3) == (256, 4, 3, [3])                          # a super-tile of their own
    assert cases.geometry(260, 6)[1] == 5
    assert cases.geometry(520, 3)[1] == 9                                      # above 8 super-tiles per side: the unfused block steps
    for k, lists in cases.SIZES.items():
        for sizes in lists:
            assert sizes == sorted(set(sizes)) and sizes[0] >= 1 and sizes[-1] == k
    s144 = cases.SIZES[144][0]
    assert {1, 63, 64, 65, 128, smax, smax + 1} <= set(s144)
    assert len(cases.SIZES16_144) == 16 and cases.SIZES16_144 == sorted(set(cases.SIZES16_144))
    assert {1, 64, 65, 143, 144} <= set(cases.SIZES16_144)
    assert any(ks <= smax for ks in cases.SIZES[260][0]) and any(ks > smax for ks in cases.SIZES[260][0][:-1])
    conj, jeff = cases.problems("conjugate"), cases.problems("jeffreys")
    big = [pr for pr in conj if len(pr["sizes"]) == 16]
    assert len(big) == 1 and big[0]["P"] == 1 and big[0]["rows0"] == cases.LIST16_144 and len(big[0]["N"]) == 16
    assert big[0]["layout"] == "index" and big[0]["delta"] is not None and big[0]["w0g"].shape == (cases.W, 1, 16, 144)
    first = [pr for pr in conj if pr["k"] == 144 and len(pr["sizes"]) == 7]
    assert len(first) == 6 and all(pr["rows0"] == cases.LIST_144[:6] + cases.LIST_144[-2:] for pr in first)
    ids = {(pr["k"], len(pr["sizes"]), pr["layout"], pr["delta"] is not None) for pr in conj}
    want = {(k, S, lay, d) for k, S in ((144, 7), (191, 2), (191, 1), (192, 3), (260, 6)) for lay in cases.wcases.LAYOUTS for d in (False, True)}
    assert ids == want | {(144, 16, "index", True), (520, 3, "contiguous", True)}
    assert {(pr["k"], len(pr["sizes"]), pr["layout"], pr["delta"] is not None) for pr in jeff} == want | {(520, 3, "contiguous", True)}
    assert {f for pr, f in JEFF if pr["k"] == 144} == {0, 1, 2} and {f for pr, f in JEFF if pr["k"] != 144} == {0}
    assert all(len(pr["N"]) == 3 for pr in conj + jeff if pr["k"] == 520)
    for pr in conj + jeff:
        assert pr["w0g"].shape == (cases.W, pr["P"], len(pr["sizes"]), pr["k"]) and pr["n0"].shape == (cases.W, pr["P"], len(pr["N"]))
        assert pr["rows"].shape == (cases.W, len(pr["N"])) and (pr["delta"] is None or pr["delta"].shape[:2] == pr["rows"].shape)
        for s, ks in enumerate(pr["sizes"]):
            assert not pr["w0g"][:, :, s, ks:].any() and np.allclose(pr["w0g"][:, :, s].sum(axis=-1), 1.0)
    for pr in jeff:
        # rows to spare at the largest size, hence at every size (window 1 has one row fewer than the list says)
        assert pr["rows0"][0] >= pr["k"] + 16 and (pr["rows"] >= pr["k"] + 15).all()


# ---- the binding ------------------------------------------------------------------------------------------------------
class _NoDevice:
    def _check(self, rc):
        pytest.fail("the binding called into the library")


def _batch(W=3, k=200, n_r=50):
    b = object.__new__(_native.Batch)
    b.dev, b.W, b.k, b.n_r, b._b = _NoDevice(), W, k, n_r, ctypes.c_void_p()
    return b


_ROWS = np.tile(np.array([10, 20], dtype=np.int32), (3, 1))
_SZ = [100, 200]


@pytest.mark.parametrize("sizes,N,rows,n0,w0,delta", [
    ([], [11, 21], _ROWS, None, None, None),                                                   # no size
    (list(range(1, 18)), [11, 21], _ROWS, None, None, None),                                   # more than 16 sizes
    ([100.0, 200.0], [11, 21], _ROWS, None, None, None),                                       # sizes not integers
    (None, [11, 21], _ROWS, None, None, None),
    ([100, 100], [11, 21], _ROWS, None, None, None),                                           # not strictly increasing
    ([0, 200], [11, 21], _ROWS, None, None, None),                                             # below 1
    ([100, 201], [11, 21], _ROWS, None, None, None),                                           # above k
    (_SZ, [], np.zeros((3, 0), dtype=np.int32), None, None, None),                             # no length
    (_SZ, list(range(1, 18)), np.ones((3, 17), dtype=np.int32), None, None, None),             # more than 16 lengths
    (_SZ, [11.0, 21.0], _ROWS, None, None, None),                                              # N not integers
    (_SZ, [11, 21], None, None, None, None),                                                   # no rows
    (_SZ, [11, 21], _ROWS[:2], None, None, None),                                              # wrong W
    (_SZ, [11, 21], _ROWS[:, :1], None, None, None),                                           # wrong L
    (_SZ, [11, 21], _ROWS, None, None, np.zeros((3, 2, 49))),                                  # delta not [W x L x n_r]
    (_SZ, [11, 21], _ROWS, np.ones((3, 2, 2)), None, None),                                    # one of the two priors alone
    (_SZ, [11, 21], _ROWS, np.ones((3, 2)), np.ones((3, 2, 2, 200)), None),                    # n0 not [W x P x L]
    (_SZ, [11, 21], _ROWS, np.ones((3, 2, 2)), np.ones((3, 2, 200)), None),                    # w0 not [W x P x S x k]
    (_SZ, [11, 21], _ROWS, np.ones((3, 2, 2)), np.ones((3, 2, 3, 200)), None),                 # S of w0 differs
    (_SZ, [11, 21], _ROWS, np.ones((3, 2, 2)), np.ones((3, 2, 2, 199)), None),                 # wrong k
    (_SZ, [11, 21], _ROWS, np.ones((3, 2, 2), dtype=complex), np.ones((3, 2, 2, 200)), None),
])
def test_binding_rejects_wrong_arguments_before_any_device_call(sizes, N, rows, n0, w0, delta, monkeypatch):
    monkeypatch.setattr(_native.lib, "tp_batch_grid_sweep_tiled", lambda *a: pytest.fail("the binding called into the library"), raising=False)
    with pytest.raises(ValueError):
        _batch().grid_sweep_tiled(sizes, N, rows, n0, w0, delta=delta)


def test_symbol_is_exported_by_the_library_and_listed():
    assert "tp_batch_grid_sweep_tiled" in _native.EXPORTS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "tp_batch_grid_sweep_tiled")


# ---- the routing of calculate_weights_for_grid ------------------------------------------------------------------------
def _spec(k, N, strat="conjugate_hf_vix_vw"):
    return {"weighting_strategy": strat, "size": k, "risk_aversion": 5, "turnover_cost": 15, "rebalancing_frequency": "daily",
            "rolling_window": N, "rolling_window_frequency": "daily", "mcm_scaling": 1, "display_name": f"{strat}_{k}_{N}"}


def _routed(monkeypatch, sizes, windows):
    """((sizes, windows) the pack was asked for, (size, window) pairs that went through _weights_for_dates); the pack raises, so
    nothing is swept and no device is needed."""
    from incorporating_different_sources_amd import portfolio_calculations as pc
    packs, alone = [], []

    def pack(dates, spec, szs, wins, md, **kw):
        packs.append((list(szs), list(wins)))
        raise ValueError("no pack in this test")

    monkeypatch.setattr(batch, "pack_windows_grid", pack)
    monkeypatch.setattr(pc, "_weights_for_dates",
                        lambda d, sp, m: (alone.append((sp["size"], sp["rolling_window"])), (np.zeros((len(d), sp["size"])), [], None, None))[1])
    monkeypatch.setattr(pc, "_fill_spec_cache", lambda sps, d, m, w, n, same, lab, cols, cp: [(w, lab, cols, cp)])
    monkeypatch.setattr(_native, "Batch", lambda *a, **kw: pytest.fail("a device batch was created"))
    specs = [_spec(k, N) for k in sizes for N in windows]
    out = pc.calculate_weights_for_grid([], specs, {"members_of": None})
    assert len(out) == len(specs)
    return packs, alone


def test_routing_is_unchanged_with_the_switch_off(monkeypatch):
    from incorporating_different_sources_amd import portfolio_calculations as pc
    assert pc.GRID_SWEEP_TILED is False                                # off by default
    smax = _native.sweep_max_assets()
    every = lambda sizes, wins: [(k, N) for k in sizes for N in wins]
    assert _routed(monkeypatch, [100, 500], [60, 30]) == ([([100], [30, 60])], every([100, 500], [60, 30]))    # 500 is not packed
    assert _routed(monkeypatch, [smax + 1, 500], [30]) == ([], every([smax + 1, 500], [30]))                  # nothing to pack
    assert _routed(monkeypatch, [50, smax], [30, 60])[0] == [([50, smax], [30, 60])]


def test_switch_on_packs_every_size_once_at_the_largest(monkeypatch):
    from incorporating_different_sources_amd import portfolio_calculations as pc
    monkeypatch.setattr(pc, "GRID_SWEEP_TILED", True)
    smax = _native.sweep_max_assets()
    packs, alone = _routed(monkeypatch, [500, 100], [60, 30])
    assert packs == [([100, 500], [30, 60])] and len(alone) == 4               # ONE pack, the sizes below the bound in it
    assert _routed(monkeypatch, [smax + 1], [30])[0] == [([smax + 1], [30])]
    assert _routed(monkeypatch, [50, smax], [30, 60])[0] == [([50, smax], [30, 60])]           # within the LDS sweep: as with the switch off
    many = list(range(30, 30 + _native.SWEEP_MAX_RHS + 1))                     # more lengths than one sweep holds: the old route
    assert _routed(monkeypatch, [100, 500], many)[0] == []
    wide = list(range(200, 200 + _native.SWEEP_MAX_RHS + 1))                   # more sizes than one sweep holds: the sizes <= 143 alone
    assert _routed(monkeypatch, [100] + wide, [30])[0] == [([100], [30])]
    top = _native.max_assets()
    assert _routed(monkeypatch, [100, top], [30])[0] == [([100], [30])]                        # largest + S > max_assets() + 1
    assert _routed(monkeypatch, [100, top - 1], [30])[0] == [([100, top - 1], [30])]           # largest + S = max_assets() + 1: fits
