"""Tiled window sweep (tp_batch_window_sweep_tiled), what can be checked without a GPU.  About the case table
(tests/_window_sweep_tiled_cases.py): for every (case, window, length) the GPU test compares, the oracle and an independent
np.longdouble Cholesky solve of the same system agree within a QUARTER of the bound the GPU test applies - so a miss on the GPU
is the kernel's, not the reference's - and the table has the geometry it is there for.  About the binding: wrong arguments are
rejected before any device call, the symbol is listed and exported.  About calculate_weights_for_windows: its routing with the
WINDOW_SWEEP_TILED switch off and on, with no device."""
import ctypes

import numpy as np
import pytest

from incorporating_different_sources_amd import _native, batch
from oracle import oracle

import _window_sweep_tiled_cases as cases
from test_host_window_sweep_cases import conjugate_ld, jeffreys_ld

LD = np.longdouble


def quarter(got, ref, what):
    b = cases.bound(ref)
    err = float(np.abs(got - ref.astype(LD)).max())
    assert np.isfinite(ref).all() and err <= 0.25 * b, f"{what}: {err:.3e} > a quarter of {b:.3e}"
    return err / b


CONJ = list(cases.problems("conjugate"))
JEFF = [(pr, f) for pr in cases.problems("jeffreys") for f in cases.jeffreys_flags(pr["k"])]


# ---- well-posedness ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pr", CONJ, ids=[pr["id"] for pr in CONJ])
def test_conjugate_oracle_is_good_to_a_quarter_of_the_bound(pr):
    ref, rstat, raux = cases.reference(pr)
    assert (rstat == 0).all()
    worst, worst_aux = 0.0, 0.0
    for w in range(cases.W):
        for l in range(len(pr["N"])):
            X, Y = cases.window_rows(pr, w, l)
            assert X.shape == (pr["rows"][w, l], pr["k"]) and Y.shape[0] > pr["k"]      # m > k: the prior alone is definite
            for p in range(cases.P):
                ld, ald = conjugate_ld(X, Y, pr["w0"][w, p], pr["n0"][w, p, l], int(pr["N"][l]), pr["k"], cases.GAMMA)
                worst = max(worst, quarter(ld, ref[w, p, l], f"{pr['id']} w={w} p={p} rows={pr['rows'][w, l]}"))
                # aux[:6] against the extended-precision values, in units of the GPU test's tolerance
                ra = np.abs(raux[w, p, l, :6].astype(LD) - ald) / (cases.AUX_TOL["atol"] + cases.AUX_TOL["rtol"] * np.abs(ald))
                worst_aux = max(worst_aux, float(ra.max()))
                assert raux[w, p, l, 5] > 0                            # no BAD_DENOM among the cases
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
            assert X.shape[0] >= pr["k"] + 2
            Nw = None if flag == 2 else (X.shape[0] if flag == 1 else int(pr["N"][l]))
            ld, q1_ld = jeffreys_ld(X, Nw, cases.GAMMA)
            worst = max(worst, quarter(ld, ref[w, 0, l], f"{pr['id']} flag={flag} w={w} rows={pr['rows'][w, l]}"))
            # the GPU test's stand-in for q1, gamma t'(the oracle's weights), in units of its tolerance for aux
            q1 = cases.GAMMA * X.sum(axis=0) @ ref[w, 0, l]
            worst_q1 = max(worst_q1, float(abs(LD(q1) - q1_ld) / (cases.AUX_TOL["atol"] + cases.AUX_TOL["rtol"] * abs(q1_ld))))
    print(f"{pr['id']} flag={flag}: worst |oracle - longdouble| = {worst:.2e} of the bound, q1 stand-in {worst_q1:.2e} of its tolerance")
    assert worst_q1 <= 0.25


def test_the_reference_is_the_oracle_on_the_suffix_rows():
    pr = next(p for p in cases.problems("conjugate", ks=[144]) if p["layout"] == "index" and p["delta"] is not None)
    ref, _, _ = cases.reference(pr)
    for w, p, l in ((0, 0, 0), (1, 1, 4), (1, 0, len(pr["N"]) - 1)):
        X, Y = cases.window_rows(pr, w, l)
        wt = oracle.conjugate_window(X, Y, pr["w0"][w, p], float(pr["n0"][w, p, l]), int(pr["N"][l]), pr["k"], cases.GAMMA)
        assert np.array_equal(wt, ref[w, p, l])


# ---- geometry ---------------------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_is_there_for():
    smax = _native.sweep_max_assets()
    assert min(cases.CASES) == smax + 1                                # the first size of the call
    # (NS, super-tile of the border column, its column there)
    assert cases.geometry(144) == (3, 2, 16)
    assert cases.geometry(191) == (3, 2, 63)                           # last column of super-tile 2
    assert cases.geometry(192) == (4, 3, 0)                            # opens a super-tile of its own
    assert cases.geometry(260)[0] == 5
    assert cases.geometry(520)[0] == 9 and cases.geometry(520)[0] > 8  # the three-kernel form of the factorisation
    for k, (N, conj, jeff) in cases.CASES.items():
        assert cases.hf_days(k) * 78 - 1 > k
        for rows0 in conj + jeff:
            assert rows0 == sorted(set(rows0)) and rows0[-1] == N - 1 and len(rows0) <= _native.SWEEP_MAX_RHS
        assert all(rows0[0] >= k + 2 for rows0 in jeff)
        if k <= 260:
            assert all(rows0[0] == 1 for rows0 in conj)
    assert len(cases.LIST16_144) == 16 and len(cases.CASES[520][1][0]) == 3 and len(cases.CASES[520][2][0]) == 3
    seg = np.diff([0] + cases.LIST_144).tolist()
    assert {1, 2, 3, 5} <= set(seg)
    for mod in (4, 12):                                                # on, before and after a multiple: lengths and ends
        assert {0, 1, mod - 1} <= {s % mod for s in seg} and {0, 1, mod - 1} <= {r % mod for r in cases.LIST_144}
    n_r = cases.CASES[144][0] - 1
    tied = cases.rows_table(cases.LIST_144, [n_r, n_r])                # a tie: window 1 shifts a count onto its neighbour
    assert tied[0].tolist() == cases.LIST_144 and tied[1, 0] == tied[1, 1] == 1
    ids = {(pr["k"], pr["layout"], pr["delta"] is not None) for pr in CONJ}
    assert {(k, lay, d) for k in (144, 191, 192, 260) for lay in cases.LAYOUTS for d in (False, True)} | {(520, "contiguous", True)} == ids
    assert sum(pr["k"] == 520 for pr in CONJ) == 1 and sum(pr["k"] == 520 for pr, _ in JEFF) == 1
    assert {f for pr, f in JEFF if pr["k"] == 144} == {0, 1, 2} and {f for pr, f in JEFF if pr["k"] != 144} == {0}
    # the index layout cuts the longest length to the window's own rows
    assert any((pr["rows"][:, -1] < pr["inp"]["n_r"]).any() for pr in CONJ if pr["layout"] == "index")


# ---- the binding ------------------------------------------------------------------------------------------------------
class _NoDevice:
    def _check(self, rc):
        pytest.fail("the binding called into the library")


def _batch(W=3, k=200, n_r=50):
    b = object.__new__(_native.Batch)
    b.dev, b.W, b.k, b.n_r, b._b = _NoDevice(), W, k, n_r, ctypes.c_void_p()
    return b


_ROWS = np.tile(np.array([10, 20], dtype=np.int32), (3, 1))


@pytest.mark.parametrize("N,rows,n0,w0,delta", [
    ([], np.zeros((3, 0), dtype=np.int32), None, None, None),                          # no length
    (list(range(1, 18)), np.ones((3, 17), dtype=np.int32), None, None, None),          # more than 16 lengths
    ([[11, 21]], _ROWS, None, None, None),                                             # N not 1-D
    ([11.0, 21.0], _ROWS, None, None, None),                                           # N not integers
    (None, _ROWS, None, None, None),
    ([11, 21], None, None, None, None),                                                # no rows
    ([11, 21], _ROWS.astype(float), None, None, None),                                 # rows not integers
    ([11, 21], _ROWS[:2], None, None, None),                                           # wrong W
    ([11, 21], _ROWS[:, :1], None, None, None),                                        # wrong L
    ([11, 21], _ROWS, None, None, np.zeros((3, 2, 49))),                               # delta not [W x L x n_r]
    ([11, 21], _ROWS, None, None, np.zeros((3, 2, 50), dtype=complex)),
    ([11, 21], _ROWS, np.ones((3, 2, 2)), None, None),                                 # one of the two priors alone
    ([11, 21], _ROWS, None, np.ones((3, 2, 200)), None),
    ([11, 21], _ROWS, np.ones((3, 2)), np.ones((3, 2, 200)), None),                    # n0 not [W x P x L]
    ([11, 21], _ROWS, np.ones((3, 2, 3)), np.ones((3, 2, 200)), None),                 # L of n0 differs
    ([11, 21], _ROWS, np.ones((2, 2, 2)), np.ones((2, 2, 200)), None),                 # wrong W
    ([11, 21], _ROWS, np.ones((3, 2, 2)), np.ones((3, 2, 199)), None),                 # wrong k
    ([11, 21], _ROWS, np.ones((3, 2, 2)), np.ones((3, 1, 200)), None),                 # P of w0 differs
    ([11, 21], _ROWS, np.ones((3, 2, 2), dtype=complex), np.ones((3, 2, 200)), None),
])
def test_binding_rejects_wrong_arguments_before_any_device_call(N, rows, n0, w0, delta, monkeypatch):
    monkeypatch.setattr(_native.lib, "tp_batch_window_sweep_tiled", lambda *a: pytest.fail("the binding called into the library"), raising=False)
    with pytest.raises(ValueError):
        _batch().window_sweep_tiled(N, rows, n0, w0, delta=delta)


def test_symbol_is_exported_by_the_library_and_listed():
    assert "tp_batch_window_sweep_tiled" in _native.EXPORTS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "tp_batch_window_sweep_tiled")


# ---- the routing of calculate_weights_for_windows ---------------------------------------------------------------------
def _spec(k, N, strat="conjugate_hf_vix_vw"):
    return {"weighting_strategy": strat, "size": k, "risk_aversion": 5, "turnover_cost": 15, "rebalancing_frequency": "daily",
            "rolling_window": N, "rolling_window_frequency": "daily", "mcm_scaling": 1, "display_name": f"{strat}_{k}_{N}"}


def _routed(monkeypatch, k, windows):
    """(window lists the pack was asked for, rolling windows that went through _weights_for_dates); the pack raises, so nothing
    is swept and no device is needed."""
    from incorporating_different_sources_amd import portfolio_calculations as pc
    packs, alone = [], []

    def pack(dates, spec, wins, md, **kw):
        packs.append((spec["size"], list(wins)))
        raise ValueError("no pack in this test")

    monkeypatch.setattr(batch, "pack_windows_lengths", pack)
    monkeypatch.setattr(pc, "_weights_for_dates", lambda d, sp, m: (alone.append(sp["rolling_window"]), (np.zeros((len(d), sp["size"])), [], None, None))[1])
    monkeypatch.setattr(pc, "_fill_spec_cache", lambda sps, d, m, w, n, same, lab, cols, cp: [(w, lab, cols, cp)])
    monkeypatch.setattr(_native, "Batch", lambda *a, **kw: pytest.fail("a device batch was created"))
    out = pc.calculate_weights_for_windows([], [_spec(k, N) for N in windows], {"members_of": None})
    assert len(out) == len(windows)
    return packs, alone


def test_routing_is_unchanged_with_the_switch_off(monkeypatch):
    from incorporating_different_sources_amd import portfolio_calculations as pc
    assert pc.WINDOW_SWEEP_TILED is False                              # off by default
    smax = _native.sweep_max_assets()
    assert _routed(monkeypatch, smax + 1, [30, 60, 90]) == ([], [30, 60, 90])      # above the bound: no pack, every spec alone
    assert _routed(monkeypatch, 500, [250, 125]) == ([], [250, 125])
    assert _routed(monkeypatch, smax, [30, 60]) == ([(smax, [30, 60])], [30, 60])  # (the pack raised: every spec on its own)


def test_switch_on_packs_once_at_the_longest_window(monkeypatch):
    from incorporating_different_sources_amd import portfolio_calculations as pc
    monkeypatch.setattr(pc, "WINDOW_SWEEP_TILED", True)
    smax = _native.sweep_max_assets()
    packs, alone = _routed(monkeypatch, smax + 1, [60, 30, 90])
    assert packs == [(smax + 1, [30, 60, 90])] and alone == [60, 30, 90]           # ONE pack; it ends at the longest window
    assert _routed(monkeypatch, 500, [250, 125])[0] == [(500, [125, 250])]
    assert _routed(monkeypatch, smax, [30, 60])[0] == [(smax, [30, 60])]           # within the LDS sweep: as with the switch off
    many = list(range(30, 30 + _native.SWEEP_MAX_RHS + 1))                         # more lengths than one sweep holds: the old route
    assert _routed(monkeypatch, 500, many) == ([], many)
