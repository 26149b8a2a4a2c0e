"""`portfolio_calculations._grid_replay_plan` (no GPU): where every spec of a grid family reads its weights and statuses in a
grid sweep's results [W x P x L x S x k] / [W x P x L x S], which (spec, date) pairs become patches, and the per-spec scale -
on hand-made masks, against a plain restatement with loops over a table that holds every element's own flat index."""
import numpy as np
import pytest

from incorporating_different_sources_amd import portfolio_calculations as pc


def _spec(strat, k, N, gamma=5, scaling=1):
    return {"weighting_strategy": strat, "size": k, "risk_aversion": gamma, "turnover_cost": 15,
            "rebalancing_frequency": "daily", "rolling_window": N, "rolling_window_frequency": "daily",
            "mcm_scaling": scaling, "display_name": f"{strat}_{k}_{N}_{gamma}_{scaling}"}


def _restated(specs, sizes, windows, prior_keys, mask, k):
    """The plan, element by element: flat indices are read out of index tables of the sweep's shapes."""
    W = mask.shape[0]
    P, L, S = max(len(prior_keys), 1), len(windows), len(sizes)
    w_index = np.arange(W * P * L * S * k).reshape(W, P, L, S, k)
    s_index = np.arange(W * P * L * S).reshape(W, P, L, S)
    gammas = {sp["risk_aversion"] for sp in specs}
    rows, patches = [], []
    for i, sp in enumerate(specs):
        scale = 1.0 if len(gammas) == 1 else 1.0 / sp["risk_aversion"]
        if sp["size"] not in sizes:
            rows.append((0, 0, 0, 0, scale, False))
            patches += [(i, j) for j in range(W)]
            continue
        s, l = sizes.index(sp["size"]), windows.index(sp["rolling_window"])
        p = prior_keys.index((sp["weighting_strategy"], sp["mcm_scaling"])) if prior_keys else 0
        w_stride = int(w_index[1, p, l, s, 0] - w_index[0, p, l, s, 0]) if W > 1 else P * L * S * k
        s_stride = int(s_index[1, p, l, s] - s_index[0, p, l, s]) if W > 1 else P * L * S
        rows.append((int(w_index[0, p, l, s, 0]), w_stride, int(s_index[0, p, l, s]), s_stride, scale, True))
        patches += [(i, j) for j in range(W) if not mask[j, s, l]]
    return rows, patches


def _check(specs, sizes, windows, prior_keys, mask, k):
    plan = pc._grid_replay_plan(specs, sizes, windows, prior_keys, mask, k)
    rows, patches = _restated(specs, sizes, windows, prior_keys, mask, k)
    n = len(specs)
    for name, dtype in (("w_off", np.int64), ("w_stride", np.int64), ("s_off", np.int64), ("s_stride", np.int64),
                        ("w_scale", np.float64), ("swept", np.bool_)):
        assert plan[name].shape == (n,) and plan[name].dtype == dtype, name
    assert plan["patch_port"].dtype == np.int64 and plan["patch_date"].dtype == np.int32
    got = list(zip(plan["w_off"].tolist(), plan["w_stride"].tolist(), plan["s_off"].tolist(), plan["s_stride"].tolist(),
                   plan["w_scale"].tolist(), plan["swept"].tolist()))
    assert got == rows
    assert list(zip(plan["patch_port"].tolist(), plan["patch_date"].tolist())) == patches
    assert patches == sorted(set(patches))                                # strictly increasing by (spec, date)
    # every row a spec reads lies inside the source, and rows of different (prior, length, size) never overlap
    W = mask.shape[0]
    P, L, S = max(len(prior_keys), 1), len(windows), len(sizes)
    for i, sp in enumerate(specs):
        last = plan["w_off"][i] + (W - 1) * plan["w_stride"][i] + sp["size"]
        if plan["swept"][i]:
            assert last <= W * P * L * S * k and plan["s_off"][i] + (W - 1) * plan["s_stride"][i] < W * P * L * S
    return plan


def test_jeffreys_grid_with_served_and_unserved_dates():
    sizes, windows, k = [5, 8], [12, 20, 30], 8
    specs = [_spec("jeffreys", ks, N) for ks in sizes for N in windows]
    mask = np.ones((4, 2, 3), dtype=bool)
    mask[1, :, 0] = False                    # date 1: the shortest window is another universe, at every size
    mask[3, 1, 2] = False
    mask[0, 1, 2] = False
    plan = _check(specs, sizes, windows, [], mask, k)
    assert (plan["w_scale"] == 1.0).all() and plan["swept"].all()
    assert list(zip(plan["patch_port"].tolist(), plan["patch_date"].tolist())) == [(0, 1), (3, 1), (5, 0), (5, 3)]
    # the order of the specs is the caller's, not the sweep's
    shuffled = [specs[i] for i in (4, 0, 5, 2, 1, 3)]
    again = _check(shuffled, sizes, windows, [], mask, k)
    assert list(zip(again["patch_port"].tolist(), again["patch_date"].tolist())) == [(1, 1), (2, 0), (2, 3), (5, 1)]


def test_conjugate_priors_and_mixed_risk_aversions():
    sizes, windows, k = [3, 6, 7], [10, 40], 7
    keys = [("conjugate_hf_vix_vw", 1), ("conjugate_hf_epu_ew", 5)]
    specs = [_spec(name, ks, N, gamma, scaling) for (name, scaling), gamma in zip(keys, (3, 7)) for ks in sizes for N in windows]
    specs.append(_spec("conjugate_hf_vix_vw", 6, 40, gamma=1, scaling=1))
    rng = np.random.default_rng(5)
    mask = rng.random((6, 3, 2)) < 0.7
    plan = _check(specs, sizes, windows, keys, mask, k)
    want = [1.0 / 3] * 6 + [1.0 / 7] * 6 + [1.0]
    assert plan["w_scale"].tobytes() == np.array(want).tobytes()          # the host's 1.0 / risk_aversion, to the bit
    assert plan["patch_port"].size == sum(int((~mask[:, sizes.index(sp["size"]), windows.index(sp["rolling_window"])]).sum())
                                          for sp in specs)
    # equal risk aversions: no scale at all
    same = [dict(sp, risk_aversion=4) for sp in specs]
    assert (_check(same, sizes, windows, keys, mask, k)["w_scale"] == 1.0).all()


def test_a_size_outside_the_sweep_is_all_patches():
    sizes, windows, k = [4, 9], [15], 9
    specs = [_spec("jeffreys", 4, 15, gamma=2), _spec("jeffreys", 200, 15, gamma=4), _spec("jeffreys", 9, 15, gamma=2)]
    mask = np.ones((5, 2, 1), dtype=bool)
    mask[2, 1, 0] = False
    plan = _check(specs, sizes, windows, [], mask, k)
    assert plan["swept"].tolist() == [True, False, True]
    assert (plan["w_off"][1], plan["w_stride"][1], plan["s_off"][1], plan["s_stride"][1]) == (0, 0, 0, 0)
    assert plan["w_scale"].tolist() == [0.5, 0.25, 0.5]                   # (a patched row is never scaled; the value is unused)
    assert list(zip(plan["patch_port"].tolist(), plan["patch_date"].tolist())) == [(1, j) for j in range(5)] + [(2, 2)]


def test_one_date_and_no_patch():
    specs = [_spec("jeffreys", 3, 10)]
    plan = _check(specs, [3], [10], [], np.ones((1, 1, 1), dtype=bool), 3)
    assert plan["patch_port"].size == 0 and plan["patch_date"].size == 0
    assert (plan["w_off"][0], plan["w_stride"][0], plan["s_off"][0], plan["s_stride"][0]) == (0, 3, 0, 1)


def test_the_pure_function_needs_no_device(monkeypatch):
    from incorporating_different_sources_amd import _native
    monkeypatch.setattr(_native, "default_device", lambda: pytest.fail("a device was asked for"))
    _check([_spec("jeffreys", 2, 10), _spec("jeffreys", 3, 10)], [2, 3], [10], [], np.array([[[True], [False]]] * 3), 3)
