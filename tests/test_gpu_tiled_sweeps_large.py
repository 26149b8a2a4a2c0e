"""The tiled sweeps (tp_batch_prior_sweep_tiled, tp_batch_solve_sweep_tiled) over the whole range they are documented for,
up to k + R = 2048, against the fp64 oracle: tests/test_gpu_prior_sweep_tiled.py and tests/test_gpu_solve_sweep_tiled.py stop at
k = 300, five super-tiles per side.  Reached only here: the unfused block steps as the AUTOMATIC choice (NS > 8) and every
other form above the switch, a sweep and a run at the same k on different forms (k = 510), the back substitution of the solve
sweep with more than 64 KiB of dynamic LDS (KP = 2048, R >= 4), ws.part and the border sums at NS up to 32, the C pass over
1715 intraday rows, and sub-ranges that the 256 MiB bound cuts by itself.  Cases, references and bounds:
tests/_tiled_sweep_cases.py; tests/test_host_tiled_sweep_cases.py shows on the CPU that every reference here is good to a
tenth of its bound.  -m gpu.

Every test goes through all its checks, prints the worst |got - ref| per group next to its bound, and fails at the end if any
check missed."""
import numpy as np
import pytest

from incorporating_different_sources_amd import _native, synthetic
from oracle import oracle

import _tiled_sweep_cases as cases

pytestmark = pytest.mark.gpu

GAMMA = cases.GAMMA
W = cases.W
RUN_TOL = 2e-10                         # a single sweep column against set_rhs + set_shift + run (tests/test_gpu_solve_sweep.py)
SWEEP_WORKSPACE_BYTES = 256 << 20       # TP_SWEEP_WORKSPACE_BYTES of csrc/tangency_sweep.cpp: kept matrices of one sub-range
# {tiled_wave, tiled_fuse}: one-wave / four-wave diagonal-block kernels x automatic / three-kernel / fused update + solve
FORMS = {"auto": {}, "wave0": {"tiled_wave": 0}, "fuse0": {"tiled_fuse": 0}, "wave0-fuse0": {"tiled_wave": 0, "tiled_fuse": 0},
         "fuse1": {"tiled_fuse": 1}}
# above the switch (NS > 8) the automatic update is the three-kernel one: the same launches, so the same bits
SAME_LAUNCHES = (("auto", "fuse0"), ("wave0", "wave0-fuse0"))
IDS = {name: [cases.case_id(c) for c in getattr(cases, name)] for name in ("JEFFREYS_SOLVE", "CONJUGATE_SOLVE", "PRIOR")}


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


def test_flag_value_of_the_helper_is_the_librarys():
    assert cases.FLAG_NO_CENTER == _native.FLAG_NO_CENTER


class Checks:
    """Collects every comparison of one test: the worst error-to-bound ratio per group for the printout, the misses for
    the assertion at the end (tests/test_gpu_run_options.py)."""

    def __init__(self, title):
        self.title, self.worst, self.missed = title, {}, []

    def that(self, ok, what):
        if not ok:
            self.missed.append(what)

    def close(self, group, got, ref, bound, what):
        """max |got - ref| <= bound."""
        err = float(np.abs(got - ref).max()) if np.isfinite(got).all() else np.inf
        if group not in self.worst or err / bound > self.worst[group][0] / self.worst[group][1]:
            self.worst[group] = (err, bound, f"{what}, |ref|.max() = {float(np.abs(ref).max()):.3e}")
        self.that(err <= bound, f"{what}: |got - ref| = {err:.3e} > {bound:.3e}")

    def solution(self, group, got, ref, what, tol=cases.SOL_TOL):
        self.close(group, got, ref, tol * max(1.0, float(np.abs(ref).max())), what)

    def kept_rhs(self, group, got, ref, what):
        self.close(group, got, ref, cases.rhs_bound(ref), what)

    def aux(self, group, got, ref, what):
        """numpy.testing.assert_allclose(got, ref, **AUX_TOL), reported in units of atol + rtol |ref|."""
        worst = cases.aux_ratio(got, ref) if np.isfinite(got).all() else np.inf
        if group not in self.worst or worst > self.worst[group][0]:
            self.worst[group] = (worst, 1.0, what + " (in units of atol + rtol |ref|)")
        self.that(worst <= 1.0, f"{what}: {worst:.3e} x (atol + rtol |ref|), {cases.AUX_TOL}")

    def finish(self):
        for group, (err, bound, what) in self.worst.items():
            print(f"{self.title} [{group}]: worst |got - ref| = {err:.3e} (bound {bound:.3e}) at {what}")
        assert not self.missed, f"{len(self.missed)} checks missed:\n" + "\n".join(self.missed[:40])


class options:
    """dev.set_option for the body of a `with`, taken back whatever happens (`reset`: the option's automatic value)."""

    def __init__(self, dev, values, reset=-1):
        self.dev, self.values, self.reset = dev, values, reset

    def __enter__(self):
        for name, value in self.values.items():
            self.dev.set_option(name, value)

    def __exit__(self, *exc):
        for name in self.values:
            self.dev.set_option(name, self.reset)


def jeffreys_sweep(dev, c, no_center):
    """(x [W, S, R, k], status [W, S], kept t [W, k]) of a Jeffreys solve-sweep case."""
    b = dev.batch("jeffreys", c["k"], c["N"], c["n_r"], GAMMA, W, 0, _native.FLAG_NO_CENTER if no_center else 0)
    try:
        b.upload(c["panel"], **c["upload"])
        x, status = b.solve_sweep_tiled(shift=c["shift"], rhs=c["rhs"] if c["R"] > 1 else None)
        return x, status, b.download_sweep_rhs()
    finally:
        b.close()


def prior_sweep(dev, c, flags=0):
    b = dev.batch("conjugate", c["k"], c["N"], c["n_r"], GAMMA, c["n0"].shape[0], c["m"], flags)
    try:
        b.upload(c["panel"], **c["upload"])
        return b.prior_sweep_tiled(c["n0"], c["w0"])
    finally:
        b.close()


def check_jeffreys(chk, group, got, ref, c, what):
    x, status, t = got
    k, R = c["k"], c["R"]
    chk.that(x.shape == (W, cases.S, R, k) and status.shape == (W, cases.S), f"{what}: shapes {x.shape}, {status.shape}")
    chk.that((status == _native.STATUS_OK).all(), f"{what}: status {status.tolist()}")
    chk.solution(group, x, ref["x"], what)
    chk.kept_rhs(group + " kept rhs", t, ref["t"], f"{what} kept t")


def check_prior(chk, group, got, ref, c, what):
    wts, status, aux = got
    chk.that(wts.shape == ref["weights"].shape and aux.shape[-1] == 8, f"{what}: shapes {wts.shape}, {aux.shape}")
    chk.that((status == _native.STATUS_OK).all(), f"{what}: status {status.tolist()}")
    chk.solution(group, wts, ref["weights"], what)
    chk.aux(group + " aux", aux[..., :6], ref["aux"], f"{what} aux")
    chk.that(np.array_equal(aux[..., 0], c["n0"]), f"{what}: aux[0] is not the caller's n0")


# ---- 1. against the references ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_center", [False, True], ids=["centred", "no_center"])
@pytest.mark.parametrize("k,R,layouts", cases.JEFFREYS_SOLVE, ids=IDS["JEFFREYS_SOLVE"])
def test_jeffreys_tiled_solve_sweep_matches_reference(dev, k, R, layouts, no_center):
    chk = Checks(f"jeffreys solve sweep k={k} R={R} {'no_center' if no_center else 'centred'}")
    for layout in layouts:
        c = cases.jeffreys_solve_case(k, R, layout)
        check_jeffreys(chk, "solutions", jeffreys_sweep(dev, c, no_center), cases.jeffreys_solve_reference(k, R, layout, no_center),
                       c, f"k={k} R={R} {layout}")
    chk.finish()


@pytest.mark.parametrize("k,N,hf_days,R", cases.CONJUGATE_SOLVE, ids=IDS["CONJUGATE_SOLVE"])
def test_conjugate_tiled_solve_sweep_matches_reference(dev, k, N, hf_days, R):
    chk = Checks(f"conjugate solve sweep k={k} N={N} hf_days={hf_days} R={R}")
    c, ref = cases.conjugate_solve_case(k, N, hf_days, R), cases.conjugate_solve_reference(k, N, hf_days, R)
    b = dev.batch("conjugate", k, N, c["n_r"], GAMMA, W, c["m"])
    try:
        b.upload(c["panel"], **c["upload"])
        x, status = b.solve_sweep_tiled(rhs=c["rhs"])
        b0 = b.download_sweep_rhs()
    finally:
        b.close()
    chk.that(x.shape == (W, 1, R, k) and (status == _native.STATUS_OK).all(), f"shape {x.shape}, status {status.tolist()}")
    chk.solution("solutions", x, ref["x"], f"k={k}")
    chk.kept_rhs("kept rhs", b0, ref["b0"], f"k={k} kept c S0 w0 + t")
    chk.finish()


@pytest.mark.parametrize("k,N,hf_days,layouts", cases.PRIOR, ids=IDS["PRIOR"])
def test_tiled_prior_sweep_matches_reference(dev, k, N, hf_days, layouts):
    chk = Checks(f"prior sweep k={k} N={N} hf_days={hf_days}")
    for layout in layouts:
        c = cases.prior_case(k, N, hf_days, layout)
        check_prior(chk, "weights", prior_sweep(dev, c), cases.prior_reference(k, N, hf_days, layout), c, f"k={k} {layout}")
    chk.finish()


# ---- 2. every block-step form above the switch -------------------------------------------------------------------------
def test_every_block_step_form_carries_16_rhs_columns_above_the_switch():
    """(575, R = 16): NS = 10 > 8, so the automatic update is the three-kernel one, which the small-size tests reach only by
    option; the fused one (tiled_fuse = 1) runs above the size the automatic rule gives it."""
    k, R = 575, 16
    c, ref = cases.jeffreys_solve_case(k, R, "contiguous"), cases.jeffreys_solve_reference(k, R, "contiguous", True)
    chk = Checks(f"block-step forms, jeffreys solve sweep k={k} R={R}")
    got = {}
    with _native.Device(0) as own:                       # the forms are options of the handle: a handle of the test's own
        for form, values in FORMS.items():
            with options(own, values):
                got[form] = jeffreys_sweep(own, c, True)
            check_jeffreys(chk, form, got[form], ref, c, f"k={k} R={R} {form}")
    for a, b in SAME_LAUNCHES:
        chk.that(all(np.array_equal(x, y) for x, y in zip(got[a], got[b])), f"{a} and {b} differ: not the same launches")
    chk.finish()


def test_every_block_step_form_of_the_prior_sweep_above_the_switch():
    """(512, 260, 5): the border column alone in super-tile column 8, NS = 9."""
    shape = (512, 260, 5, "contiguous")
    c, ref = cases.prior_case(*shape), cases.prior_reference(*shape)
    chk = Checks(f"block-step forms, prior sweep k={shape[0]}")
    got = {}
    with _native.Device(0) as own:
        for form, values in FORMS.items():
            with options(own, values):
                got[form] = prior_sweep(own, c)
            check_prior(chk, form, got[form], ref, c, f"k={shape[0]} {form}")
    for a, b in SAME_LAUNCHES:
        chk.that(all(np.array_equal(x, y) for x, y in zip(got[a], got[b])), f"{a} and {b} differ: not the same launches")
    chk.finish()


# ---- 3. sweep against run where their forms differ --------------------------------------------------------------------
def test_single_solve_agrees_with_run_where_the_sweep_is_unfused_and_the_run_fused(dev):
    """k = 510, one column: the sweep's arena has NS = 8 as the run's (k + 1 = 511), so add the case's two columns to reach
    NS = 9 - the sweep's block steps are the three-kernel ones, the run's the fused ones - and compare column 0."""
    k, R = 510, 3
    c = cases.jeffreys_solve_case(k, R, "contiguous")
    shift = c["shift"][:, 1:2, :]
    rhs = np.random.default_rng(953000 + k).normal(size=(W, R, k))
    b = dev.batch("jeffreys", k, c["N"], c["n_r"], GAMMA, W, 0, _native.FLAG_NO_CENTER)
    try:
        b.upload(c["panel"], **c["upload"])
        x, status = b.solve_sweep_tiled(shift=shift, rhs=rhs, default_rhs=False)
        x1, status1 = b.solve_sweep_tiled(shift=shift, rhs=rhs[:, :1], default_rhs=False)
        b.set_rhs(rhs[:, 0, :]).set_shift(shift[:, 0, :])
        wts, wstatus, _ = b.run().download(want_aux=False)
    finally:
        b.close()
    chk = Checks(f"sweep vs run k={k}")
    chk.that(x.shape == (W, 1, R, k) and x1.shape == (W, 1, 1, k), f"shapes {x.shape}, {x1.shape}")
    chk.that((wstatus == _native.STATUS_OK).all() and (status[:, 0] == wstatus).all() and (status1[:, 0] == wstatus).all(),
             f"statuses {status.tolist()}, {status1.tolist()}, run {wstatus.tolist()}")
    chk.solution("NS 9 sweep vs run", x[:, 0, 0, :], wts, "column 0 of 3", tol=RUN_TOL)
    chk.solution("NS 8 sweep vs run", x1[:, 0, 0, :], wts, "single column", tol=RUN_TOL)
    chk.finish()


def test_prior_sweep_agrees_with_run_at_config_4(dev):
    """k = 1000, N = 500, 22 intraday days: slot 1 carries the batch's own prior; the run centres S0 by a row of the window,
    the sweep's C pass by the raw moments of 1715 rows."""
    c = dict(cases.prior_case(1000, 500, 22, "contiguous"))
    c["n0"], c["w0"] = c["n0"].copy(), c["w0"].copy()
    c["n0"][:, 1], c["w0"][:, 1, :] = c["upload"]["n0"], c["upload"]["w0"]
    b = dev.batch("conjugate", c["k"], c["N"], c["n_r"], GAMMA, W, c["m"], _native.FLAG_NO_SHARED_GRAM)
    try:
        b.upload(c["panel"], **c["upload"])
        ref, rstat, raux = b.run().download()
        wts, status, aux = b.prior_sweep_tiled(c["n0"], c["w0"])
    finally:
        b.close()
    chk = Checks("prior sweep vs run k=1000")
    chk.that((rstat == 0).all() and (status == 0).all(), f"statuses {status.tolist()}, run {rstat.tolist()}")
    chk.solution("weights", wts[:, 1], ref, "slot 1 vs run")
    chk.aux("aux", aux[:, 1, :6], raux[:, :6], "slot 1 vs run")
    chk.finish()


# ---- 4. automatic sub-ranges -------------------------------------------------------------------------------------------
def test_prior_sweep_cuts_sub_ranges_by_itself(dev):
    """k = 1023: 16 windows' C and T fill 256 MiB, so W = 18 runs as 16 + 2 with no option set."""
    k, N, Wn, Pn = 1023, 1100, 18, 2
    fit = SWEEP_WORKSPACE_BYTES // (2 * k * k * 8)
    assert fit == 16 and Wn > fit, f"{fit} windows per sub-range: W = {Wn} no longer reaches a second one"
    inp, n0, w0 = cases.prior_inputs(k, N, 1, Wn, Pn, 954000 + k)
    n0[:, 1], w0[:, 1, :] = inp["n0"], inp["w0"]
    up = dict(start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, Wn, inp["m"], _native.FLAG_NO_SHARED_GRAM)
    try:
        b.upload(inp["panel"], **up)
        run_w, run_s, run_a = b.run().download()
        auto = b.prior_sweep_tiled(n0, w0)
        with options(dev, {"sweep_chunk_windows": 5}, reset=0):
            forced = b.prior_sweep_tiled(n0, w0)
    finally:
        b.close()
    chk = Checks(f"automatic sub-ranges, prior sweep k={k} W={Wn}")
    chk.that((run_s == 0).all() and (auto[1] == 0).all(), f"statuses {auto[1].tolist()}, run {run_s.tolist()}")
    chk.solution("vs run", auto[0][:, 1], run_w, "slot 1 of every window vs run")
    chk.aux("vs run, aux", auto[2][:, 1, :6], run_a[:, :6], "slot 1 of every window vs run")
    c = dict(k=k, N=N, panel=inp["panel"], okw=dict(up, n_r=inp["n_r"], m=inp["m"]), n0=n0, w0=w0)
    for w in (0, fit - 1, fit, Wn - 1):
        wts, aux, _, _ = cases.prior_window_reference(c, w)
        chk.solution("vs oracle", auto[0][w], wts, f"window {w}")
        chk.aux("vs oracle, aux", auto[2][w, :, :6], aux, f"window {w}")
    chk.that(all(np.array_equal(a, f) for a, f in zip(auto, forced)), "automatic sub-ranges and sweep_chunk_windows = 5 differ")
    chk.finish()


def test_solve_sweep_cuts_sub_ranges_by_itself(dev):
    """k = 1023: 32 kept matrices fill 256 MiB, so W = 34 runs as 32 + 2 with no option set."""
    k, Wn = 1023, 34
    N = 2 * k + 24
    fit = SWEEP_WORKSPACE_BYTES // (k * k * 8)
    assert fit == 32 and Wn > fit, f"{fit} windows per sub-range: W = {Wn} no longer reaches a second one"
    inp = synthetic.make_kernel_inputs(k, N, Wn, seed=955000 + k)
    rng = np.random.default_rng(955000 + k)
    shift = cases.make_shift(rng, Wn, 2)[:, 1:, :]
    rhs = rng.normal(size=(Wn, 1, k))
    b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, Wn, 0, _native.FLAG_NO_CENTER)
    try:
        b.upload(inp["panel"], start=inp["start"])
        auto = b.solve_sweep_tiled(shift=shift, rhs=rhs, default_rhs=False)
        with options(dev, {"sweep_chunk_windows": 5}, reset=0):
            forced = b.solve_sweep_tiled(shift=shift, rhs=rhs, default_rhs=False)
        b.set_rhs(rhs[:, 0, :]).set_shift(shift[:, 0, :])
        run_w, run_s, _ = b.run().download(want_aux=False)
    finally:
        b.close()
    chk = Checks(f"automatic sub-ranges, solve sweep k={k} W={Wn}")
    chk.that(auto[0].shape == (Wn, 1, 1, k), f"shape {auto[0].shape}")
    chk.that((run_s == 0).all() and (auto[1] == 0).all(), f"statuses {auto[1].tolist()}, run {run_s.tolist()}")
    chk.solution("vs run", auto[0][:, 0, 0, :], run_w, "every window vs run", tol=RUN_TOL)
    for w in (0, fit - 1, fit, Wn - 1):
        X = inp["panel"][inp["start"][w]:inp["start"][w] + inp["n_r"]]
        ref, _ = cases.shifted_solves(oracle.canonical_statistics_T(X), shift[w], rhs[w].T, False)
        chk.solution("vs oracle", auto[0][w], ref, f"window {w}")
    chk.that(all(np.array_equal(a, f) for a, f in zip(auto, forced)), "automatic sub-ranges and sweep_chunk_windows = 5 differ")
    chk.finish()


# ---- 5. statuses at depth ----------------------------------------------------------------------------------------------
def plain_row_idx(c):
    return (c["upload"]["start"][:, None] + np.arange(c["n_r"])[None, :]).astype(np.int32)


def test_nan_row_flags_every_prior_of_its_window_only_at_9_block_rows(dev):
    """the statuses are the tiled run's."""
    shape = (575, 300, 5, "contiguous")
    c, ref = cases.prior_case(*shape), cases.prior_reference(*shape)
    row_idx = plain_row_idx(c)
    row_idx[1, 7] = c["panel"].shape[0]                    # window 1 alone reads the extra row
    up = dict(c["upload"], row_idx=row_idx)
    del up["start"]
    b = dev.batch("conjugate", c["k"], c["N"], c["n_r"], GAMMA, W, c["m"])
    try:
        b.upload(np.concatenate([c["panel"], np.full((1, c["k"]), np.nan)], axis=0), **up)
        _, rstat, _ = b.run().download()
        wts, status, aux = b.prior_sweep_tiled(c["n0"], c["w0"])
    finally:
        b.close()
    chk = Checks("NaN row, prior sweep k=575")
    chk.that((status[1] != _native.STATUS_OK).all() and (status[1] == rstat[1]).all(), f"status {status.tolist()}, run {rstat.tolist()}")
    chk.that((status[0] == _native.STATUS_OK).all(), f"status {status.tolist()}")
    chk.solution("the other window", wts[0], ref["weights"][0], "window 0")
    chk.aux("the other window, aux", aux[0, :, :6], ref["aux"][0], "window 0")
    chk.finish()


def test_nan_row_flags_every_shift_of_its_window_only_at_9_block_rows(dev):
    """a NaN in the window's rows makes its first pivot a NaN, which is "not > 0": TP_STATUS_NOT_PD."""
    k, R = 575, 16
    c, ref = cases.jeffreys_solve_case(k, R, "contiguous"), cases.jeffreys_solve_reference(k, R, "contiguous", True)
    row_idx = plain_row_idx(c)
    row_idx[1, 7] = c["panel"].shape[0]
    bad = dict(c, panel=np.concatenate([c["panel"], np.full((1, k), np.nan)], axis=0), upload=dict(row_idx=row_idx))
    x, status, _ = jeffreys_sweep(dev, bad, True)
    chk = Checks("NaN row, solve sweep k=575")
    chk.that((status[1] == _native.STATUS_NOT_PD).all() and (status[0] == _native.STATUS_OK).all(), f"status {status.tolist()}")
    chk.solution("the other window", x[0], ref["x"][0], "window 0")
    chk.finish()


def test_duplicate_column_in_the_last_pivot_block_is_not_pd_unshifted_and_solved_when_shifted(dev):
    """Column 560 of window 1 repeats column 4: block row 8 of 9 (63 pivots) meets a pivot that is zero in exact arithmetic and
    rounding noise in floating point.  Under "a pivot that is not > 0" alone the noise here was positive and the unshifted
    entry came back with status OK (the shifted ones were right all along); the solve sweep now also flags
    d_i <= k 2^-52 M_ii."""
    k, R = 575, 16
    c = cases.jeffreys_solve_case(k, R, "contiguous")
    col_idx = np.tile(np.arange(k, dtype=np.int32), (W, 1))
    col_idx[1, 560] = col_idx[1, 4]
    row_idx = plain_row_idx(c)
    shift = np.tile(np.array([[0.0, 0.0], [0.5, 0.0], [2.0, 3.0]]), (W, 1, 1))
    x, status, t = jeffreys_sweep(dev, dict(c, shift=shift, upload=dict(row_idx=row_idx, col_idx=col_idx)), True)
    chk = Checks("duplicate column, solve sweep k=575")
    chk.that(status[1, 0] == _native.STATUS_NOT_PD, f"status {status.tolist()}")
    chk.that((np.delete(status.reshape(-1), cases.S) == _native.STATUS_OK).all(), f"status {status.tolist()}")
    X = c["panel"][np.ix_(row_idx[1], col_idx[1])]
    tt = oracle.canonical_statistics_t(X)
    B = np.column_stack([tt] + [c["rhs"][1, j] for j in range(R - 1)])
    ref, _ = cases.shifted_solves(oracle.canonical_statistics_T(X), shift[1, 1:], B, False)
    chk.solution("shifted", x[1, 1:], ref, "window 1, shifts 1 and 2")
    chk.kept_rhs("kept rhs", t[1], tt, "window 1 kept t")
    chk.finish()
