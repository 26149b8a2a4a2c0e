"""Batches that run "with options" - a caller's or a kept right-hand side, a shift, TP_FLAG_CENTER_BY_ROWS / TP_FLAG_NO_CENTER,
a matrix read-back - against the fp64 oracle, at every size of the multi-wave register-tile kernel they are sent to (k <= 239,
one instantiation per tile count), on both Gram forms and both update forms of the tiled path above it, in the contiguous and
in the index layout (row_idx / ragged n_rows / col_idx / rf_adj: what every backtest uploads), and through the Jorion and
Greyserman portfolios above the solve sweep's largest universe.  Cases, references and bounds: tests/_run_option_cases.py;
tests/test_host_run_option_cases.py shows on the CPU that every reference here is good to a tenth of its bound.  -m gpu.

Every test goes through all its checks, prints the worst |got - ref| per group next to its bound, and fails at the end if any
check missed."""
import numpy as np
import pytest

from incorporating_different_sources_amd import _native
from incorporating_different_sources_amd import portfolio_calculations as pc

import _run_option_cases as cases

pytestmark = pytest.mark.gpu

GAMMA = cases.GAMMA
# (tiled_wave, tiled_fuse): one-wave / four-wave Gram and diagonal-block kernels x fused / three-kernel update
TILED_FORMS = ((1, 1), (1, 0), (0, 1), (0, 0))
FORM_TOL = 1e-12      # the two Gram forms against each other: FORM_TOL max(1, |w|.max())


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


@pytest.fixture(autouse=True)
def one_blas_thread():
    with cases.small_matrix_blas():
        yield


def test_flag_values_of_the_helper_are_the_librarys():
    assert (cases.FLAG_CENTER_BY_ROWS, cases.FLAG_NO_CENTER) == (_native.FLAG_CENTER_BY_ROWS, _native.FLAG_NO_CENTER)


class Checks:
    """Collects every comparison of one test: the worst error-to-bound ratio per group for the printout, the misses for
    the assertion at the end."""

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

    def solution(self, group, got, ref, what):
        self.close(group, got, ref, cases.sol_bound(ref), what)

    def kept_rhs(self, group, got, ref, what):
        self.close(group, got, ref, cases.RHS_TOL * max(1.0, float(np.abs(ref).max())), what)

    def elementwise(self, group, got, ref, tol, what):
        """numpy.testing.assert_allclose(got, ref, **tol), reported as the worst ratio of |got - ref| to atol + rtol |ref|."""
        ratio = np.abs(got - ref) / (tol["atol"] + tol["rtol"] * np.abs(ref))
        worst = float(ratio.max()) if np.isfinite(got).all() else np.inf
        if group not in self.worst or worst > self.worst[group][0] / self.worst[group][1]:
            self.worst[group] = (worst, 1.0, what + " (in units of atol + rtol |ref|)")
        self.that(worst <= 1.0, f"{what}: {worst:.3e} x (atol + rtol |ref|), rtol = {tol['rtol']}, atol = {tol['atol']}")

    def finish(self):
        for group, (err, bound, what) in self.worst.items():
            print(f"{self.title} [{group}]: worst |got - ref| = {err:.3e} (bound {bound:.3e}) at {what}")
        assert not self.missed, f"{len(self.missed)} checks missed:\n" + "\n".join(self.missed[:40])


def run(b):
    return b.run().download()


def jeffreys_references(case):
    """({flag: {run: weights}}, t): computed once per case, shared by the kernel forms that run it."""
    return ({flag: {name: cases.jeffreys_reference(case, flag, shifted, with_rhs)
                    for name, shifted, with_rhs in cases.JEFFREYS_RUNS} for flag in cases.FLAGS}, cases.jeffreys_t(case))


def jeffreys_sequence(dev, case, references, chk, group, what):
    """For each flag value one Batch, one upload and four runs: kept right-hand side; shift; shift and caller's right-hand
    side; both taken back.  Returns {(flag, run): weights} for comparisons between kernel forms."""
    k, W = case["k"], case["W"]
    refs, t_ref = references
    out = {}
    for flag in cases.FLAGS:
        tag = f"{what} flag={flag}"
        ref = refs[flag]
        b = dev.batch("jeffreys", k, case["N"], case["n_r"], GAMMA, W, 0, flag)
        try:
            b.upload(case["panel"], **case["upload"])
            b.keep_rhs()
            w1, s1, _ = run(b)                                              # 1. kept right-hand side
            t1 = b.download_rhs()
            chk.that((s1 == 0).all(), f"{tag} plain: status {s1}")
            chk.solution(group, w1, ref["plain"], f"{tag} plain")
            chk.kept_rhs(group + " kept rhs", t1, t_ref, f"{tag} kept t")
            b.set_shift(case["shift"])                                      # 2. shift (window 0 unshifted)
            w2, s2, _ = run(b)
            chk.that((s2 == 0).all(), f"{tag} shift: status {s2}")
            chk.solution(group, w2, ref["shift"], f"{tag} shift")
            b.set_rhs(case["rhs"])                                          # 3. caller's right-hand side, shift still set
            w3, s3, _ = run(b)
            chk.that((s3 == 0).all(), f"{tag} shift+rhs: status {s3}")
            chk.solution(group, w3, ref["shift+rhs"], f"{tag} shift+rhs")
            chk.that(np.array_equal(b.download_rhs(), case["rhs"]), f"{tag}: download_rhs is not the caller's rows")
            b.set_shift(None).set_rhs(None)                                 # 4. both taken back: run 1 again, bit for bit
            w4, s4, _ = run(b)
            chk.that(np.array_equal(w4, w1) and np.array_equal(s4, s1), f"{tag}: options taken back, weights differ from run 1")
            chk.that(np.array_equal(b.download_rhs(), t1), f"{tag}: options taken back, kept t differs from run 1")
        finally:
            b.close()
        out.update({(flag, "plain"): w1, (flag, "shift"): w2, (flag, "shift+rhs"): w3})
    if case["layout"] == "index":
        # the cases discriminate: with fewer rows than N the two centrings are far apart, an ignored flag cannot pass
        apart = float(np.abs(refs[0]["plain"] - refs[cases.FLAG_CENTER_BY_ROWS]["plain"]).max())
        chk.that(apart > cases.DISCRIMINATE * max(1.0, float(np.abs(refs[0]["plain"]).max())),
                 f"{what}: default and row-count centring only {apart:.3e} apart")
    return out


def conjugate_sequence(dev, case, ref, chk, group, what):
    """Kept right-hand side; caller's right-hand side (the nu rescale of ref:572-575 still applies); taken back.  Returns
    {run: weights}."""
    k, W = case["k"], case["W"]
    b = dev.batch("conjugate", k, case["N"], case["n_r"], GAMMA, W, case["m"])
    try:
        b.upload(case["panel"], **case["upload"])
        b.keep_rhs()
        w1, s1, a1 = run(b)
        b0 = b.download_rhs()
        chk.that((s1 == 0).all(), f"{what}: status {s1}")
        chk.solution(group, w1, ref["weights"], f"{what} weights")
        chk.elementwise(group + " aux", a1[:, :6], ref["aux"], cases.AUX_TOL, f"{what} aux")
        chk.kept_rhs(group + " kept rhs", b0, ref["b0"], f"{what} kept c S0 w0 + t")
        b.set_rhs(case["rhs"])
        w2, s2, a2 = run(b)
        chk.that((s2 == 0).all(), f"{what} rhs: status {s2}")
        chk.solution(group, w2, ref["weights_rhs"], f"{what} rhs weights")
        chk.elementwise(group + " aux", a2[:, :6], ref["aux_rhs"], cases.AUX_TOL, f"{what} rhs aux")
        chk.that(np.array_equal(b.download_rhs(), case["rhs"]), f"{what}: download_rhs is not the caller's rows")
        b.set_rhs(None)
        w3, s3, a3 = run(b)
        chk.that(np.array_equal(w3, w1) and np.array_equal(s3, s1) and np.array_equal(a3, a1),
                 f"{what}: right-hand side taken back, results differ from the first run")
        chk.that(np.array_equal(b.download_rhs(), b0), f"{what}: right-hand side taken back, kept one differs from the first run")
    finally:
        b.close()
    return {"default": w1, "rhs": w2}


def conjugate_matrices(dev, case, ref, chk, group, what):
    """tp_batch_download_matrix of the last window: S0 and c S0 w0, T and t, S1 and c S0 w0 + t."""
    k, W = case["k"], case["W"]
    w = W - 1
    a = ref["windows"][w]
    prior_rhs = a["c"] * (a["S0"] @ case["w0"][w])
    with dev.batch("conjugate", k, case["N"], case["n_r"], GAMMA, W, case["m"]) as b:
        b.upload(case["panel"], **case["upload"])
        b.run()
        for name, M_ref, v_ref in (("prior", a["S0"], prior_rhs), ("gram", a["T"], a["t"]), ("posterior", a["S1"], ref["b0"][w])):
            M, v = b.download_matrix(w, name)
            chk.elementwise(f"{group} {name} matrix", M, M_ref, cases.MATRIX_TOL, f"{what} {name} matrix")
            chk.kept_rhs(f"{group} {name} vector", v, v_ref, f"{what} {name} vector")


# ---- (a) Jeffreys, register-tile path, every size -----------------------------------------------------------------------
@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("nt", cases.TILE_COUNTS)
def test_jeffreys_options_at_every_size_of_the_register_tile_kernel(dev, nt, layout):
    chk = Checks(f"(a) jeffreys NT={nt} {layout}")
    for k in cases.sizes_of_tile_count(nt):
        case = cases.make_case("jeffreys", k, layout, 4)
        jeffreys_sequence(dev, case, jeffreys_references(case), chk, "solutions", f"k={k} {layout}")
    chk.finish()


# ---- (b) conjugate, register-tile path, the three positions of the border column ------------------------------------
@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("nt", cases.TILE_COUNTS)
def test_conjugate_options_at_the_border_sizes_of_the_register_tile_kernel(dev, nt, layout):
    chk = Checks(f"(b) conjugate NT={nt} {layout}")
    for k in cases.border_sizes_of_tile_count(nt):
        case = cases.make_case("conjugate", k, layout, 3)
        conjugate_sequence(dev, case, cases.conjugate_reference(case), chk, "weights", f"k={k} {layout}")
    chk.finish()


@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("nt", cases.TILE_COUNTS)
def test_conjugate_matrix_read_back_at_the_border_sizes_of_the_register_tile_kernel(dev, nt, layout):
    """S0, T, S1 element-wise at rtol = 1e-11.  The read-back of S0 centres the intraday rows first (two passes): the one-pass
    shifted scatter a run uses has an absolute error, ~1e-16 of the terms summed, and missed this bound by factors 1.05 .. 3.5
    at k = 129, 145, 176, 177, 192, 193, 208, 209 on off-diagonal entries that cancel to 1e-6 of the typical one."""
    chk = Checks(f"(b) conjugate matrices NT={nt} {layout}")
    for k in cases.border_sizes_of_tile_count(nt):
        case = cases.make_case("conjugate", k, layout, 3)
        conjugate_matrices(dev, case, cases.conjugate_reference(case), chk, "read-back", f"k={k} {layout}")
    chk.finish()


# ---- (c) the tiled path, every kernel form ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("k", cases.TILED_SIZES)
def test_options_on_every_form_of_the_tiled_path(k, layout):
    chk = Checks(f"(c) tiled k={k} {layout}")
    jcase, ccase = cases.make_case("jeffreys", k, layout, 3), cases.make_case("conjugate", k, layout, 3)
    jrefs, cref = jeffreys_references(jcase), cases.conjugate_reference(ccase)
    got = {}
    with _native.Device(0) as own:                       # the forms are options of the handle: a handle of the test's own
        for wave, fuse in TILED_FORMS:
            own.set_option("tiled_wave", wave).set_option("tiled_fuse", fuse)
            form = f"wave={wave} fuse={fuse}"
            got[wave, fuse] = dict(jeffreys_sequence(own, jcase, jrefs, chk, f"{form} jeffreys", f"k={k} {layout} {form}"))
            got[wave, fuse].update(conjugate_sequence(own, ccase, cref, chk, f"{form} conjugate", f"k={k} {layout} {form}"))
        # tp_batch_download_matrix stops at the register-tile path: refused here, not answered with something else
        with own.batch("conjugate", k, ccase["N"], ccase["n_r"], GAMMA, 3, ccase["m"]) as b:
            b.upload(ccase["panel"], **ccase["upload"])
            with pytest.raises(_native.TangencyError) as refused:
                b.download_matrix(2, "prior")
            chk.that(refused.value.code == _native.TP_ERR_UNSUPPORTED, f"k={k}: download_matrix failed with {refused.value}")
    for fuse in (0, 1):                                  # the two Gram forms against each other
        for key, w_wave in got[1, fuse].items():
            w_four = got[0, fuse][key]
            chk.close("one-wave vs four-wave Gram", w_wave, w_four, FORM_TOL * max(1.0, float(np.abs(w_four).max())),
                      f"k={k} {layout} fuse={fuse} {key}")
    chk.finish()


# ---- (d) portfolios above 143 assets ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", cases.PORTFOLIO_SIZES)
def test_jorion_above_the_solve_sweeps_largest_universe(k):
    case, kw, _ = cases.portfolio_case(k)
    assert k > _native.sweep_max_assets()
    chk = Checks(f"(d) jorion k={k}")
    chk.solution("weights", pc._jorion_batch(kw, GAMMA, k, case["N"]), cases.jorion_reference(case), f"k={k}")
    chk.finish()


@pytest.mark.parametrize("k,tiled_sweep", [(150, False), (150, True), (239, False), (256, False), (256, True)])
def test_greyserman_above_the_solve_sweeps_largest_universe(monkeypatch, k, tiled_sweep):
    case, kw, draws = cases.portfolio_case(k)
    assert k > _native.sweep_max_assets()
    monkeypatch.setattr(pc, "GREYSERMAN_TILED_SWEEP", tiled_sweep)
    chk = Checks(f"(d) greyserman k={k} {'tiled sweep' if tiled_sweep else 'replicated batch'}")
    chk.solution("weights", pc._greyserman_batch(kw, GAMMA, k, case["N"], draws=draws), cases.greyserman_from(case, draws),
                 f"k={k}")
    chk.finish()
