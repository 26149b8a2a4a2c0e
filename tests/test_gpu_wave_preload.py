"""The preloaded form of the one-wave kernel (csrc/posterior_wave_impl.h, PRE): plain conjugate batches on the contiguous
layout with shared tables start a window's accumulators from its table slot, accumulate the intraday rows already scaled,
take the centring's rank-one term as one more k-step and touch only the border tile column between the row loops.  -m gpu.

* sizes at both ends of the eligible range (kc = k mod 16 <= 13; kc = 14 keeps the present form), a border tile column
  without an asset, and eight tiles per side (tiles beyond the first 32 live in VGPRs) - against the oracle, the present
  form (option wave_preload = 0) and the batch without tables;
* windows with no whole block of their own beside ordinary ones (the tables' all-zero slot);
* a constant intraday column; a NaN daily row flags exactly the windows that contain it."""
import numpy as np
import pytest

from oracle import oracle
from incorporating_different_sources_amd import synthetic

pytestmark = pytest.mark.gpu

SHAPES = [13, 14, 29, 30, 96, 97, 100, 109, 110, 125]
GAMMA = 5.0


@pytest.fixture(scope="module")
def native():
    from incorporating_different_sources_amd import _native
    return _native


@pytest.fixture()
def preload(native):
    dev = native.default_device()
    yield lambda v: dev.set_option("wave_preload", int(v))
    dev.set_option("wave_preload", -1)


def _windows(k):
    """48 windows cover every start mod 16 three times; below k = 32 the plan shares from 256 windows on."""
    return 272 if k <= 31 else 48


def _kw(inp, **over):
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"],
              m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    kw.update(over)
    return kw


def _run_shared(native, k, N, W, kw):
    """One run of a batch that must have qualified for the shared tables."""
    dev = native.default_device()
    b = native.Batch(dev, "conjugate", k, N, kw["n_r"], GAMMA, W, kw["m"])
    try:
        b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
        assert b.shared_gram_blocks() > 0
        b.run()
        return b.download()
    finally:
        b.close()


def _three_forms(native, preload, k, N, W, kw):
    preload(1)
    pre = _run_shared(native, k, N, W, kw)
    preload(0)
    old = _run_shared(native, k, N, W, kw)
    preload(-1)
    plain = native.posterior_batch("conjugate", k, N, GAMMA, flags=native.FLAG_NO_SHARED_GRAM, **kw)
    return pre, old, plain


def test_the_automatic_choice_takes_the_preloaded_form_at_the_flagship_size(native, preload):
    """wave_preload = -1 picks per tile count (wave_preload_pays): at seven tiles per side it is the preloaded form, bit
    for bit what wave_preload = 1 gives, and not what wave_preload = 0 gives."""
    k, N, W = 100, 130, 48
    kw = _kw(synthetic.make_kernel_inputs(k, N, W, seed=19100))
    preload(1)
    w_on, _, _ = _run_shared(native, k, N, W, kw)
    preload(0)
    w_off, _, _ = _run_shared(native, k, N, W, kw)
    preload(-1)
    w_auto, _, _ = _run_shared(native, k, N, W, kw)
    assert np.array_equal(w_auto, w_on) and not np.array_equal(w_auto, w_off)


@pytest.mark.parametrize("k", [45, 61, 77, 93, 141])
def test_the_tile_counts_between(native, preload, k):
    """3, 4, 5, 6 and 9 tiles per side at kc = 13 (test_shapes has 1, 2, 7 and 8): same assertions."""
    test_shapes(native, preload, k)


@pytest.mark.parametrize("k", SHAPES)
def test_shapes(native, preload, k):
    """The oracle at the project's flat 1e-10, the present form and the batch without tables at 1e-12 (the scale goes into
    the rows as its square root, so the last bits of S0 differ), the oracle's statuses, aux at the parity tests' bound."""
    N, W = k + 30, _windows(k)
    inp = synthetic.make_kernel_inputs(k, N, W, seed=19000 + k)
    kw = _kw(inp)
    ref, rstat, raux = oracle.posterior_batch_c("conjugate", k, N, GAMMA, **kw)
    (w_pre, s_pre, a_pre), (w_old, s_old, _), (w_plain, s_plain, _) = _three_forms(native, preload, k, N, W, kw)
    print(f"k={k}: |pre - oracle| = {np.abs(w_pre - ref).max():.3e}, |pre - old| = {np.abs(w_pre - w_old).max():.3e}, "
          f"|pre - no tables| = {np.abs(w_pre - w_plain).max():.3e}, bad statuses {int((s_pre != 0).sum())}")
    assert (s_pre == rstat).all(), (s_pre, rstat)
    np.testing.assert_allclose(w_pre, ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(w_pre, w_old, rtol=0, atol=1e-12)
    np.testing.assert_allclose(w_pre, w_plain, rtol=0, atol=1e-12)
    np.testing.assert_allclose(a_pre[:, :6], raux[:, :6], rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("k", [29, 61])
def test_windows_without_a_whole_block_start_from_the_zero_slot(native, preload, k):
    """Every third window has 10 rows (never a whole aligned 16-row block), every third 20 (none or one), the rest all
    of them: the short ones read the all-zero slot and push every row through the MFMAs."""
    N, W = k + 30, 272
    inp = synthetic.make_kernel_inputs(k, N, W, seed=19500 + k)
    n_rows = np.full(W, inp["n_r"], dtype=np.int32)
    n_rows[1::3] = 10
    n_rows[2::3] = 20
    kw = _kw(inp, n_rows=n_rows)
    ref, rstat, raux = oracle.posterior_batch_c("conjugate", k, N, GAMMA, **kw)
    (w_pre, s_pre, a_pre), (w_old, s_old, _), (w_plain, s_plain, _) = _three_forms(native, preload, k, N, W, kw)
    print(f"k={k}: |pre - oracle| = {np.abs(w_pre - ref).max():.3e}, |pre - old| = {np.abs(w_pre - w_old).max():.3e}, "
          f"statuses {np.unique(s_pre).tolist()}")
    assert (s_pre == rstat).all(), (s_pre, rstat)
    np.testing.assert_allclose(w_pre, ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(w_pre, w_old, rtol=0, atol=1e-12)
    np.testing.assert_allclose(w_pre, w_plain, rtol=0, atol=1e-12)
    np.testing.assert_allclose(a_pre[:, :6], raux[:, :6], rtol=1e-11, atol=1e-14)


def test_a_constant_intraday_column_stays_exactly_zero(native, preload):
    """Column 7 of the intraday panel is one value throughout: shifted by the window's first row it is exactly zero, and
    scaled it still is - row and column 7 of S0 vanish as on the present path."""
    k, N, W = 100, 130, 48
    inp = synthetic.make_kernel_inputs(k, N, W, seed=19700)
    hf = inp["hf_panel"].copy()
    hf[:, 7] = 1.25e-3
    kw = _kw(inp, hf_panel=hf)
    ref, rstat, _ = oracle.posterior_batch_c("conjugate", k, N, GAMMA, **kw)
    (w_pre, s_pre, _), (w_old, s_old, _), _ = _three_forms(native, preload, k, N, W, kw)
    print(f"|pre - oracle| = {np.abs(w_pre - ref).max():.3e}, |pre - old| = {np.abs(w_pre - w_old).max():.3e}")
    assert (s_pre == rstat).all() and (s_old == rstat).all(), (s_pre, s_old, rstat)
    np.testing.assert_allclose(w_pre, w_old, rtol=0, atol=1e-12)
    np.testing.assert_allclose(w_pre, ref, rtol=0, atol=1e-10)


def test_a_nan_daily_row_flags_exactly_the_windows_that_contain_it(native, preload):
    """test_a_non_finite_row_poisons_only_the_windows_that_contain_it on the preloaded form: the NaN reaches a window
    through its slot or through its edge rows, and nobody else."""
    k, N, W = 100, 130, 48
    inp = synthetic.make_kernel_inputs(k, N, W, seed=19800)
    n_r = inp["n_r"]
    panel = inp["panel"].copy()
    r_bad = 20
    panel[r_bad, :] = np.nan
    kw = _kw(inp, panel=panel)
    (w_pre, s_pre, _), (w_old, s_old, _), (w_plain, s_plain, _) = _three_forms(native, preload, k, N, W, kw)
    contains = (inp["start"] <= r_bad) & (r_bad < inp["start"] + n_r)
    assert 0 < contains.sum() < W
    assert (s_pre[contains] != 0).all()
    assert (s_pre[~contains] == 0).all(), np.flatnonzero((s_pre != 0) & ~contains)[:10]
    assert np.array_equal(s_pre != 0, s_plain != 0) and np.array_equal(s_pre != 0, s_old != 0)
    np.testing.assert_allclose(w_pre[~contains], w_plain[~contains], rtol=0, atol=1e-12)
    clean, s_clean, _ = native.posterior_batch("conjugate", k, N, GAMMA, **_kw(inp))
    np.testing.assert_allclose(w_pre[~contains], clean[~contains], rtol=0, atol=1e-12)
