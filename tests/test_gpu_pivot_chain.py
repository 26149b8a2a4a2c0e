"""The pivot chain of the one-wave kernel (csrc/posterior_wave_impl.h, phase F): the multipliers of a pivot reach the
rows below it through an LDS row (two rows, by pivot parity) instead of v_readlane pairs; the rows the next pivot waits
for keep the v_readlane form.  -m gpu.

* every shape of a chain: 1, 2 and 3 live pivots in the last tile, a full last tile, a border column alone in its tile,
  both register homes of the tiles - against the oracle and the multi-wave kernel, both strategies, both layouts;
* a zero pivot at every kind of chain position (first pivot, a row on the v_readlane path, the first row on the LDS
  path, the last pivot of a tile, the first pivot of the next tile) is flagged, and leaves nothing behind on the handle."""
import numpy as np
import pytest

from oracle import oracle
from incorporating_different_sources_amd import synthetic

pytestmark = pytest.mark.gpu

CHAIN_K = [1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 100, 143]
ZERO_PIVOTS = [(17, c) for c in (0, 1, 2, 3, 15, 16)] + [(33, c) for c in (31, 32)] + [(100, c) for c in (0, 3, 47, 96, 99)]
EXTRA_COLS = 5           # index layout: the panels carry this many columns the windows do not gather


@pytest.fixture(scope="module")
def native():
    from incorporating_different_sources_amd import _native
    return _native


@pytest.fixture()
def kernel_choice(native):
    dev = native.default_device()
    yield lambda v: dev.set_option("wave_kernel", int(v))
    dev.set_option("wave_kernel", -1)


def _rows(strat, k):
    return max(2 * k + 10, 40) if strat == "jeffreys" else max(k + 30, 40)


def _kwargs(strat, k, N, W, seed, layout):
    """Arguments of `posterior_batch` (the oracle's and the library's alike) for W windows of k assets."""
    if layout == "contiguous":
        inp = synthetic.make_kernel_inputs(k, N, W, seed=seed)
        kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
        if strat == "conjugate":
            kw.update(hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=inp["m"], w0=inp["w0"], n0=inp["n0"])
        return kw
    # index layout: explicit (shuffled) rows per window, k gathered columns of a wider panel
    rng = np.random.default_rng(seed)
    kp = k + EXTRA_COLS
    inp = synthetic.make_kernel_inputs(kp, N, W, seed=seed)
    n_r = inp["n_r"]
    col_idx = np.stack([np.sort(rng.choice(kp, k, replace=False)) for _ in range(W)]).astype(np.int32)
    row_idx = np.stack([inp["start"][w] + rng.permutation(n_r) for w in range(W)]).astype(np.int32)
    kw = dict(panel=inp["panel"], start=None, row_idx=row_idx, col_idx=col_idx, n_r=n_r)
    if strat == "conjugate":
        w0 = np.abs(rng.normal(size=(W, k)))
        w0 /= w0.sum(axis=1, keepdims=True)
        kw.update(hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=inp["m"], w0=w0, n0=inp["n0"])
    return kw


@pytest.mark.parametrize("layout", ["contiguous", "index"])
@pytest.mark.parametrize("strat", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("k", CHAIN_K)
def test_chain_shapes(native, kernel_choice, k, strat, layout):
    """Bounds as in test_every_universe_size_of_the_wave_kernel: the oracle at 1e-10, the multi-wave kernel (same
    arithmetic per element) at 1e-12 - 1e-11 where k + 1 = 0 (mod 16), DESIGN section 4 - and the oracle's status."""
    N = _rows(strat, k)
    kw = _kwargs(strat, k, N, 9, 41000 + k, layout)
    ref, rstat, _ = oracle.posterior_batch_c(strat, k, N, 5.0, **kw)
    kernel_choice("0")
    w_multi, s_multi, _ = native.posterior_batch(strat, k, N, 5.0, **kw)
    kernel_choice("1")
    w_wave, s_wave, _ = native.posterior_batch(strat, k, N, 5.0, **kw)
    print(f"k={k} {strat} {layout}: |wave - oracle| = {np.abs(w_wave - ref).max():.3e}, "
          f"|wave - multi| = {np.abs(w_wave - w_multi).max():.3e}, status {s_wave.tolist()}")
    assert (s_wave == rstat).all(), (s_wave, rstat)
    np.testing.assert_allclose(w_wave, ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(w_wave, w_multi, rtol=0, atol=1e-11 if k % 16 == 15 else 1e-12)


@pytest.mark.parametrize("strat", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("k,c", ZERO_PIVOTS)
def test_a_zero_pivot_at_every_chain_position(native, kernel_choice, k, c, strat):
    """Column c of both panels is zero, so pivot c is exactly zero: its 1/sqrt is an infinity, and the status
    accumulation (0 * rinv per pivot) must see it wherever pivot c sits in the chain.  Every window is flagged; the same
    batch shape with the untouched panels, run afterwards on the same handle, gives the oracle's weights."""
    N = _rows(strat, k)
    inp = synthetic.make_kernel_inputs(k, N, 4, seed=41000 + k)
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"])
    if strat == "conjugate":
        kw.update(hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    bad = dict(kw, panel=kw["panel"].copy())
    bad["panel"][:, c] = 0.0
    if strat == "conjugate":
        bad["hf_panel"] = kw["hf_panel"].copy()
        bad["hf_panel"][:, c] = 0.0
    _, rstat_bad, _ = oracle.posterior_batch_c(strat, k, N, 5.0, **bad)
    assert (rstat_bad == 2).all(), rstat_bad
    kernel_choice("1")
    _, s_bad, _ = native.posterior_batch(strat, k, N, 5.0, **bad)
    print(f"k={k} c={c} {strat}: status {s_bad.tolist()}")
    assert (s_bad != 0).all(), s_bad
    ref, rstat, _ = oracle.posterior_batch_c(strat, k, N, 5.0, **kw)
    w, s, _ = native.posterior_batch(strat, k, N, 5.0, **kw)
    print(f"k={k} c={c} {strat}: afterwards |wave - oracle| = {np.abs(w - ref).max():.3e}, status {s.tolist()}")
    assert (rstat == 0).all() and (s == 0).all(), (s, rstat)
    np.testing.assert_allclose(w, ref, rtol=0, atol=1e-10)
