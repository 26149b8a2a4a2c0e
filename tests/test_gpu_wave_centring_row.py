"""The centring row of the one-wave kernel's preloaded form (csrc/posterior_wave_impl.h, wave_gram TROW): the rank-one term
of the centring is one row behind a window's last daily edge row, in the last k-step of that pass, and the border pass
follows the edge rows.  What decides where the row lands is the LENGTH of the edge-row sequence, which
test_gpu_wave_preload.py cannot vary (N = k + 30: 1 or 17 edge rows).  -m gpu.

* every residue of the edge-row count mod 4, no edge row at all, and exactly 12 and 24 of them (whole triples of k-steps
  from the main loop, the centring row alone behind it), at every start mod 16 - per-window n_rows over two whole-block
  counts; the edge counts are computed here the way the kernel computes them and their coverage is asserted;
* windows without a slot: every row goes through that pass and the centring row follows row n_rows - 1;
* keep_posterior (mode 3): bit-equal results, symmetric matrices, the oracle's S1.

Bounds: the project's own (test_gpu_wave_preload.py, test_gpu_posterior_matrices.py)."""
import numpy as np
import pytest

from oracle import oracle
from incorporating_different_sources_amd import synthetic

from test_gpu_posterior_matrices import oracle_mats

pytestmark = pytest.mark.gpu

GAMMA = 5.0
BLK = 16
# edge-row counts asked for, in the order a window tries them: 0, 12, 24 and every residue mod 4 on both sides of a k-step
TARGETS = [0, 12, 24, 1, 2, 3, 13, 14, 15, 9, 25, 30, 4, 7, 22, 17]


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
    """As test_gpu_wave_preload.py: every start mod 16 three times; below k = 32 the plan shares from 256 windows on."""
    return 272 if k <= 31 else 48


def _kw(inp, **over):
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"],
              m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    kw.update(over)
    return kw


def edge_rows(start, n_rows):
    """Per window: (rows that go through the MFMAs, has a slot) - the kernel's own arithmetic.  A window has a slot when it
    holds a whole aligned block; the batches here have at most four distinct block counts, so every such window shares."""
    first = np.asarray(start, dtype=np.int64)
    count = np.asarray(n_rows, dtype=np.int64)
    b0 = (first + BLK - 1) // BLK
    b1 = (first + count) // BLK
    slot = b1 - b0 > 0
    assert len(np.unique((b1 - b0)[slot])) <= 4
    edges = (BLK * b0 - first) + (first + count - BLK * b1)
    return np.where(slot, edges, count), slot


def varied_n_rows(start, n_r):
    """n_rows per window: head rows in front of the first aligned block (given by the start), L whole blocks, L one of two
    values, and a tail chosen so that head + tail is the first reachable entry of TARGETS, tried from the window's own
    position in the list on."""
    l_hi = (n_r - 30) // BLK
    assert l_hi >= 1, n_r
    l_lo = max(l_hi - 1, 1)
    out = np.empty(len(start), dtype=np.int32)
    for w, first in enumerate(start):
        head = int(-first) % BLK
        for j in range(len(TARGETS)):
            tail = TARGETS[(w // BLK + w + j) % len(TARGETS)] - head
            if 0 <= tail < BLK:
                break
        else:
            raise AssertionError("no reachable target")
        out[w] = head + BLK * (l_hi if w % 2 else l_lo) + tail
    assert (out >= 1).all() and (out <= n_r).all()
    return out


def _run_shared(native, k, N, W, kw, keep=False):
    """One run with wave_preload as set, of a batch that must have qualified for the shared tables."""
    dev = native.default_device()
    b = native.Batch(dev, "conjugate", k, N, kw["n_r"], GAMMA, W, kw["m"])
    try:
        b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
        assert b.shared_gram_blocks() > 0
        if keep:
            b.keep_posterior(0, None)
        b.run()
        mats = b.download_posterior() if keep else None
        return b.download(), mats
    finally:
        b.close()


def _check_against_all(native, preload, k, N, W, kw):
    ref, rstat, raux = oracle.posterior_batch_c("conjugate", k, N, GAMMA, **kw)
    preload(1)
    (w_pre, s_pre, a_pre), _ = _run_shared(native, k, N, W, kw)
    preload(0)
    (w_old, s_old, _), _ = _run_shared(native, k, N, W, kw)
    preload(-1)
    w_plain, s_plain, _ = native.posterior_batch("conjugate", k, N, GAMMA, flags=native.FLAG_NO_SHARED_GRAM, **kw)
    print(f"k={k}: |pre - oracle| = {np.abs(w_pre - ref).max():.3e}, |pre - old| = {np.abs(w_pre - w_old).max():.3e}, "
          f"|pre - no tables| = {np.abs(w_pre - w_plain).max():.3e}, statuses {np.unique(s_pre).tolist()}")
    assert (s_pre == rstat).all(), (s_pre, rstat)
    np.testing.assert_allclose(w_pre, ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(w_pre, w_old, rtol=0, atol=1e-12)
    np.testing.assert_allclose(w_pre, w_plain, rtol=0, atol=1e-12)
    np.testing.assert_allclose(a_pre[:, :6], raux[:, :6], rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("k", [13, 29, 100, 109, 125, 141])
def test_every_length_of_the_edge_row_sequence(native, preload, k):
    """One, two, seven, eight and nine tiles per side (kc = 13 at 1, 2, 7 and 9; k = 100 the flagship; 125 and 141 keep
    tiles in VGPRs): the centring row in row slot 0, 1, 2 and 3 of its k-step, alone in a k-step of its own behind 0, 12
    and 24 edge rows, and behind one, two and three masked k-steps."""
    N, W = k + 62, _windows(k)
    inp = synthetic.make_kernel_inputs(k, N, W, seed=26000 + k)
    n_rows = varied_n_rows(inp["start"], inp["n_r"])
    edges, slot = edge_rows(inp["start"], n_rows)
    got = set(edges[slot].tolist())
    print(f"k={k}: edge-row counts {sorted(got)}")
    assert set(np.unique(edges[slot] % 4).tolist()) == {0, 1, 2, 3}
    assert 0 in got and 12 in got and 24 in got
    assert set((inp["start"][slot] % 16).tolist()) == set(range(16))
    _check_against_all(native, preload, k, N, W, _kw(inp, n_rows=n_rows))


@pytest.mark.parametrize("k", [29, 61])
def test_windows_without_a_slot_take_the_row_behind_their_last_row(native, preload, k):
    """Every third window has 10 rows (never a whole aligned block), every third 20 (none or one), the rest all of them: a
    window without a slot pushes all its rows through the edge-row pass, and the centring row is slot n_rows of it."""
    N, W = k + 30, 272
    inp = synthetic.make_kernel_inputs(k, N, W, seed=26500 + k)
    n_rows = np.full(W, inp["n_r"], dtype=np.int32)
    n_rows[1::3] = 10
    n_rows[2::3] = 20
    edges, slot = edge_rows(inp["start"], n_rows)
    assert {10, 20} <= set(edges[~slot].tolist()) and slot[0::3].all()
    _check_against_all(native, preload, k, N, W, _kw(inp, n_rows=n_rows))


def test_keep_posterior_changes_nothing_and_keeps_the_centred_matrix(native, preload):
    """Mode 3 at k = 100 over the varied edge counts: weights, statuses and aux bit-equal to the run without it, the kept
    matrices exactly symmetric and the oracle's S1 at test_gpu_posterior_matrices.py's bound."""
    k = 100
    N, W = k + 62, _windows(k)
    inp = synthetic.make_kernel_inputs(k, N, W, seed=26900)
    n_rows = varied_n_rows(inp["start"], inp["n_r"])
    kw = _kw(inp, n_rows=n_rows)
    preload(1)
    (w0_, s0_, a0_), _ = _run_shared(native, k, N, W, kw)
    (w3_, s3_, a3_), mats = _run_shared(native, k, N, W, kw, keep=True)
    assert np.array_equal(w0_, w3_) and np.array_equal(s0_, s3_) and np.array_equal(a0_, a3_, equal_nan=True)
    assert (s3_ == 0).all()
    assert np.array_equal(mats, mats.transpose(0, 2, 1))
    ref = oracle_mats("conjugate", k, N, **kw)
    scale = np.abs(ref).max()
    err = np.abs(mats - ref).max()
    print(f"max|kept - oracle| = {err:.3e}, scale {scale:.3e}")
    assert err <= 1e-11 * scale, f"max|kept - oracle| = {err:.3e} > 1e-11 x {scale:.3e}"
