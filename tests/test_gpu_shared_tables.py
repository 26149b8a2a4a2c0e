"""The block-window tables of the register-tile path from ONE kernel (csrc/posterior_shared_tables.hip, option
shared_tables = 1) against the pair block_gram_kernel + tp_window_sums_kernel (shared_tables = 0).  -m gpu.

The tables are the same bit for bit by construction (same MFMA operands, same k-step order, same additions in the same
order), so every window kernel computes the same thing from them: each case uploads ONE batch, runs it in both forms and
compares weights, statuses and aux byte for byte (uint64 views: NaNs compare too).  With starts 0 .. W-1 every position
of every table is read by some window, so a wrong table element changes some window's bits.  Every batch must have
qualified for the shared sums (shared_gram_blocks() > 0), and the handle must report the form that ran
(tp_get_option "last_shared_tables": tp_last_launch's signature is part of the C ABI and stays as it is).

One case per kernel family also compares form 1 with the oracle, at test_gpu_wave_preload.py's bounds.

Sensitivity (once, in a scratch build): with the one kernel's prefix run started one block late (block g + L + n - R + 1
instead of g + L + n - R) 55 of the 57 cases fail, each on its first comparison of the two forms ("weights: ... elements
differ, first at [1, 0]": every position but a group's first is wrong, e.g. 283 of 300 windows at k = 5).  The two that
pass cannot see a table: the batch with a fifth block count builds none, and the option contract compares automatic with
form 1 - the same kernel twice - and what the handle reports."""
import numpy as np
import pytest

from oracle import oracle
from incorporating_different_sources_amd import synthetic

pytestmark = pytest.mark.gpu

GAMMA = 5.0
W = 300
SEED = 7
# tile counts 1..15 and the kernel families: one wave (k <= 143), two waves (144..191), four waves and 32-row blocks (>= 192);
# 111: no spare column, 112: the border column alone in the last tile column
SHAPES = [5, 20, 40, 55, 77, 90, 100, 111, 112, 120, 140, 150, 191, 200, 239]
ORACLE_SHAPES = {100, 150, 200}          # one per family (the multi-wave kernel: test_the_multi_wave_kernel)


@pytest.fixture(scope="module")
def native():
    from incorporating_different_sources_amd import _native
    return _native


@pytest.fixture()
def dev(native):
    d = native.default_device()
    yield d
    for name in ("shared_tables", "wave_kernel", "wave_preload"):
        d.set_option(name, -1)


_inputs_cache = {}


def _inputs(k, N):
    """synthetic.make_kernel_inputs(k, N, W=300, seed=7), made once per shape and never written to."""
    if (k, N) not in _inputs_cache:
        inp = synthetic.make_kernel_inputs(k, N, W, seed=SEED)
        for v in inp.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _inputs_cache[(k, N)] = inp
    return _inputs_cache[(k, N)]


def _kw(inp, **over):
    kw = dict(panel=inp["panel"], start=inp["start"], n_r=inp["n_r"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"],
              m=inp["m"], w0=inp["w0"], n0=inp["n0"])
    kw.update(over)
    return kw


def _both_forms(native, dev, strategy, k, N, kw, shared=True):
    """One upload, one run per form: ((weights, status, aux) of the pair, of the one kernel)."""
    b = native.Batch(dev, strategy, k, N, kw["n_r"], GAMMA, W, kw["m"])
    try:
        b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
        if shared:
            assert b.shared_gram_blocks() > 0
        else:
            assert b.shared_gram_blocks() == 0
        out = []
        for form in (0, 1):
            dev.set_option("shared_tables", form)
            b.run()
            out.append(b.download())
            assert dev.get_option("last_shared_tables") == (form if shared else -1)
        return out
    finally:
        dev.set_option("shared_tables", -1)
        b.close()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _assert_same_bytes(pair, one):
    for name, p, o in zip(("weights", "status", "aux"), pair, one):
        assert p.shape == o.shape and p.dtype == o.dtype
        diff = _bits(p) != _bits(o)
        assert not diff.any(), f"{name}: {int(diff.sum())} elements differ, first at {np.argwhere(diff)[0].tolist()}"


def _assert_oracle(strategy, k, N, kw, one):
    ref, rstat, raux = oracle.posterior_batch_c(strategy, k, N, GAMMA, **kw)
    w, s, a = one
    print(f"{strategy} k={k}: |one kernel - oracle| = {np.abs(w - ref).max():.3e}")
    assert (s == rstat).all(), (s, rstat)
    np.testing.assert_allclose(w, ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(a[:, :6], raux[:, :6], rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("k", SHAPES)
def test_tile_counts_and_kernel_families(native, dev, k, strategy):
    N = 251
    kw = _kw(_inputs(k, N))
    pair, one = _both_forms(native, dev, strategy, k, N, kw)
    _assert_same_bytes(pair, one)
    assert (one[1] == 0).all(), np.flatnonzero(one[1])[:10]
    if k in ORACLE_SHAPES and strategy == "conjugate":
        _assert_oracle(strategy, k, N, kw, one)


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_the_multi_wave_kernel(native, dev, strategy):
    """wave_kernel = 0: four waves per window read the same tables."""
    k, N = 100, 251
    kw = _kw(_inputs(k, N))
    dev.set_option("wave_kernel", 0)
    pair, one = _both_forms(native, dev, strategy, k, N, kw)
    _assert_same_bytes(pair, one)
    assert (one[1] == 0).all()
    if strategy == "conjugate":
        _assert_oracle(strategy, k, N, kw, one)


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_the_one_wave_kernel_without_preload(native, dev, strategy):
    """wave_preload = 0: the form that adds the slot to the accumulators after the intraday rows."""
    k, N = 100, 251
    kw = _kw(_inputs(k, N))
    dev.set_option("wave_preload", 0)
    pair, one = _both_forms(native, dev, strategy, k, N, kw)
    _assert_same_bytes(pair, one)
    assert (one[1] == 0).all()


# whole 16-row blocks per window: 1 / 2, 2 / 3, 14 / 15, 16 / 17 (across the group length), 17 / 18 (the middle sum is one
# or two blocks), 31 / 32
@pytest.mark.parametrize("N,strategy", [(34, "conjugate"), (49, "conjugate"), (49, "jeffreys"), (251, "conjugate"),
                                        (251, "jeffreys"), (273, "conjugate"), (273, "jeffreys"), (301, "conjugate"),
                                        (301, "jeffreys"), (521, "conjugate"), (521, "jeffreys")])
def test_block_counts_per_window(native, dev, N, strategy):
    k = 40
    kw = _kw(_inputs(k, N))
    pair, one = _both_forms(native, dev, strategy, k, N, kw)
    _assert_same_bytes(pair, one)
    assert (one[1] == 0).all(), np.flatnonzero(one[1])[:10]


def _block_counts(start, n_rows, blk=16):
    return (start + n_rows) // blk - (start + blk - 1) // blk


def _mixed_rows(inp, lengths, allowed):
    """Per-window row counts drawn from `lengths`, redrawn as 300 wherever the window's whole-block count would fall
    outside `allowed` (a batch gets at most four tables: a fifth distinct count switches sharing off)."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    n_rows = rng.choice(np.asarray(lengths, dtype=np.int32), size=W).astype(np.int32)
    bad = ~np.isin(_block_counts(inp["start"], n_rows), allowed)
    n_rows[bad] = 300
    return n_rows


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("lengths,allowed", [((300, 270), (18, 17, 16)), ((300, 270, 250), (18, 17, 16, 15))])
def test_three_and_four_tables_in_one_batch(native, dev, lengths, allowed, strategy):
    """Row counts 300 (17 or 18 whole blocks by the start's offset), 270 (15 / 16) and 250 (14 / 15), kept to the starts
    where the count is one of three or four values.  (Drawn freely from {300, 270, 250, 200} the counts would take up to
    eight values and the batch would not share at all; 200 rows - 11 / 12 blocks - are the fifth count of the test below.)"""
    k, N = 40, 301
    inp = _inputs(k, N)
    n_rows = _mixed_rows(inp, lengths, allowed)
    assert sorted(set(_block_counts(inp["start"], n_rows).tolist())) == sorted(allowed)
    assert all((n_rows == n).any() for n in lengths)
    pair, one = _both_forms(native, dev, strategy, k, N, _kw(inp, n_rows=n_rows))
    _assert_same_bytes(pair, one)
    assert (one[1] == 0).all(), np.flatnonzero(one[1])[:10]


def test_a_fifth_block_count_switches_sharing_off_in_both_forms(native, dev):
    k, N = 40, 301
    inp = _inputs(k, N)
    n_rows = _mixed_rows(inp, (300, 270, 250), (18, 17, 16, 15))
    n_rows[150] = 200
    assert len(set(_block_counts(inp["start"], n_rows).tolist())) == 5
    pair, one = _both_forms(native, dev, "conjugate", k, N, _kw(inp, n_rows=n_rows), shared=False)
    _assert_same_bytes(pair, one)
    assert (one[1] == 0).all()


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_a_panel_whose_rows_are_no_multiple_of_the_block(native, dev, strategy):
    """W - 1 + N = 550 rows: 34 whole blocks and 6 rows no table holds.  The batch is the k = 100 one of
    test_tile_counts_and_kernel_families; this case pins the precondition, so that a change of the generator which made
    the panel a whole number of blocks would not go unnoticed."""
    k, N = 100, 251
    inp = _inputs(k, N)
    assert inp["panel"].shape[0] % 16 != 0
    pair, one = _both_forms(native, dev, strategy, k, N, _kw(inp))
    _assert_same_bytes(pair, one)
    assert (one[1] == 0).all()


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
@pytest.mark.parametrize("value", [np.nan, 1e200])
def test_a_bad_row_spoils_exactly_the_windows_that_contain_it(native, dev, value, strategy):
    """Additions only: the row reaches a window through its slot or its edge rows and nobody else - every other window has
    the bits of the batch without the bad row, in both forms."""
    k, N = 100, 251
    inp = _inputs(k, N)
    panel = inp["panel"].copy()
    r_bad = panel.shape[0] // 2
    panel[r_bad, :] = value
    contains = (inp["start"] <= r_bad) & (r_bad < inp["start"] + inp["n_r"])
    assert 0 < contains.sum() < W
    pair, one = _both_forms(native, dev, strategy, k, N, _kw(inp, panel=panel))
    _assert_same_bytes(pair, one)
    clean_pair, clean_one = _both_forms(native, dev, strategy, k, N, _kw(inp))
    for got, clean in ((pair, clean_pair), (one, clean_one)):
        assert (got[1][contains] != 0).all(), np.flatnonzero(got[1] == 0)[:10]
        assert (got[1][~contains] == 0).all(), np.flatnonzero((got[1] != 0) & ~contains)[:10]
        for g, c in zip(got, clean):
            assert np.array_equal(_bits(g[~contains]), _bits(c[~contains]))


def test_the_option_contract(native, dev):
    """shared_tables takes -1, 0 and 1 and nothing else; -1 runs the one kernel at the flagship's seven tiles per side."""
    for bad in (2, -2):
        with pytest.raises(native.TangencyError) as e:
            dev.set_option("shared_tables", bad)
        assert e.value.code == native.TP_ERR_INVALID
    assert dev.get_option("shared_tables") == -1
    k, N = 100, 251
    kw = _kw(_inputs(k, N))
    b = native.Batch(dev, "conjugate", k, N, kw["n_r"], GAMMA, W, kw["m"])
    try:
        b.upload(**{key: val for key, val in kw.items() if key not in ("n_r", "m")})
        assert b.shared_gram_blocks() > 0
        got = {}
        for form in (-1, 0, 1):
            dev.set_option("shared_tables", form)
            assert dev.get_option("shared_tables") == form
            b.run()
            got[form] = (dev.get_option("last_shared_tables"), b.download())
    finally:
        b.close()
    assert got[-1][0] == 1 and got[0][0] == 0 and got[1][0] == 1
    _assert_same_bytes(got[-1][1], got[1][1])
    # a batch without shared sums reports that it built no tables
    w, s, _ = native.posterior_batch("conjugate", k, N, GAMMA, flags=native.FLAG_NO_SHARED_GRAM, device=dev, **kw)
    assert dev.get_option("last_shared_tables") == -1 and (s == 0).all()
