"""The group dispatch the tiled solve sweep and the tiled size sweep share (csrc/posterior_tiled_sweep_prims.h: back_substitute,
for_each_group): columns / sizes are back-substituted in groups of up to 4, and both kernel files promise that a column's /
size's arithmetic does not depend on which other columns share its group.  Asserted here as bit-identity at the smallest shapes
where the dispatch can go wrong, with the arena's geometry held equal: k = 144 is the first tiled k - three pivot block rows,
the last with 16 pivots - and k + R <= 192, k + S <= 192 keep KP = 192 for every list length, a list of one included; k = 193
has one pivot in its last block (KP = 256 for R = 1 and R = 5 alike).  The oracle comparison of these shapes is
test_gpu_solve_sweep_tiled.py's and test_gpu_size_sweep_tiled.py's and is not repeated.  -m gpu."""
import numpy as np
import pytest

from incorporating_different_sources_amd import _native, synthetic

import _size_sweep_tiled_cases as size_cases
from _tiled_sweep_cases import make_shift

pytestmark = pytest.mark.gpu

GAMMA = 5.0
W = 2
OK = _native.STATUS_OK
SIZES = [16, 63, 64, 65, 128, 129, 144]                    # all three blocks; groups (16, 63, 64, 65) and (128, 129, 144)


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


# R: remainders 1, 2, 3, a full group of 4, and 4 + 3; k = 193: 4 + 1 with one pivot in the last block
@pytest.mark.parametrize("k,counts", [(144, (1, 2, 3, 4, 7)), (193, (5,))], ids=["k144", "k193"])
def test_solve_sweep_column_does_not_depend_on_its_group(dev, k, counts):
    N, R = 2 * k + 24, max(counts)
    assert -(-(k + 1) // 64) == -(-(k + R) // 64)          # one geometry for every R
    inp = synthetic.make_kernel_inputs(k, N, W, seed=970000 + k)
    rng = np.random.default_rng(970000 + k)
    shift = make_shift(rng, W, 2)
    rhs = rng.normal(size=(W, R, k))
    b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W, 0)
    try:
        b.upload(inp["panel"], start=inp["start"])
        alone = [b.solve_sweep_tiled(shift=shift, rhs=rhs[:, r:r + 1], default_rhs=False) for r in range(R)]
        for x, status in alone:
            assert (status == OK).all() and np.isfinite(x).all()
        for n in counts:
            x, status = b.solve_sweep_tiled(shift=shift, rhs=rhs[:, :n], default_rhs=False)
            assert x.shape == (W, 2, n, k) and (status == OK).all()
            for r in range(n):
                same = np.array_equal(x[:, :, r], alone[r][0][:, :, 0])
                print(f"k={k} R={n} column {r}: bit-identical to the column alone: {same}, "
                      f"max|diff| = {np.abs(x[:, :, r] - alone[r][0][:, :, 0]).max():.3e}")
                assert same, f"k={k}: column {r} of {n} differs from the column solved alone"
    finally:
        b.close()


@pytest.mark.parametrize("strategy", ["conjugate", "jeffreys"])
def test_size_sweep_size_does_not_depend_on_its_group(dev, strategy):
    k, P = 144, 2
    N = 2 * k + 24
    assert k + len(SIZES) <= 192                           # KP = 192 for the list and for every size alone
    inp = synthetic.make_kernel_inputs(k, N, W, seed=971000, hf_days=2)
    conj = strategy == "conjugate"
    b = dev.batch(strategy, k, N, inp["n_r"], GAMMA, W, inp["m"] if conj else 0)
    try:
        if conj:
            n0, w0 = size_cases.make_size_priors(np.random.default_rng(971000), W, P, SIZES, k, N)
            b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
            sweep = lambda slots: b.size_sweep_tiled([SIZES[s] for s in slots], n0, np.ascontiguousarray(w0[:, :, slots]))
        else:
            b.upload(inp["panel"], start=inp["start"])
            sweep = lambda slots: b.size_sweep_tiled([SIZES[s] for s in slots])
        full = sweep(list(range(len(SIZES))))
        assert (full[1] == OK).all(), full[1]
        for s, ks in enumerate(SIZES):
            assert np.isfinite(full[0][:, :, s]).all() and not full[0][:, :, s, ks:].any()     # exactly zero beyond k_s
            one = sweep([s])
            for what, a, f in zip(("weights", "status", "aux"), one, full):
                same = np.array_equal(a[:, :, 0], f[:, :, s])
                print(f"{strategy} k_s={ks} alone: {what} bit-identical to the list of {len(SIZES)}: {same}")
                assert same, f"{strategy}: {what} of k_s={ks} alone differ from the list's"
    finally:
        b.close()
