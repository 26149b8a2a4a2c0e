"""Every sweep family keeps results of its own on ONE batch: what a sweep's download returns does not change when another
sweep or a run follows it, and the batch's own results do not change either.  The library's downloads are called again through
`_native.lib` after all the sweeps and compared bit for bit with what each call returned.  -m gpu.

Shapes: k = 20 for the three sweeps of the register kernels (conjugate, W = 4); k = 150 for the two tiled sweeps (W = 3), where
the prior sweep borrows - and, with W P = 6 entries for 3 windows, grows - the workspace the following run uses."""
import ctypes

import numpy as np
import pytest

from incorporating_different_sources_amd import _native, synthetic

pytestmark = pytest.mark.gpu

GAMMA = 5.0


@pytest.fixture(scope="module")
def dev():
    d = _native.Device(0)
    yield d
    d.close()


def _p(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def again(b, call, *like):
    """`call(batch, arrays...)` of the library into fresh arrays shaped like `like`."""
    out = [np.full_like(a, -1) for a in like]
    cts = [ctypes.c_int32 if a.dtype == np.int32 else ctypes.c_double for a in out]
    b.dev._check(call(b._b, *[_p(a, ct) for a, ct in zip(out, cts)]))
    return out


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def priors(rng, W, P, k, N, S=None):
    n0 = N * rng.uniform(0.5, 2.0, size=(W, P))
    w0 = rng.dirichlet(np.ones(k), size=(W, P) if S is None else (W, P, S))
    return n0, w0


def conjugate_batch(dev, inp, k, N, W):
    b = dev.batch("conjugate", k, N, inp["n_r"], GAMMA, W, inp["m"])
    b.upload(inp["panel"], start=inp["start"], hf_panel=inp["hf_panel"], hf_start=inp["hf_start"], w0=inp["w0"], n0=inp["n0"])
    return b


def test_register_kernel_sweeps_and_the_run_keep_results_of_their_own(dev):
    k, N, W, P = 20, 60, 4, 2
    sizes = [7, 20]
    inp = synthetic.make_kernel_inputs(k, N, W, seed=120020)
    rng = np.random.default_rng(120020)
    b = conjugate_batch(dev, inp, k, N, W)
    first = b.run().download()
    assert (first[1] == _native.STATUS_OK).all()
    prior = b.prior_sweep(*priors(rng, W, P, k, N))
    solve = b.solve_sweep(rhs=rng.normal(size=(W, 2, k)))              # R = the default right-hand side + 2
    rhs0 = b.download_sweep_rhs()
    size = b.size_sweep(sizes, *priors(rng, W, P, k, N, S=len(sizes)))
    assert prior[0].shape == (W, P, k) and solve[0].shape == (W, 1, 3, k) and size[0].shape == (W, P, len(sizes), k)
    for status in (prior[1], solve[1], size[1]):
        assert (status == _native.STATUS_OK).all()
    lib = _native.lib
    assert same(again(b, lib.tp_batch_download_prior_sweep, *prior), prior)
    assert same(again(b, lib.tp_batch_download_sweep, *solve), solve)
    assert same(again(b, lib.tp_batch_download_sweep_rhs, rhs0), [rhs0])
    assert same(again(b, lib.tp_batch_download_size_sweep, *size), size)
    assert same(b.download(), first)
    b.close()


def test_tiled_sweeps_keep_their_results_through_a_run(dev):
    k, N, W = 150, 200, 3
    inp = synthetic.make_kernel_inputs(k, N, W, seed=120150)
    rng = np.random.default_rng(120150)
    lib = _native.lib

    b = conjugate_batch(dev, inp, k, N, W)
    prior = b.prior_sweep_tiled(*priors(rng, W, 2, k, N))
    assert (prior[1] == _native.STATUS_OK).all()
    ran = b.run().download()
    assert (ran[1] == _native.STATUS_OK).all()
    assert same(again(b, lib.tp_batch_download_prior_sweep, *prior), prior)
    b.close()

    b = dev.batch("jeffreys", k, N, inp["n_r"], GAMMA, W, 0, _native.FLAG_NO_CENTER)
    b.upload(inp["panel"], start=inp["start"])
    shift = np.stack([rng.gamma(1.0, 10.0, size=(W, 2)) / 2, rng.uniform(0.0, 50.0, size=(W, 2))], axis=2)
    solve = b.solve_sweep_tiled(shift=shift, rhs=rng.normal(size=(W, 1, k)))   # S = 2, R = the default + 1
    rhs0 = b.download_sweep_rhs()
    assert solve[0].shape == (W, 2, 2, k) and (solve[1] == _native.STATUS_OK).all()
    ran = b.run().download()
    assert (ran[1] == _native.STATUS_OK).all()
    assert same(again(b, lib.tp_batch_download_sweep, *solve), solve)
    assert same(again(b, lib.tp_batch_download_sweep_rhs, rhs0), [rhs0])
    b.close()
