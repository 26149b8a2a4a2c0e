"""`portfolio_calculations._greyserman_from_spectrum` - the numpy mirror of the spectral ridge sweep - on the CPU: fed
`numpy.linalg.eigh` it is held to the long-double truth of tests/_spectral_reference.py and to `_greyserman_from_solves` fed
fp64 solves, on the shapes of tests/test_gpu_spectral.py.  Every case asserts the conditions of the finish's bound
(`assert_greyserman_case`): the seeds of `_spectral_reference.seed_of` are chosen so that they hold.

Two rules, the GPU test's: (i) the project's flat 1e-10 (the cases have max |w| of about 1); (ii) the spectral error is at most
16 x max(the solves' error, the finish's bound 2^-53 (k + S + 32) max M), both errors against the same truth."""
import numpy as np
import pytest

from incorporating_different_sources_amd import portfolio_calculations as pc

import _spectral_reference as sref
import _sweep_finish_reference as ref

FLAT = 1e-10
FACTOR = 16.0


@pytest.mark.parametrize("k,n,S", sref.CASES)
def test_from_spectrum_against_the_truth_and_the_solves(k, n, S):
    X, xi, eta, M, t, truth = sref.host_case(k, n, S)
    sref.assert_case(truth, k, n, S)
    lam, V = np.linalg.eigh(M)
    nn = np.array([float(n)])
    got = pc._greyserman_from_spectrum(lam[None], V[None], t[None], nn, xi[None], eta[None], k, sref.GAMMA)[0]
    A = M[None, :, :] + (eta / 2)[:, None, None] * np.eye(k)[None]
    u_t = np.linalg.solve(A, np.repeat(t[None, :, None], S, axis=0))[:, :, 0]
    u_one = np.linalg.solve(A, np.ones((S, k, 1)))[:, :, 0]
    solves = pc._greyserman_from_solves(u_t[None], u_one[None], t[None], nn, xi[None], eta[None], k, sref.GAMMA)[0]
    err, err_solves = float(np.abs(got - truth["weights"]).max()), float(np.abs(solves - truth["weights"]).max())
    bound = ref.bound(k, S, truth["M"])
    print(f"k={k} n={n} S={S}: max|w| {np.abs(truth['weights']).max():.3g} spectrum {err:.3e} solves {err_solves:.3e} bound {bound:.3e}")
    assert err <= FLAT
    assert err <= FACTOR * max(err_solves, bound)


def test_from_spectrum_is_vectorised_over_windows():
    cases = [sref.host_case(65, 105, S) for S in (16,)] + [sref.host_case(65, 40, sref.S_MAIN)]
    one = []
    for (X, xi, eta, M, t, _truth), n in zip(cases, (105, 40)):
        lam, V = np.linalg.eigh(M)
        one.append(pc._greyserman_from_spectrum(lam[None], V[None], t[None], [float(n)], xi[None, :16], eta[None, :16], 65, 3.0)[0])
    lamV = [np.linalg.eigh(c[3]) for c in cases]
    both = pc._greyserman_from_spectrum(np.stack([e[0] for e in lamV]), np.stack([e[1] for e in lamV]),
                                        np.stack([c[4] for c in cases]), [105.0, 40.0],
                                        np.stack([c[1][:16] for c in cases]), np.stack([c[2][:16] for c in cases]), 65, 3.0)
    np.testing.assert_allclose(both, np.stack(one), rtol=1e-13, atol=1e-15)
