"""The truth of the sweep-finish tests (tests/test_host_sweep_finish.py, tests/test_gpu_sweep_finish.py): the Greyserman and
Jorion finishes of `portfolio_calculations._greyserman_from_solves` / `_jorion_from_solves` from GIVEN solutions, in
numpy.longdouble, every sum sequential.  Next to the weights it returns what the tests' bound is made of - per output element
the sum of the absolute values of its terms - and the cancellation ratios sum|terms| / |result| of the differences the bound's
validity depends on.  No tests in here.

The bound (per window):  |got - truth|_j <= 2^-53 (k + S + 32) amp max_j M_j
  - k stands for the k-term sums, S for the S-term mean, 32 for the scalar operations;
  - amp = 1 for Greyserman, the window's cancellation ratio of q for Jorion;
  - valid while ratio(K12) <= 64, ratio(K22) <= 8, ratio(det) <= 2 (Greyserman, every draw) and ratio(q) <= 32 (Jorion): the
    case builders assert these on the CPU."""
import numpy as np

L = np.longdouble
EPS = 2.0 ** -53
GREYSERMAN_RATIO_LIMITS = {"K12": 64.0, "K22": 8.0, "det": 2.0}
JORION_RATIO_LIMIT = 32.0


def greyserman_kappa(n):
    """Python's round(0.1 n) (ref:920), as the host forms it."""
    return float(round(0.1 * float(n)))


def greyserman_truth(u_t, u_one, t, n, kappa, xi, eta, gamma):
    """One window.  u_t, u_one [S x k] (the solves for t and for the ones vector), t [k], xi and eta [S].  Returns a dict:
    weights [k] (float64 of the long-double result), M [k], ratios {K12, K22, det} (the worst over the draws), aux [S x 4] =
    (s1, s2, s3, det)."""
    ut, uo, tt = np.asarray(u_t, dtype=L), np.asarray(u_one, dtype=L), np.asarray(t, dtype=L)
    xi, eta = np.asarray(xi, dtype=L), np.asarray(eta, dtype=L)
    S, k = ut.shape
    n, kappa, gamma = L(n), L(kappa), L(gamma)
    s1, s2, s3 = np.zeros(S, L), np.zeros(S, L), np.zeros(S, L)
    for j in range(k):                                        # sequential in j, vectorised over the draws
        s1 = s1 + uo[:, j]
        s2 = s2 + ut[:, j]
        s3 = s3 + tt[j] * ut[:, j]
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = eta / 2 + kappa * xi * xi
        K11 = 1 / beta + s1
        p12 = kappa * xi / beta
        K12 = s2 - p12
        p22 = kappa * eta / (2 * beta)
        K22 = s3 - n - p22
        det = K11 * K22 - K12 * K12
        ratios = {"K12": float(np.max((np.abs(s2) + np.abs(p12)) / np.abs(K12))),
                  "K22": float(np.max((np.abs(s3) + np.abs(n) + np.abs(p22)) / np.abs(K22))),
                  "det": float(np.max((np.abs(K11 * K22) + K12 * K12) / np.abs(det)))}
        c = (1 / gamma) * (k + n + 1) * (1 - 1 / n)
        cA, cB = K12 / det, K11 / det
        w, M = np.zeros(k, L), np.zeros(k, L)
        for s in range(S):                                    # sequential in s
            a_, b_ = cA[s] * uo[s], cB[s] * ut[s]
            w = w + c * (a_ - b_)
            M = M + (np.abs(a_) + np.abs(b_))
    return {"weights": (w / S).astype(np.float64), "M": (np.abs(c) * M / S).astype(np.float64), "ratios": ratios,
            "aux": np.stack([s1, s2, s3, det], axis=1).astype(np.float64)}


def jorion_truth(x_t, x_one, t, T, gamma):
    """One window.  x_t, x_one, t [k].  Returns a dict: weights [k], M [k] (the sum of the absolute values of the three terms
    of every element), ratio_q, aux [4] = (s1, s2, s3, q)."""
    xt, xo, tt = np.asarray(x_t, dtype=L), np.asarray(x_one, dtype=L), np.asarray(t, dtype=L)
    k = xt.shape[0]
    T, N, gamma = L(T), L(k), L(gamma)
    kap = (T - N - 2) * (T - 1) / T
    mu = tt / T
    a = kap * xt / T
    b = kap * xo
    s1 = s2 = s3 = s_bb = s_ab = s_aa = L(0)
    for j in range(k):
        s1, s2, s3 = s1 + xo[j], s2 + xt[j], s3 + tt[j] * xt[j]
        s_bb, s_ab, s_aa = s_bb + b[j], s_ab + a[j], s_aa + mu[j] * a[j]
    mu_g = s_ab / s_bb
    q_terms = (s_aa, 2 * mu_g * s_ab, mu_g * mu_g * s_bb)
    q = q_terms[0] - q_terms[1] + q_terms[2]
    lam = (N + 2) / q
    v = (N + 2) / ((N + 2) + T * q)
    alpha = 1 + 1 / (T + lam)
    beta = lam / (T * (T + 1 + lam)) / s_bb
    g = (1 - v) * a + v * mu_g * b
    g_sum = L(0)
    for j in range(k):
        g_sum = g_sum + g[j]
    t1 = (1 - v) * a / alpha
    t2 = v * mu_g * b / alpha
    t3 = (beta / alpha ** 2) * b * g_sum / (1 + (beta / alpha) * s_bb)
    return {"weights": ((t1 + t2 - t3) / gamma).astype(np.float64),
            "M": ((np.abs(t1) + np.abs(t2) + np.abs(t3)) / np.abs(gamma)).astype(np.float64),
            "ratio_q": float(sum(abs(x) for x in q_terms) / abs(q)),
            "aux": np.array([s1, s2, s3, q], dtype=np.float64)}


def bound(k, S, M, amp=1.0):
    """The tests' bound for one window: a scalar."""
    return EPS * (k + S + 32) * amp * float(np.max(M))


def assert_greyserman_case(truth, what=""):
    for name, limit in GREYSERMAN_RATIO_LIMITS.items():
        assert truth["ratios"][name] <= limit, f"{what}: ratio({name}) = {truth['ratios'][name]:.3g} > {limit}: pick another seed"


def assert_jorion_case(truth, what=""):
    assert truth["ratio_q"] <= JORION_RATIO_LIMIT, f"{what}: ratio(q) = {truth['ratio_q']:.3g} > {JORION_RATIO_LIMIT}: pick another seed"


def one_factor_window(k, n, seed):
    """X [n x k]: the project's one-factor synthetic returns (synthetic.make_kernel_inputs' daily panel)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    beta = rng.uniform(0.5, 1.5, size=k)
    f = rng.normal(0.0, 0.01, size=n)
    return 3e-4 + f[:, None] * beta[None, :] + rng.normal(0.0, 0.01, size=(n, k))


def draws(S, seed):
    """(xi [S], eta [S]) with the distributions of ref:926-927 from a generator of their own."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1000, 1000, size=S), rng.standard_gamma(1.0, size=S) * 10
