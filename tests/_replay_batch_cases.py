"""Helpers of the device-fed replay's tests, shared by tests/test_gpu_replay_batch.py (k <= 513) and
tests/test_gpu_replay_batch_large.py (the class edges up to k = 2047, patches and flagged rows above 512 assets, tiled sweeps as
sources).  `_jeffreys_batch`, `_common`, `_yardstick` and `_scales` came from tests/test_gpu_replay_batch.py unchanged.  No tests
in here."""
import numpy as np

GAMMA = 5.0


def _jeffreys_batch(dev, rng, k, W, n_r=None, poison=None):
    """W disjoint windows of n_r > k random normal rows (every window positive definite); `poison`: (window, row, column) of
    one NaN in the daily panel."""
    n_r = n_r or k + 24
    panel = rng.normal(0.0, 1.0, (W * n_r, k))
    if poison is not None:
        panel[poison[0] * n_r + poison[1], poison[2]] = np.nan
    b = dev.batch("jeffreys", k, n_r, n_r, GAMMA, W)
    b.upload(panel, start=np.arange(W, dtype=np.int64) * n_r)
    return b


def _common(rng, R, K, D=None, gap=3):
    """Returns, risk-free rates and a rebalancing schedule with single days and longer stretches between the dates."""
    reb_day = np.cumsum([0] + [1 + (j * gap) % 5 for j in range(R - 1)]).astype(np.int32)
    D = D or int(reb_day[-1]) + 3
    S = rng.normal(0.0005, 0.02, (D, K))
    S[2:4, 0] = np.nan
    return dict(S=S, rf_daily=0.0001 * rng.random(D), reb_day=reb_day, K=K)


def _yardstick(dev, common, ks, universe, src, w_off, w_stride, gammas=None, patches=None):
    """`Device.replay` on rows formed on the host: portfolio p's row of date j is src.flat[w_off[p] + j w_stride[p] : + k[p]],
    as `1.0 / g * w` where a risk aversion g is given, replaced - unscaled - by a patch row where (p, j) is patched."""
    R = len(common["reb_day"])
    src = np.asarray(src).reshape(-1)
    dense = []
    for p, k in enumerate(ks):
        rows = np.stack([src[w_off[p] + j * w_stride[p]: w_off[p] + j * w_stride[p] + k] for j in range(R)])
        if gammas is not None and gammas[p] is not None:
            rows = 1.0 / gammas[p] * rows
        else:
            rows = rows.copy()
        if patches is not None:
            for q, (pp, jj) in enumerate(zip(patches[0], patches[1])):
                if pp == p:
                    rows[jj] = patches[2][q, :k]
        dense.append(rows.reshape(-1))
    ks = np.asarray(ks, dtype=np.int32)
    lens = R * ks.astype(np.int64)
    return dev.replay(weights=np.concatenate(dense), w_off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64),
                      w_stride=ks.astype(np.int64), k=ks, **common, **universe)


def _scales(gammas):
    return np.array([1.0 if g is None else 1.0 / g for g in gammas])
