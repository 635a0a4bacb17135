"""Entropy parameters over the edges of the table kernels (lic_gmm_cdf_tables), and the host view of the activated
parameters in the kernels' element order: shared by tests/test_codec.py and tests/test_gpu_codec_windows.py."""
import numpy as np


def edge_raw(r, K, M, P, W):
    """raw entropy parameters [1, G*K*M, P, 1] over the table kernels' edges: sigma at its 1e-6 floor and sigma far
    wider than the window; for K >= 2 saturated softmax weights and components more than W + 5 away from the weighted
    centre the window is placed on (their mass lands in the two tail symbols)"""
    if K == 1:
        mu = r.randn(P, M) * 8
        sg = r.randn(P, M) * 2
        sel = r.rand(P, M)
        sg[sel < 0.15] = -60.0                                    # softplus -> 0: sigma = 1e-6
        sg[sel > 0.85] = r.uniform(2e3, 1e4, size=(sel > 0.85).sum())   # sigma >> W
        return np.concatenate([mu, sg], 1).astype(np.float32).T.reshape(1, 2 * M, P, 1)
    wr, mus, sgs = r.randn(P, K, M), r.randn(P, K, M) * 8, r.randn(P, K, M) * 2
    sel = r.rand(P, M)
    sat = sel < 0.2                                               # one component takes all the weight
    wr[:, 0][sat], wr[:, 1:][np.broadcast_to(sat[:, None], (P, K - 1, M))] = 60.0, -60.0
    far = (sel >= 0.2) & (sel < 0.6)                              # component 0 dominant, the last one far away
    wr[:, 0][far] = 3.0 + np.log(K)
    side = np.where(r.rand(far.sum()) < 0.5, -1.0, 1.0)
    mus[:, K - 1][far] = mus[:, 0][far] + side * (3 * W + 20 + 10 * r.rand(far.sum()))
    s = r.rand(P, K, M)
    sgs[s < 0.15] = -60.0
    sgs[s > 0.9] = r.uniform(2e3, 1e4, size=(s > 0.9).sum())
    raw = np.concatenate([wr.reshape(P, K * M), mus.reshape(P, K * M), sgs.reshape(P, K * M)], 1)
    return raw.astype(np.float32).T.reshape(1, 3 * K * M, P, 1)


def split_act(a, K, M):
    """host act [P, G*K*M] -> (weights, mus, sigmas) [K, P*M] in the table kernels' element order"""
    P = a.shape[0]
    if K == 1:
        return np.ones((1, P * M), np.float32), a[:, :M].reshape(1, -1), a[:, M:].reshape(1, -1)
    T = K * M
    return tuple(a[:, i * T:(i + 1) * T].reshape(P, K, M).transpose(1, 0, 2).reshape(K, -1) for i in range(3))
