"""Float64 host evaluation of the symplectic defect of monodromy blocks and the rounding bound the GPU tests hold it to.

Every element of E1 = A^T C - C^T A, E2 = A^T D - C^T B - 1, E3 = B^T D - D^T B is a sum of m = 2D products (plus the 1 on the
diagonal of E2); in any summation order, fused or not, its rounding error is at most gamma_{m+1} S_ab with S_ab the same
expression of absolute values and gamma_k = k u / (1 - k u), u = 2^-53.  The scaling adds two roundings.  This evaluation and
the kernel's each carry that bound, so they differ by at most 2 gamma_{2D+5} max_ab(w_ab S_ab) per trajectory and block.
"""
import numpy as np

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def _t(x):
    return np.swapaxes(x, 1, 2)


def weights(scale):
    """scale factors w_ab of the three blocks, (3, D, D)"""
    s = np.asarray(scale, dtype=np.float64)
    return np.stack((1.0 / (s[:, None] * s[None, :]), s[None, :] / s[:, None], s[:, None] * s[None, :]))


def deviation_and_bound(blocks, scale):
    """blocks (n, 4, D, D) = Mqq, Mqp, Mpq, Mpp of n trajectories -> (dev (n, 3), bound (n, 3))"""
    blocks = np.asarray(blocks, dtype=np.float64)
    A, B, C, Dm = (blocks[:, k] for k in range(4))
    D = A.shape[1]
    eye = np.eye(D)
    s = np.asarray(scale, dtype=np.float64)
    E = (_t(A) @ C - _t(C) @ A, _t(A) @ Dm - _t(C) @ B - eye, _t(B) @ Dm - _t(Dm) @ B)
    aA, aB, aC, aD = (np.abs(x) for x in (A, B, C, Dm))
    S = (_t(aA) @ aC + _t(aC) @ aA, _t(aA) @ aD + _t(aC) @ aB + 1.0, _t(aB) @ aD + _t(aD) @ aB)
    sa, sb = s[:, None], s[None, :]
    scaled = (E[0] / (sa * sb), E[1] * sb / sa, E[2] * sa * sb)       # the kernel's order of the two roundings
    w = weights(s)
    dev = np.stack([np.abs(x).reshape(len(x), -1).max(axis=1) for x in scaled], axis=1)
    bound = np.stack([2.0 * gamma(2 * D + 5) * (w[k] * S[k]).reshape(len(S[k]), -1).max(axis=1) for k in range(3)], axis=1)
    return dev, bound


def blocks_from_matrices(mats):
    """the propagator's monodromy_matrices() -- four (D, D, n) tensors -- as (n, 4, D, D) float64"""
    return np.stack([np.asarray(m.detach().cpu().numpy()).transpose(2, 0, 1) for m in mats], axis=1)


def blocks_from_y(y, D):
    """the monodromy rows of a state in the reference's layout (2D + 4 D^2 + 1, n) as (n, 4, D, D)"""
    y = np.asarray(y)
    return np.ascontiguousarray(y[2 * D:2 * D + 4 * D * D].T).reshape(-1, 4, D, D)


def y_from_blocks(blocks):
    """a reference-layout state with q = p = S = 0 and the given monodromy blocks (n, 4, D, D)"""
    blocks = np.asarray(blocks, dtype=np.float64)
    n, _, D, _ = blocks.shape
    y = np.zeros((2 * D + 4 * D * D + 1, n))
    y[2 * D:2 * D + 4 * D * D] = blocks.reshape(n, 4 * D * D).T
    return y
