"""Quartic force field: a numpy restatement of the folded forms of DESIGN.md section 4.18 (evaluated in any dtype, the tests take
np.longdouble as the reference), the literally written Taylor sum over the derivative arrays, random constants, and the rounding
bound the tests hold every entry to."""
import functools
import itertools

import numpy as np

PARTS = ("all", "cubic", "quartic", "none")


def gamma(D):
    """rounding bound per unit of the sum of the absolute values of an entry's terms: every sum of section 4.18 has at most D + 8
    terms behind a product of at most four factors; 4 covers the products, the folded constants and the subtraction r - pos0"""
    return 4.0 * (D + 8) * 2.0 ** -53


def symmetrise(a):
    perms = [np.transpose(a, p) for p in itertools.permutations(range(a.ndim))]
    s = np.sort(np.stack(perms), axis=0)
    return np.ascontiguousarray(s[0] + (s[1:] - s[0]).sum(axis=0) / len(perms))


def random_constants(D, seed, parts="all"):
    """derivative arrays of a random force field with displacements of order one: every part contributes at the same order"""
    rng = np.random.default_rng([D, seed])
    c = {"pos0": rng.normal(0, 1.0, D), "energy0": np.float64(rng.normal()), "grad0": rng.normal(0, 1.0, D),
         "hess0": symmetrise(rng.normal(0, 1.0, (D, D))), "masses": rng.uniform(0.8, 1.6, D), "nac0": rng.normal(0, 1e-3, D),
         "cubic": None, "quartic_iijj": None, "quartic_iiij": None}
    if parts in ("all", "cubic"):
        c["cubic"] = symmetrise(rng.normal(0, 1.0, (D, D, D)))
    if parts in ("all", "quartic"):
        c["quartic_iijj"] = symmetrise(rng.normal(0, 1.0, (D, D)))
        b = rng.normal(0, 1.0, (D, D))
        b[np.diag_indices(D)] = 0.0
        c["quartic_iiij"] = b
    return c


def geometries(c, n, seed=0):
    """r [n][D] around pos0"""
    rng = np.random.default_rng([len(c["pos0"]), n, seed])
    return c["pos0"][None, :] + rng.normal(0, 1.0, (n, len(c["pos0"])))


def fold(c):
    """A_ij = u_iijj / 8 (i != j), A_ii = u_iiii / 24, B_ij = u_iiij / 6"""
    A = B = None
    if c["quartic_iijj"] is not None:
        u = np.asarray(c["quartic_iijj"])
        A = u / 8.0
        A[np.diag_indices(len(u))] = np.diag(u) / 24.0
    if c["quartic_iiij"] is not None:
        B = np.asarray(c["quartic_iiij"]) / 6.0
    return A, B


def folded_forms(e0, g, H, t, A, B, x):
    """E [n], grad [n][D], hess [n][D][D] at the displacements x [n][D], in the dtype of the arguments"""
    n, D = x.shape
    y, z = x * x, x * x * x
    Hx = x @ H.T
    E = e0 + x @ g + 0.5 * np.sum(x * Hx, axis=1)
    grad = g[None, :] + Hx
    hess = np.broadcast_to(H[None], (n, D, D)).copy()
    if t is not None:
        W = np.tensordot(x, t, axes=([1], [2]))                     # [n][i][j] = sum_k t_ijk x_k
        Wx = np.einsum('nij,nj->ni', W, x)
        E = E + np.sum(x * Wx, axis=1) / 6
        grad = grad + Wx / 2
        hess = hess + W
    diag = np.zeros_like(x)
    if A is not None:
        Ay = y @ A.T
        E = E + np.sum(y * Ay, axis=1)
        grad = grad + 4 * x * Ay
        hess = hess + 8 * A[None] * x[:, :, None] * x[:, None, :]
        diag = diag + 4 * Ay
    if B is not None:
        Bx = x @ B.T
        E = E + np.sum(z * Bx, axis=1)
        grad = grad + 3 * y * Bx + z @ B
        hess = hess + 3 * B[None] * y[:, :, None] + 3 * B.T[None] * y[:, None, :]
        diag = diag + 6 * x * Bx
    idx = np.arange(D)
    hess[:, idx, idx] += diag
    return E, grad, hess


def evaluate(c, r, dtype=np.longdouble, origin=0.0):
    """the folded forms in ``dtype`` and, with them, the sums of the absolute values of every entry's terms (float64)"""
    cast = lambda a: None if a is None else np.asarray(a, dtype=dtype)
    A, B = fold(c)
    x = cast(r) - cast(c["pos0"])[None, :]
    args = [cast(c["energy0"]) - dtype(origin), cast(c["grad0"]), cast(c["hess0"]), cast(c["cubic"]), cast(A), cast(B)]
    E, grad, hess = folded_forms(*args, x)
    mag = folded_forms(*[None if a is None else np.abs(np.asarray(a, dtype=np.float64)) for a in args],
                       np.abs(x.astype(np.float64)))
    return (E, grad, hess), mag


@functools.lru_cache(maxsize=None)
def case(D, parts, n, seed=0):
    """constants, geometries r [n][D], the np.longdouble reference and the magnitudes, computed once per shape and shared"""
    c = random_constants(D, seed, parts)
    r = geometries(c, n, seed)
    ref, mag = evaluate(c, r)
    for a in (r,) + ref + mag:
        a.setflags(write=False)
    return c, r, ref, mag


def within_bound(got, ref, mag, D):
    """largest |got - ref| / (gamma(D) * magnitude) over the entries: <= 1 passes"""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - ref).astype(np.float64)
    return float(np.max(err / (gamma(D) * mag + np.finfo(np.float64).tiny)))


def taylor_sum(c, x):
    """V at ONE displacement x (torch tensor, D) as the six sums over the DERIVATIVE arrays written out, no folding (torch, so
    that autograd differentiates it): pins the factorial factors"""
    import torch
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    D = x.shape[0]
    V = T(c["energy0"]) + torch.einsum('i,i->', T(c["grad0"]), x) + 0.5 * torch.einsum('i,ij,j->', x, T(c["hess0"]), x)
    if c["cubic"] is not None:
        V = V + torch.einsum('ijk,i,j,k->', T(c["cubic"]), x, x, x) / 6.0
    if c["quartic_iijj"] is not None:
        u = T(c["quartic_iijj"])
        for i in range(D):
            V = V + u[i, i] * x[i] ** 4 / 24.0
            for j in range(i + 1, D):
                V = V + u[i, j] * x[i] ** 2 * x[j] ** 2 / 4.0
    if c["quartic_iiij"] is not None:
        v = T(c["quartic_iiij"])
        for i in range(D):
            for j in range(D):
                if i != j:
                    V = V + v[i, j] * x[i] ** 3 * x[j] / 6.0
    return V


def potential(c, origin=0.0):
    from semiclassical_amd.potentials import QuarticForceFieldPotential
    return QuarticForceFieldPotential.from_arrays(c["pos0"], c["energy0"], c["grad0"], c["hess0"], cubic=c["cubic"],
                                                  quartic_iijj=c["quartic_iijj"], quartic_iiij=c["quartic_iiij"],
                                                  masses=c["masses"], nac0=c["nac0"], origin=origin)
