"""Shared pieces of the direct determinant tests (test_prefactor_det_host.py, test_prefactor_det_gpu.py): an extended-precision
reference determinant, matrix families that are hostile to a pivot search, encodings that make the prefactor matrix of
sc_dense_mono_step equal a chosen complex matrix A bit for bit, and a driver that hands such blocks to one of its three
determinant routes:

  R  dense_prefactor_reg_kernel<NR> + fix-up by the LDS kernel   diagonal widths, flags given, D <= 96
  L  dense_prefactor_kernel -> lds_lu_det on LDS                  flags == NULL, or dense / rank-deficient widths, D <= 96
  G  prefactor_any_kernel -> lds_lu_det on global scratch         D > 96
"""
import functools
import zlib

import numpy as np

LD, CLD = np.longdouble, np.clongdouble

# sizes at which each route changes shape (every NR with full and partial last tiles; 64 / 128-row search windows; the panelised
# general matrix at (96, 96); one and two candidates per lane; the first sizes beyond the two-candidate window)
ROUTE_R_DIMS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 80, 81, 95, 96)
ROUTE_L_DIMS = (1, 2, 63, 64, 65, 96)
ROUTE_L_SELECT = ((5, 5), (20, 7), (64, 64), (70, 33), (96, 1), (96, 65), (96, 96))
ROUTE_G_DIMS = (97, 127, 128, 129, 130, 168, 191, 192, 193, 257, 300)
ROUTE_G_SELECT = ((97, 1), (130, 64), (130, 65), (168, 129), (300, 300))
PIVOT_ROWS = (63, 64, 65, 127, 128, 129)          # and d - 1: rows in which the column-0 pivot of a shift matrix is put
NOISE = (1e-9, 0.05)
FAMILIES = ("generic", "gaussian", "shift", "shift_noise", "permutation", "singular")


def batch_size(D):
    return 5 if D > 96 else 9


def all_dims():
    """every matrix size d (= D for diagonal widths, d' for selections) a GPU case uses"""
    return sorted(set(ROUTE_R_DIMS) | set(ROUTE_L_DIMS) | set(ROUTE_G_DIMS)
                  | {dp for _, dp in ROUTE_L_SELECT + ROUTE_G_SELECT})


# ---------------------------------------------------------------------------------------------------------------- reference
def det_longdouble(A):
    """determinant of one square complex matrix: LU with full partial pivoting (largest modulus of the whole remaining
    column) in numpy.clongdouble, one rank-1 update per column"""
    A = np.array(A, dtype=CLD)
    d = A.shape[0]
    assert A.shape == (d, d)
    det = CLD(1.0)
    for k in range(d):
        col = A[k:, k]
        p = k + int(np.argmax(col.real * col.real + col.imag * col.imag))
        if p != k:
            A[[k, p]] = A[[p, k]]
            det = -det
        piv = A[k, k]
        det = det * piv
        if piv == 0:
            return CLD(0.0)
        if k + 1 < d:
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k] / piv, A[k, k + 1:])
    return det


def permutation_sign(perm):
    """+1 / -1: parity of a permutation given as an index array (d - number of cycles)"""
    perm = np.asarray(perm)
    seen, sign = np.zeros(len(perm), dtype=bool), 1
    for i in range(len(perm)):
        if not seen[i]:
            j, n = i, 0
            while not seen[j]:
                seen[j] = True
                j, n = int(perm[j]), n + 1
            if n % 2 == 0:
                sign = -sign
    return sign


def monomial_det(perm, factors):
    """analytic determinant of the matrix with A[i, perm[i]] = factors[i] and exact zeros elsewhere, in extended precision"""
    det = CLD(permutation_sign(perm))
    for f in np.asarray(factors, dtype=CLD):
        det = det * f
    return det


# ----------------------------------------------------------------------------------------------------------------- families
def _rng(family, d, extra=0):
    return np.random.default_rng([zlib.crc32(family.encode()), d, extra])


def pivot_rows(d):
    """rows d - s in which shift(s) puts the only entry of column 0"""
    return tuple(r for r in sorted(set(PIVOT_ROWS + (d - 1,))) if 1 <= r <= d - 1)


def _cgauss(rng, shape):
    """standard complex Gaussian: E|z|^2 = 1"""
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)


def generic(d, n):
    """complex Gaussian entries of variance 1/d plus 3 I, rows scaled to the 2-norm 1.05 (|det| stays near 1).  The Gaussian part
    has spectral radius about 1, so every Schur complement keeps diagonal entries of modulus 2 and more while no entry off the
    diagonal exceeds a few d^-1/2: the register elimination, which flags an in-block pivot 16 times smaller than an entry of
    its row in a later column block, has nothing to flag -- generic matrices must leave the flagged count at zero."""
    A = _cgauss(_rng("generic", d), (n, d, d)) / np.sqrt(d) + 3.0 * np.eye(d)
    return A * (1.05 / np.linalg.norm(A, axis=2, keepdims=True))


def gaussian(d, n):
    """complex Gaussian entries of variance 1 plus 3 I, rows scaled to the 2-norm 1.6: beyond d = 9 the diagonal no longer
    dominates, partial pivoting exchanges rows throughout, and the register elimination may or may not flag a trajectory"""
    A = _cgauss(_rng("gaussian", d), (n, d, d)) + 3.0 * np.eye(d)
    return A * (1.6 / np.linalg.norm(A, axis=2, keepdims=True))


def shift_parts(d, row, seed=0):
    """shift(s) with s = d - row: permutation i -> (i + s) mod d and the per-row factors (modulus 1 ... 2, random phase)"""
    rng = _rng("shift", d, 1000 * seed + row)
    fac = rng.uniform(1.0, 2.0, d) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, d))
    return (np.arange(d) + (d - row)) % d, fac


def shift(d, row, noise=0.0, seed=0):
    """np.roll(np.eye(d), s, axis=1) times the row factors: exact zeros elsewhere, or dense noise of amplitude `noise`"""
    perm, fac = shift_parts(d, row, seed)
    A = np.roll(np.eye(d), d - row, axis=1) * fac[:, None]
    assert np.count_nonzero(A) == d and A[row, 0] == fac[row]
    if noise:
        A = A + noise * _cgauss(_rng("noise", d, 1000 * seed + row), (d, d))
    return A


def permutation_parts(d, odd):
    """a random permutation of the requested parity and unit phases"""
    rng = _rng("permutation", d, int(odd))
    perm = rng.permutation(d)
    if d >= 2 and (permutation_sign(perm) < 0) != bool(odd):
        perm[[0, 1]] = perm[[1, 0]]
    return perm, np.exp(2j * np.pi * rng.uniform(0.0, 1.0, d))


def permutation(d, odd):
    perm, ph = permutation_parts(d, odd)
    A = np.zeros((d, d), dtype=np.complex128)
    A[np.arange(d), perm] = ph
    return A


def singular(d):
    """Gaussian matrices made singular: one with two equal rows (d >= 2), one with a zero column, one with a zero row"""
    base = gaussian(d, 3)
    out = []
    if d >= 2:
        a = base[0].copy()
        a[d - 1] = a[(d - 1) // 2]
        out.append(a)
    b = base[1].copy()
    b[:, d // 2] = 0.0
    out.append(b)
    c = base[2].copy()
    c[d // 3] = 0.0
    out.append(c)
    return np.stack(out)


def _fill(mats, refs, n):
    """pad a family's matrices to whole batches of n by cycling through them"""
    m = len(mats)
    total = -(-m // n) * n
    idx = [i % m for i in range(total)]
    return np.stack([mats[i] for i in idx]), (None if refs is None else np.array([refs[i] for i in idx], dtype=CLD))


@functools.lru_cache(maxsize=None)
def family_cases(family, d, n):
    """-> (A [m, d, d] complex128 with m a multiple of n, ref [m] clongdouble or None for `singular`).  The reference is computed
    once per (family, d) and shared by every test that needs it; treat both arrays as read-only."""
    if family in ("generic", "gaussian"):
        A = generic(d, n) if family == "generic" else gaussian(d, n)
        ref = np.array([det_longdouble(a) for a in A], dtype=CLD)
    elif family == "shift":                                     # exact zeros: the determinant is known analytically
        rows = pivot_rows(d)
        if not rows:
            return None
        A, ref = _fill([shift(d, r) for r in rows], [monomial_det(*shift_parts(d, r)) for r in rows], n)
    elif family == "shift_noise":
        rows = pivot_rows(d)
        if not rows:
            return None
        mats = [shift(d, r, noise=amp) for r in rows for amp in NOISE]
        A, ref = _fill(mats, [det_longdouble(a) for a in mats], n)
    elif family == "permutation":
        if d < 2:
            return None
        A, ref = _fill([permutation(d, odd) for odd in (0, 1)], [monomial_det(*permutation_parts(d, odd)) for odd in (0, 1)], n)
    elif family == "singular":
        A, ref = _fill(list(singular(d)), None, n)
    else:
        raise KeyError(family)
    A.setflags(write=False)
    if ref is not None:
        ref.setflags(write=False)
    return A, ref


def rel_err(got, ref):
    """|got - ref| / |ref| per matrix, evaluated in extended precision"""
    ref = np.asarray(ref, dtype=CLD)
    return np.asarray(np.abs(np.asarray(got).astype(CLD) - ref) / np.abs(ref), dtype=np.float64)


def err64(A, ref):
    """error of numpy.linalg.det (LAPACK, fp64) against the extended-precision reference, per matrix"""
    return rel_err(np.linalg.det(np.asarray(A)), ref)


def accuracy_bound(A, ref):
    """16 x LAPACK's own error (the pivot slack of the fixed-order / block-pivoted eliminations) plus a floor
    of a few ulps per elimination step"""
    d = A.shape[-1]
    return 16.0 * err64(A, ref) + 4.0 * d * 2.0 ** -52


# ---------------------------------------------------------------------------------------------------------------- encodings
def width_scales(D, variant):
    """st, si [D]: ones ("plain") or positive powers of two that differ per index and between st and si ("scaled")"""
    if variant == "plain":
        return np.ones(D), np.ones(D)
    rng = _rng("widths", D)
    return 2.0 ** rng.integers(-3, 4, D), 2.0 ** rng.integers(-3, 4, D)


def blocks_for(A, variant="plain"):
    """monodromy blocks [..., 4, D, D] = Mqq, Mqp, Mpq, Mpp whose prefactor matrix for the diagonal widths of
    width_scales(D, variant) is A exactly (hbar = 1).  "plain": Mqq = 2 Re A, Mpq = 2 Im A, the others zero.  "scaled": all four
    blocks carry half of A each, divided by their own (power-of-two) width factor, so a swapped st / si or row / column index
    does not give A back."""
    A = np.asarray(A, dtype=np.complex128)
    D = A.shape[-1]
    st, si = width_scales(D, variant)
    if variant == "plain":
        zero = np.zeros_like(A.real)
        return np.stack((2.0 * A.real, zero, 2.0 * A.imag, zero), axis=-3)
    ratio, prod = st[:, None] / si[None, :], st[:, None] * si[None, :]
    return np.stack((A.real / ratio, -A.imag / prod, A.imag * prod, A.real * ratio), axis=-3)


def selection(D, dp):
    """0/1 selection matrices L [d', D], R [D, d'] (complex, zero imaginary parts) that pick d' rows and d' other columns of a
    D x D matrix, in an order that is not the leading one"""
    rng = _rng("selection", D, dp)
    rows, cols = rng.permutation(D)[:dp], rng.permutation(D)[:dp]
    if D > 1:
        assert not np.array_equal(rows, cols) and not np.array_equal(rows, np.arange(dp))
    L, R = np.zeros((dp, D), dtype=np.complex128), np.zeros((D, dp), dtype=np.complex128)
    L[np.arange(dp), rows] = 1.0
    R[cols, np.arange(dp)] = 1.0
    return rows, cols, L, R


def embed(A, D):
    """D x D matrices whose submatrix picked by selection(D, d') is A [n, d', d']; Gaussian entries everywhere else"""
    A = np.asarray(A, dtype=np.complex128)
    n, dp = A.shape[0], A.shape[-1]
    rows, cols, _, _ = selection(D, dp)
    big = _cgauss(_rng("embed", D, dp), (n, D, D))
    big[:, rows[:, None], cols[None, :]] = A
    return big


def prefactor_diag_numpy(M, st, si):
    """the kernels' prefactor expression for diagonal widths (dense_prefactor_kernel, prefactor_any_kernel), hbar = 1"""
    a, b = st[:, None], si[None, :]
    return 0.5 * (a / b * M[..., 0, :, :] + b / a * M[..., 3, :, :]) + 0.5j * (-1.0 * a * b * M[..., 1, :, :] + M[..., 2, :, :] / (1.0 * a * b))


def prefactor_general_numpy(M, L1, L2, R1, R2):
    """mat = 1/2 [L1 (Mqq R1 - i hbar Mqp R2) + L2 (Mpp R2 + i/hbar Mpq R1)], hbar = 1 (general_prefactor_matrix_t)"""
    X1 = M[..., 0, :, :] @ R1 - 1j * (M[..., 1, :, :] @ R2)
    X2 = M[..., 3, :, :] @ R2 + 1j * (M[..., 2, :, :] @ R1)
    return 0.5 * (L1 @ X1 + L2 @ X2)


# ------------------------------------------------------------------------------------------------------------------- driver
def run_blocks(route, mono, st=None, si=None, L=None, R=None):
    """sc_dense_mono_step(dt = 0, mode = 1) on monodromy blocks mono [n, 4, D, D] (numpy) with diagonal widths st, si [D] or
    dense widths L1 = L2 = L [d', D], R1 = R2 = R [D, d'] (complex); sc_state / sc_hk_consts are built by ctypes.  Returns
    (c2 [n] complex128, sgn [n], flagged): `flagged` is the count the register kernel left in flags[n] (route R; None on
    the other routes), flags[:n] is asserted to be cleared.  The route is the library's choice: the arguments have to match."""
    import torch
    from semiclassical_amd._lib import lib, check, ptr, sc_state, sc_hk_consts
    dev = torch.device("cuda")
    n, D = mono.shape[0], mono.shape[-1]
    diag = L is None
    dp = D if diag else L.shape[0]
    assert mono.shape == (n, 4, D, D) and mono.dtype == np.float64
    assert route in ("R", "L", "G") and (D > 96) == (route == "G") and (route != "R" or diag)
    keep = []

    def up(x):
        keep.append(torch.from_numpy(np.ascontiguousarray(x)).to(dev))
        return keep[-1]
    mono_d = up(mono)
    if diag:
        assert st.shape == (D,) and si.shape == (D,) and st.dtype == np.float64 and si.dtype == np.float64
        hk = sc_hk_consts(dim=D, dprime=D, diag=1, st=ptr(up(st)), si=ptr(up(si)))
    else:
        assert L.shape == (dp, D) and R.shape == (D, dp) and L.dtype == np.complex128 and R.dtype == np.complex128
        Ld, Rd = up(L), up(R)
        hk = sc_hk_consts(dim=D, dprime=dp, diag=0, real_lr=1, L1=ptr(Ld), L2=ptr(Ld), R1=ptr(Rd), R2=ptr(Rd))
    c2 = torch.full((n,), float("nan"), dtype=torch.complex128, device=dev)        # the kernels have to write both
    sgn = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    qp, act = torch.zeros((n, 2 * D), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    flags = torch.zeros(n + 2, dtype=torch.int32, device=dev) if route == "R" else None
    need = lib.sc_dense_mono_scratch_bytes(n, D, dp)
    assert need >= 0 and (need > 0) == (D > 64)
    scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev) if route == "G" else None
    state = sc_state(n=n, dim=D, mono_layout=0, qp=ptr(qp), act=ptr(act), mono=ptr(mono_d), c2=ptr(c2), sgn=ptr(sgn),
                     flags=ptr(flags))
    check(lib.sc_dense_mono_step(state, hk, None, None, ptr(scratch), 0.0, 1, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    flagged = None
    if flags is not None:
        f = flags.cpu().numpy()
        assert not f[:n].any(), "the fix-up pass has to clear the flags it served"
        flagged = int(f[n])
    return c2.cpu().numpy(), sgn.cpu().numpy(), flagged


def run_route(route, A_batch, variant="plain", select_D=None):
    """Hand the matrices A_batch [n, d, d] to the named determinant route through their exact encoding: diagonal widths
    (`variant` of width_scales), or with `select_D` as the d' x d' selection out of D x D blocks under dense widths."""
    A_batch = np.asarray(A_batch, dtype=np.complex128)
    d = A_batch.shape[-1]
    if select_D is None:
        st, si = width_scales(d, variant)
        return run_blocks(route, blocks_for(A_batch, variant), st=st, si=si)
    _, _, L, R = selection(select_D, d)
    return run_blocks(route, blocks_for(embed(A_batch, select_D), "plain"), L=L, R=R)
