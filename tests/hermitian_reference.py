"""One extension step of the complex thick-restart solver and the Lanczos relation in ``np.clongdouble``, with first-order error bounds
for a float64 device: ``arnoldi_reference.py`` for a complex Hermitian matrix and ``<x, y> = sum conj(x) y``.

``step`` is what ``lz_ztrl_extend`` does for one ``j`` - ``w = A V[j]``, classical Gram-Schmidt against the rows behind the DGKS gate,
``beta = |r|``, ``v = r / beta`` - and carries an absolute bound on the modulus of the error of every returned quantity through the same
operations.  The bounds are derived as ``arnoldi_reference``'s are (``eps`` is float64's machine epsilon, twice the unit roundoff, so
every term has a factor two in hand), with two changes:

- a complex dot product of ``n`` terms counts as ``2 n`` real terms: each part of ``sum a_k b_k`` is a sum of ``2 n`` real products, whose
  moduli add up to at most ``sum |a_k||b_k|`` (Cauchy-Schwarz on ``|Re a||Re b| + |Im a||Im b|``);
- moduli take the place of absolute values.

So a product row of ``r`` entries errs by at most ``2 r eps (|A||x|)_row``, a Gram-Schmidt coefficient by ``2 n_pad eps sum|row||w|`` plus
what it inherits, and the update ``w - sum_i c_i row_i`` by ``(2 nb + 2) eps (|w| + sum_i |c_i||row_i|)`` per element on top of that.

``product_bound`` is the bar of the product kernels alone, in the form tests/test_gpu_eigs.py uses with the factor for the complex
multiplication: ``4 (r_i + 2) eps (|A||x|)_i``.

A plain module: no fixtures, nothing collected from it.
"""
import numpy as np
import scipy.sparse as sp
from arnoldi_reference import EPS, padded, worst  # noqa: F401  (worst: re-exported for the tests)

CLD = np.clongdouble
LD = np.longdouble


def matvec(A, x):
    """``A x`` in clongdouble (``A``: SciPy sparse or a dense array, complex128; ``x``: any vector)"""
    x = np.asarray(x, dtype=CLD)
    if not sp.issparse(A):
        return np.asarray(A, dtype=CLD) @ x
    A = sp.csr_matrix(A)
    y = np.zeros(A.shape[0], dtype=CLD)
    if A.nnz:
        prod = A.data.astype(CLD) * x[A.indices]
        full = np.diff(A.indptr) > 0
        y[full] = np.add.reduceat(prod, A.indptr[:-1][full])
    return y


def abs_matvec(A, x):
    """``|A||x|`` (longdouble) and the entry count of every product row"""
    ax = np.abs(np.asarray(x, dtype=np.complex128))
    if sp.issparse(A):
        A = sp.csr_matrix(A)
        # |A| entry by entry as stored.  (SciPy's ``abs(A)`` sums duplicate entries first - IN PLACE, in the arrays that
        # ``sp.csr_matrix(A)`` shares with the caller's matrix; for a canonical matrix the two are the same numbers.)
        stored = sp.csr_matrix((np.abs(A.data), A.indices, A.indptr), shape=A.shape)
        return np.asarray(stored @ ax, dtype=LD), np.diff(A.indptr)
    return np.asarray(np.abs(A) @ ax, dtype=LD), np.full(A.shape[0], A.shape[1])


def product_bound(A, x):
    """per row: ``4 (r_i + 2) eps (|A||x|)_i``"""
    aw, terms = abs_matvec(A, x)
    return (4.0 * (terms + 2) * EPS * aw).astype(np.float64)


def _pass(rows, w, e_w, n_pad):
    """one classical Gram-Schmidt pass: ``(c, r, e_c, e_r)``"""
    nb = len(rows)
    arows = np.abs(rows)
    c = rows.conj() @ w
    e_c = 2 * n_pad * EPS * (arows @ np.abs(w)) + arows @ e_w
    r = w - c @ rows
    e_r = e_w + e_c @ arows + (2 * nb + 2) * EPS * (np.abs(w) + np.abs(c) @ arows)
    return c, r, e_c, e_r


def _norm2(x):
    return np.sum(x.real * x.real + x.imag * x.imag)


def step(A, rows, force):
    """One extension step: ``w = A rows[nb - 1]``, Gram-Schmidt against all ``nb`` rows, the second pass where ``force`` or the first
    left less than half of ``|w|^2``.  Returns a dict - ``c1``, ``c2`` (complex128; zeros where the second pass did not run), ``ratio``,
    ``beta``, ``v`` (complex128), ``w_norm``, ``pass2`` - and the bounds ``e_proj`` (on ``|c1 + c2 - c|``), ``e_beta`` and ``e_v`` (per
    element, on the modulus)."""
    rows = np.asarray(rows, dtype=CLD)
    nb, n = rows.shape
    n_pad = padded(n)
    w = matvec(A, rows[nb - 1])
    aw, terms = abs_matvec(A, rows[nb - 1])
    e_w = 2 * np.maximum(terms, 1) * EPS * aw
    c1, r, e_c1, e_r = _pass(rows, w, e_w, n_pad)
    ratio = float(_norm2(r) / _norm2(w))
    pass2 = bool(force or ratio < 0.5)
    c2, e_c2 = np.zeros(nb, dtype=CLD), np.zeros(nb, dtype=LD)
    if pass2:
        c2, r, e_c2, e_r = _pass(rows, r, e_r, n_pad)
    beta = np.sqrt(_norm2(r))
    e_beta = np.sqrt(np.dot(e_r, e_r)) + 2 * n_pad * EPS * beta
    v = r / beta
    e_v = (e_r + np.abs(r) * (e_beta / beta + 2 * EPS)) / beta
    f, c = np.float64, np.complex128
    return {"c1": c1.astype(c), "c2": c2.astype(c), "ratio": ratio, "beta": float(beta), "v": v.astype(c), "pass2": pass2,
            "w_norm": float(np.sqrt(_norm2(w))), "e_proj": (e_c1 + e_c2).astype(f), "e_beta": float(e_beta), "e_v": e_v.astype(f)}


def relation(A, V, H):
    """``H`` is ``(m + 1, m)`` complex and ``V`` has at least ``m + 1`` rows of length ``n``: returns the ``m`` column norms of
    ``A V[:m]^T - V[:m + 1]^T H`` and ``max|conj(V[:m + 1]) V[:m + 1]^T - I|``, both formed in clongdouble"""
    H = np.asarray(H, dtype=CLD)
    m = H.shape[1]
    V = np.asarray(V, dtype=CLD)[: m + 1]
    D = np.stack([matvec(A, V[j]) for j in range(m)]) - H.T @ V  # row j: (A v_j - V^T H[:, j])^T
    defect = np.sqrt(np.sum(D.real * D.real + D.imag * D.imag, axis=1)).astype(np.float64)
    G = V.conj() @ V.T - np.eye(m + 1, dtype=CLD)
    return defect, float(np.abs(G).max())
