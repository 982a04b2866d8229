"""One Arnoldi extension step and the Arnoldi relation in ``np.longdouble``, with first-order error bounds for a float64 device.

``step`` is what ``lz_trl_extend`` does for one ``j`` - ``w = A V[j]``, classical Gram-Schmidt against the rows behind the DGKS gate,
``beta = |r|``, ``v = r / beta`` - and carries an absolute error bound for every returned quantity through the same operations.  The
bounds are derived, not tuned (``eps`` is float64's machine epsilon, twice the unit roundoff, so every term has a factor two in hand):

- a product row of ``nnz_row`` terms, in any order, fused or not, errs by at most ``nnz_row eps (|A||x|)_row`` (dense: ``n`` terms);
- a dot product of ``n_pad`` terms (the device streams the zero padding too) errs by at most ``n_pad eps sum|a||b|`` in any order, and
  inherits ``|row| . e_w`` from the error of ``w``;
- ``r = w - sum_i c_i row_i`` is ``nb`` subtractions of a rounded product per element: ``(nb + 2) eps (|w| + sum_i |c_i||row_i|)`` on top of
  ``e_w`` and of ``e_c[i] |row_i|``;
- the same again through the second pass, from ``r`` and ``e_r``;
- ``beta`` is the root of a sum of ``n_pad`` squares of a vector known to ``e_r``; ``v`` is a quotient of the two.

``relation`` measures ``A V_m^T = V_{m+1}^T H`` and the orthonormality of ``V_{m+1}`` in longdouble.

A plain module: no fixtures, nothing collected from it.
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
PAD = 32  # vectors on the device are padded to multiples of this many doubles (lz_padded_rows)


def padded(n):
    return -(-int(n) // PAD) * PAD


def matvec(A, x):
    """``A x`` in longdouble (``A``: SciPy sparse or a dense array of float64, ``x``: any float vector)"""
    x = np.asarray(x, dtype=LD)
    if not sp.issparse(A):
        return np.asarray(A, dtype=LD) @ x
    A = sp.csr_matrix(A)
    y = np.zeros(A.shape[0], dtype=LD)
    if A.nnz:
        prod = A.data.astype(LD) * x[A.indices]
        full = np.diff(A.indptr) > 0
        y[full] = np.add.reduceat(prod, A.indptr[:-1][full])
    return y


def _abs_matvec(A, x):
    """``|A||x|`` and the number of terms of a product row"""
    if sp.issparse(A):
        A = sp.csr_matrix(A)
        return np.asarray(abs(A) @ np.abs(x), dtype=LD), max(int(np.diff(A.indptr).max()), 1)
    return np.asarray(np.abs(A) @ np.abs(x), dtype=LD), A.shape[1]


def _pass(rows, w, e_w, n_pad):
    """one classical Gram-Schmidt pass: ``(c, r, e_c, e_r)``"""
    nb = len(rows)
    arows = np.abs(rows)
    c = rows @ w
    e_c = n_pad * EPS * (arows @ np.abs(w)) + arows @ e_w
    r = w - c @ rows
    e_r = e_w + e_c @ arows + (nb + 2) * EPS * (np.abs(w) + np.abs(c) @ arows)
    return c, r, e_c, e_r


def step(A, rows, force):
    """One extension step: ``w = A rows[nb - 1]``, Gram-Schmidt against all ``nb`` rows, the second pass where ``force`` or the first
    left less than half of ``|w|^2``.  Returns a dict of float64 values - ``c1``, ``c2`` (zeros where the second pass did not run),
    ``ratio``, ``beta``, ``v``, ``w_norm``, ``pass2`` - and the bounds ``e_proj`` (on ``c1 + c2``), ``e_beta`` and ``e_v`` (per element)."""
    rows = np.asarray(rows, dtype=LD)
    nb, n = rows.shape
    n_pad = padded(n)
    w = matvec(A, rows[nb - 1])
    aw, terms = _abs_matvec(A, np.asarray(rows[nb - 1], dtype=np.float64))
    e_w = terms * EPS * aw
    c1, r, e_c1, e_r = _pass(rows, w, e_w, n_pad)
    ratio = float(np.dot(r, r) / np.dot(w, w))
    pass2 = bool(force or ratio < 0.5)
    c2, e_c2 = np.zeros(nb, dtype=LD), np.zeros(nb, dtype=LD)
    if pass2:
        c2, r, e_c2, e_r = _pass(rows, r, e_r, n_pad)
    beta = np.sqrt(np.dot(r, r))
    e_beta = np.sqrt(np.dot(e_r, e_r)) + n_pad * EPS * beta
    v = r / beta
    e_v = (e_r + np.abs(r) * (e_beta / beta + 2 * EPS)) / beta
    f = np.float64
    return {"c1": c1.astype(f), "c2": c2.astype(f), "ratio": ratio, "beta": float(beta), "v": v.astype(f), "pass2": pass2,
            "w_norm": float(np.sqrt(np.dot(w, w))), "e_proj": (e_c1 + e_c2).astype(f), "e_beta": float(e_beta), "e_v": e_v.astype(f)}


def worst(err, bound):
    """``max(err / bound)`` with ``0 / 0 = 0`` (a position where every input is zero has a zero bound, and must be met exactly)"""
    err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    q = np.where(err == 0.0, 0.0, err / np.where(bound > 0.0, bound, 1.0))
    return float(np.max(np.where((bound > 0.0) | (err == 0.0), q, np.inf)))


def relation(A, V, H):
    """``H`` is ``(m + 1, m)`` and ``V`` has at least ``m + 1`` rows of length ``n``: returns the ``m`` column norms of
    ``A V[:m]^T - V[:m + 1]^T H`` and ``max|V[:m + 1] V[:m + 1]^T - I|``, both formed in longdouble"""
    H = np.asarray(H, dtype=LD)
    m = H.shape[1]
    V = np.asarray(V, dtype=LD)[: m + 1]
    D = np.stack([matvec(A, V[j]) for j in range(m)]) - H.T @ V  # row j: (A v_j - V^T H[:, j])^T
    defect = np.sqrt(np.sum(D * D, axis=1)).astype(np.float64)
    G = V @ V.T - np.eye(m + 1, dtype=LD)
    return defect, float(np.abs(G).max())
