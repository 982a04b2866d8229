"""``svds``: singular triplets of a rectangular or non-symmetric sparse matrix by thick-restart Golub-Kahan-Lanczos on the GPU.

The two bases - ``V`` (``ncv + 1`` rows of the short length ``q = min(M, N)``) and ``U`` (``ncv`` rows of the long length ``p``) - and
every product and pass over them live on the device (``lz_gk_*`` in include/lanczos_hip.h); the host keeps only the ``ncv x ncv``
projected matrix ``B`` and runs the outer loop below (``gkl``), as ``eigsh.trl`` does for the symmetric problem.  Nothing forms
``A^T A``: the condition number is not squared.

Golub-Kahan-Lanczos with thick restart (Baglama & Reichel 2005; SLEPc's TRLANCZOS).  Step ``j``: ``w = A V[j]`` orthogonalised against
``U[0..j)``, ``alpha_j = |w|``, ``U[j] = w / alpha_j``; ``z = A^T U[j]`` orthogonalised against ``V[0..j]``, ``beta_j = |z|``,
``V[j+1] = z / beta_j``.  ``B`` is upper triangular: column ``j`` above the diagonal holds the *measured* coefficients of the first
half step, ``B[j, j] = alpha_j``, so ``A V_m = U_m B`` holds by construction and ``A^T U_m = V_m B^T + beta_{m-1} V[m] e_m^T``.  A
cycle takes ``B = P S Q^T``, estimates the residual of triplet ``i`` as ``beta_{m-1} |P[m-1, i]|``, keeps ``kk`` triplets
(``U[0..kk) = P^T U``, ``V[0..kk) = Q^T V``, ``V[kk] = V[m]``) and goes on from ``B = diag(sigma_keep)``; the arrow column ``kk``
reappears as the measured coefficients of the next step.

Stopping rule.  A wanted triplet is converged when ``beta_{m-1} |P[m-1, i]| <= tol_eff * max sigma seen`` (``tol_eff = tol``, or
machine epsilon for ``tol == 0``): the scale ``eigsh`` uses, for the reason in its module docstring.

Breakdown.  The device runs an extension without a synchronisation, so a vanished ``alpha_j`` or ``beta_j`` is found afterwards:
everything behind the first bad half step is discarded and redone.  The bound is ``10 eps scale`` times the rows the half step
subtracted (``trl_band``'s).  A vanished ``beta_j`` (``j < m - 1``): ``V[j+1]`` becomes a random direction orthogonal to the rows
before it, with coupling 0.  A vanished ``alpha_j``: ``B[j, j] = 0`` and ``U[j]`` becomes such a direction; the extension resumes at
the second half of step ``j``.  A vanished ``beta_{m-1}``: the short space is exhausted (``ncv = min(M, N)``), the residual estimates
are zero and ``V[m]`` is not used after the restart.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse
from scipy.sparse.linalg import ArpackNoConvergence

from .eigsh import _EPS, _MAX_NCV, _SEED

_SIDES = {"u": 0, "v": 1}


class NumpyGKBackend:
    """The calls of the device backend (``lz_gk_*``) in NumPy: what the host tests drive ``gkl`` with.  ``A`` is ``p x q``, ``p >= q``."""

    def __init__(self, A, force_second_pass=False):
        self.A = A
        self.AT = A.T.tocsr() if scipy.sparse.issparse(A) else A.T
        self.p, self.q = A.shape
        self.force = force_second_pass
        self.u_ready = None

    def begin(self, m, v0):
        self.V = np.zeros((m + 1, self.q))
        self.U = np.zeros((m + 1, self.p))  # (row m stays zero, as on the device)
        self.V[0] = v0 / np.linalg.norm(v0)
        self.u_ready = None

    def _half(self, Bs, w, nb):
        """w against Bs[0..nb): CGS with the DGKS gate |w|^2 < 1/2 |w0|^2 -> (w, both passes' coefficients, |w|)"""
        c = np.zeros(nb)
        if nb > 0:
            w0 = np.dot(w, w)
            c = Bs[:nb] @ w
            w = w - c @ Bs[:nb]
            if self.force or np.dot(w, w) < 0.5 * w0:
                c2 = Bs[:nb] @ w
                w = w - c2 @ Bs[:nb]
                c = c + c2
        return w, c, np.linalg.norm(w)

    def extend(self, k, m):
        colproj = np.zeros((m, m))
        alpha = np.zeros(m)
        beta = np.zeros(m)
        with np.errstate(divide="ignore", invalid="ignore"):
            for j in range(k, m):
                if self.u_ready != j:  # (a probed U[j]: the step resumes at its second half)
                    w, c, alpha[j] = self._half(self.U, self.A @ self.V[j], j)
                    colproj[j, :j] = c
                    self.U[j] = w / alpha[j]
                self.u_ready = None
                z, _, beta[j] = self._half(self.V, self.AT @ self.U[j], j + 1)
                self.V[j + 1] = z / beta[j]
        return colproj, alpha, beta

    def restart(self, m, kk, P, Q):
        self.U[:kk] = P.T @ self.U[:m]
        self.U[kk] = self.U[m]
        self.V[:kk] = Q.T @ self.V[:m]
        self.V[kk] = self.V[m].copy()
        self.u_ready = None

    def probe(self, side, k, x):
        Bs = self.U if side == "u" else self.V
        for _ in range(2):
            x = x - (Bs[:k] @ x) @ Bs[:k]
        Bs[k] = x / np.linalg.norm(x)
        if side == "u":
            self.u_ready = k

    def get_vectors(self, side, k):
        return (self.U if side == "u" else self.V)[:k].T.copy()

    def residuals(self, k, sigma):
        return np.array([[np.linalg.norm(self.A @ self.V[i] - sigma[i] * self.U[i]) for i in range(k)],
                         [np.linalg.norm(self.AT @ self.U[i] - sigma[i] * self.V[i]) for i in range(k)]])


class DeviceGKBackend:
    """The ``lz_gk_*`` calls on one ``_capi.Handle`` that already holds the rectangular matrix (``gk_set_csr`` or ``gk_set_dense``)."""

    def __init__(self, handle, force_second_pass=False):
        self.h = handle
        if force_second_pass:
            from ._capi import FLAG_TRL_PASS2_ALWAYS

            handle.set_options(FLAG_TRL_PASS2_ALWAYS)

    def begin(self, m, v0):
        self.h.gk_begin(m, v0)

    def extend(self, k, m):
        return self.h.gk_extend(k, m)

    def restart(self, m, kk, P, Q):
        self.h.gk_restart(m, kk, P, Q)

    def probe(self, side, k, x):
        self.h.gk_probe(_SIDES[side], k, x)

    def get_vectors(self, side, k):
        return self.h.gk_get_vectors(_SIDES[side], k)

    def residuals(self, k, sigma):
        return self.h.gk_residuals(k, sigma)


def check_args(shape, k, which, ncv):
    """The argument errors of ``svds`` that depend on the shape.  Returns ncv."""
    q = min(shape)
    if len(shape) != 2 or q < 2:
        raise ValueError(f"expected a matrix with min(M, N) >= 2 (shape={tuple(shape)})")
    if which not in ("LM", "SM"):
        raise ValueError("which must be either 'LM' or 'SM'")
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= q - 1:
        raise ValueError(f"k must be an integer with 1 <= k <= min(M, N) - 1 = {q - 1}, k={k!r}")
    if ncv is None:
        ncv = min(q, max(2 * int(k) + 1, 20))
    ncv = int(ncv)
    if not k + 2 <= ncv <= min(q, _MAX_NCV):
        raise ValueError(f"ncv must be k+2<=ncv<=min(min(M, N), {_MAX_NCV}), ncv={ncv} (the thick restart keeps two spare basis rows)")
    return ncv


def gkl(backend, shape, k, which="LM", ncv=None, maxiter=None, tol=0.0, v0=None, rng=None):
    """The thick-restart Golub-Kahan-Lanczos outer loop over a backend (``NumpyGKBackend`` or ``DeviceGKBackend``) that holds a
    ``p x q`` matrix, ``shape = (p, q)``, ``p >= q``.

    Returns ``(s, info)``: the ``k`` wanted singular values in ascending order (rows ``0..k`` of the backend's ``U`` and ``V`` then hold
    their vectors) and ``{"matvecs", "cycles", "breakdowns", "anorm"}``.  Raises ``ArpackNoConvergence`` after ``maxiter`` cycles; its
    ``.eigenvectors`` are the converged rows of ``V`` (``(q, nconv)``)."""
    p, q = shape
    m = check_args(shape, k, which, ncv)
    k = int(k)
    maxiter = 10 * q if maxiter is None else int(maxiter)
    rng = np.random.default_rng(_SEED) if rng is None else rng
    tol_eff = float(tol) if tol > 0 else _EPS
    v0 = rng.uniform(-1.0, 1.0, q) if v0 is None else np.asarray(v0, dtype=np.float64).reshape(-1)
    if v0.shape != (q,) or not np.linalg.norm(v0) > 0:
        raise ValueError("v0 must be a non-zero vector of length min(M, N)")
    backend.begin(m, v0)
    B = np.zeros((m, m))
    kcur, anorm = 0, 0.0
    info = {"matvecs": 0, "cycles": 0, "breakdowns": 0}
    while True:
        j0, resume = kcur, False  # resume: step j0 starts at its second half (U[j0] is a probed direction)
        while True:  # one extension of both bases; a breakdown replaces one row and goes on behind it
            colproj, alpha, beta = backend.extend(j0, m)
            info["matvecs"] += 2 * (m - j0) - (1 if resume else 0)
            # the first vanished norm: a row behind it is made from a normalised rounding error, so neither it nor any later half step of
            # this extension may enter B or the scale (those hold anything, NaN included)
            scale = max(anorm, np.abs(B[:, :j0]).max()) if j0 else anorm
            bad = None
            for j in range(j0, m):
                if not (resume and j == j0):
                    B[:j, j] = colproj[j, :j]
                    scale = max(scale, np.abs(colproj[j, :j]).max()) if j else scale
                    if not alpha[j] > 10 * _EPS * scale * max(j, 1):
                        bad = ("u", j)
                        break
                    B[j, j] = alpha[j]
                    scale = max(scale, alpha[j])
                if not beta[j] > 10 * _EPS * scale * (j + 1):
                    bad = ("v", j)
                    break
                scale = max(scale, beta[j])
            if bad is None or bad == ("v", m - 1):
                break
            info["breakdowns"] += 1
            side, jb = bad
            if side == "u":
                B[jb, jb] = 0.0
                backend.probe("u", jb, rng.standard_normal(p))
                j0, resume = jb, True
            else:
                backend.probe("v", jb + 1, rng.standard_normal(q))
                j0, resume = jb + 1, False
        info["cycles"] += 1
        dead = bad is not None  # beta_{m-1} vanished: the short space is exhausted, V[m] is noise
        b_last = 0.0 if dead else beta[m - 1]
        P, s, Qt = np.linalg.svd(B)
        anorm = max(anorm, s[0])
        res = b_last * np.abs(P[m - 1])
        order = np.arange(m) if which == "LM" else np.arange(m)[::-1]  # most wanted first (s is descending)
        want = order[:k]
        ok = res <= tol_eff * anorm
        if ok[want].all():
            sel = want[np.argsort(s[want], kind="stable")]
            backend.restart(m, k, np.ascontiguousarray(P[:, sel]), np.ascontiguousarray(Qt[sel].T))
            info["anorm"] = anorm
            return s[sel], info
        if info["cycles"] >= maxiter:
            conv = sorted((i for i in want if ok[i]), key=lambda i: s[i])
            vecs = np.zeros((q, 0))
            if conv:
                backend.restart(m, len(conv), np.ascontiguousarray(P[:, conv]), np.ascontiguousarray(Qt[conv].T))
                vecs = backend.get_vectors("v", len(conv))
            err = ArpackNoConvergence(f"No convergence ({info['cycles']} iterations, {len(conv)}/{k} singular triplets converged)", s[conv], vecs)
            info["anorm"] = anorm
            err.info = info
            err.nconv = len(conv)
            raise err
        nconv = int(ok[want].sum())
        kk = min(m - 2, k + max(nconv, (m - k) // 2))
        keep = order[:kk]
        backend.restart(m, kk, np.ascontiguousarray(P[:, keep]), np.ascontiguousarray(Qt[keep].T))
        B = np.zeros((m, m))
        B[np.arange(kk), np.arange(kk)] = s[keep]
        if dead:
            backend.probe("v", kk, rng.standard_normal(q))
        kcur = kk


def _pack(A):
    """``A`` (SciPy sparse of any format or a dense ndarray, real) -> ``(Aop, AopT, transposed)``, ``Aop`` the tall orientation
    (``p x q``, ``p >= q``).  Sparse input, and a dense array with ``12 nnz < 8 size`` (its CSR stream is the smaller one): float64 CSR
    with sorted indices and summed duplicates.  Any other dense array stays dense: ``Aop`` is a float64 *view* of the tall orientation
    and ``AopT = Aop.T``, so one of the two is C-contiguous.  A C- or F-contiguous float64 array is not copied (an F-contiguous
    ``M x N`` array is the C-contiguous ``N x M`` transpose); any other layout or dtype takes one ``np.ascontiguousarray``."""
    dense = not scipy.sparse.issparse(A)
    if dense:
        A = np.asarray(A)
        if A.ndim != 2:
            raise ValueError(f"expected a matrix (shape={A.shape})")
    if np.iscomplexobj(A):
        raise NotImplementedError("svds on the device is implemented for real matrices only")
    if A.dtype == np.float32:
        from ._solver import LanczosBase

        if LanczosBase.verbose:
            print("+++ svds: float32 input is converted to float64 (the device kernels are FP64).")
    if dense and not 12 * np.count_nonzero(A) < 8 * A.size:
        if max(A.shape) >= 2**31:
            raise ValueError("matrix too large for int32 indices")
        if A.dtype != np.float64 or not (A.flags.c_contiguous or A.flags.f_contiguous):
            A = np.ascontiguousarray(A, dtype=np.float64)
        transposed = A.shape[0] < A.shape[1]
        Aop = A.T if transposed else A
        return Aop, Aop.T, transposed
    A = scipy.sparse.csr_matrix(A, dtype=np.float64)
    if A.nnz >= 2**31 or max(A.shape) >= 2**31:
        raise ValueError("matrix too large for int32 CSR indices")
    transposed = A.shape[0] < A.shape[1]
    Aop = (A.T if transposed else A).tocsr().copy()
    Aop.sum_duplicates()
    Aop.sort_indices()
    AopT = Aop.T.tocsr()
    AopT.sort_indices()
    return Aop, AopT, transposed


def _svds(make_backend, A, k, ncv, tol, which, v0, maxiter, return_singular_vectors, solver, rng, random_state, options, info):
    """``svds`` over ``make_backend(Aop, AopT)``: everything but the choice of the backend (the host tests pass ``NumpyGKBackend``)"""
    if solver != "arpack":
        raise NotImplementedError(f"solver={solver!r}: only solver='arpack' (the Lanczos method) is implemented")
    if options is not None:
        raise NotImplementedError("options must be None")
    if not any(return_singular_vectors is f for f in (True, False)) and return_singular_vectors not in ("u", "vh"):
        raise ValueError("return_singular_vectors must be True, False, 'u' or 'vh'")
    shape = tuple(A.shape)
    if np.iscomplexobj(A):
        raise NotImplementedError("svds on the device is implemented for real matrices only")
    m = check_args(shape, k, which, ncv)
    seed = rng if rng is not None else random_state
    gen = np.random.default_rng(_SEED if seed is None else seed)
    Aop, AopT, transposed = _pack(A)
    backend = make_backend(Aop, AopT)
    left_side = "v" if transposed else "u"  # which basis holds A's left singular vectors (length M)
    right_side = "u" if transposed else "v"
    try:
        s, run = gkl(backend, Aop.shape, k, which, ncv=m, maxiter=maxiter, tol=tol, v0=v0, rng=gen)
    except ArpackNoConvergence as err:
        nconv = len(err.eigenvalues)
        if transposed:  # (the loop's own vectors are those of its V: A's left singular vectors here)
            err.eigenvectors = backend.get_vectors("u", nconv) if nconv else np.zeros((shape[1], 0))
        raise
    if info is not None:
        info.update(run)
        res = backend.residuals(k, s)
        info["residuals"] = res[::-1].copy() if transposed else res
    if return_singular_vectors is False:
        return s
    u = backend.get_vectors(left_side, k) if return_singular_vectors in (True, "u") else None
    vh = np.ascontiguousarray(backend.get_vectors(right_side, k).T) if return_singular_vectors in (True, "vh") else None
    return u, s, vh


def svds(A, k=6, ncv=None, tol=0, which="LM", v0=None, maxiter=None, return_singular_vectors=True, solver="arpack", rng=None,
         random_state=None, options=None, device_id=0, handle=None, info=None):
    """Find ``k`` singular values and vectors of the real ``M x N`` matrix ``A`` - ``scipy.sparse.linalg.svds``'s signature and
    defaults, solved by thick-restart Golub-Kahan-Lanczos bidiagonalisation on the GPU (module docstring).  Returns ``(u, s, vh)``
    with ``u`` of shape ``(M, k)``, ``s`` ascending and ``vh`` of shape ``(k, N)``.

    ``A``: any SciPy sparse format or a dense ndarray with ``min(M, N) >= 2``; float32 is converted to float64 with a notice, complex
    input raises ``NotImplementedError``.  A dense array stays dense on the device - one row-major copy of 8 B per entry, both
    products by dense GEMV kernels on it - unless ``12 count_nonzero(A) < 8 A.size``: then the CSR of its entries is the smaller
    stream and it is packed as CSR like sparse input.  A C-contiguous or F-contiguous float64 array is uploaded as it lies in memory,
    without a host copy or a transpose (an F-ordered ``M x N`` array is the C-ordered ``N x M`` transpose); any other layout or dtype
    takes one contiguous float64 copy.  The loop's short side carries the start vector: for ``M < N`` it runs on ``A^T`` and swaps ``u`` and ``vh`` at the end; ``v0`` has
    length ``min(M, N)`` and ``ncv`` counts against ``min(M, N)``.
    ``1 <= k <= min(M, N) - 1``; ``ncv`` (default ``min(min(M, N), max(2k + 1, 20))``) must satisfy ``k + 2 <= ncv <= min(min(M, N), 128)``;
    ``which``: ``"LM"`` or ``"SM"``.  ``"SM"`` is the same loop keeping the smallest Ritz values, without harmonic extraction: it is
    slow on ill-conditioned matrices.  ``solver`` other than ``"arpack"`` and ``options`` raise ``NotImplementedError``.
    ``rng`` / ``random_state`` (an int or a ``numpy.random.Generator``) seed the private generator of start and breakdown vectors;
    without them the same call gives the same bits, and NumPy's global RNG is never touched.
    ``return_singular_vectors``: ``True`` the triple, ``False`` ``s`` only, ``"u"`` ``(u, s, None)``, ``"vh"`` ``(None, s, vh)``.
    Convergence: ``beta |P[m-1, i]| <= tol * max sigma`` (machine epsilon for ``tol = 0``).  After ``maxiter`` restart cycles (default
    ``10 min(M, N)``) ``ArpackNoConvergence`` carries the converged singular values (ascending) in ``.eigenvalues``, their right
    singular vectors (``(N, nconv)``) in ``.eigenvectors`` and the counts in ``.info``.
    A single-vector method may return fewer copies of a repeated singular value than exist: there is no probe for multiplicities.
    ``handle``: an open ``_capi.Handle`` to run on - its square matrix and thick-restart basis are left alone; ``info``: a dict that
    receives ``matvecs`` (products with ``A`` or ``A^T``), ``cycles``, ``breakdowns``, ``anorm``, ``residuals`` (``(2, k)``:
    ``|A v - sigma u|`` and ``|A^T u - sigma v|``) and ``plan`` (``"dense"`` or ``"csr"``: how the device holds ``A``)."""
    from . import _capi

    h = None

    def make_backend(Aop, AopT):
        nonlocal h
        h = handle if handle is not None else _capi.Handle(device_id)
        if isinstance(Aop, np.ndarray):  # one dense copy: whichever of the two views is C-contiguous, as it lies in memory
            wide = not Aop.flags.c_contiguous
            h.gk_set_dense(AopT if wide else Aop, stored_transposed=wide)
        else:
            h.gk_set_csr(Aop, AopT)
        plan.append("dense" if isinstance(Aop, np.ndarray) else "csr")
        return DeviceGKBackend(h)

    plan = []
    try:
        out = _svds(make_backend, A, k, ncv, tol, which, v0, maxiter, return_singular_vectors, solver, rng, random_state, options, info)
        if info is not None:
            info["plan"] = plan[0]
        return out
    finally:
        if handle is None and h is not None:
            h.close()
