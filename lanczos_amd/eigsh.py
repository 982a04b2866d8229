"""``eigsh``: converged eigenpairs of a symmetric matrix by thick-restart Lanczos on the GPU.

The Krylov basis (at most ``ncv + 1`` rows; ``ncv + b`` in the band form) and every pass over it live on the device (``lz_trl_*`` in
include/lanczos_hip.h); the host keeps only the ``ncv x ncv`` projected matrix ``T`` and runs the outer loop below.

Thick restart (Wu & Simon, 2000) is what ``scipy.sparse.linalg.eigsh`` does for a symmetric matrix in another form (ARPACK's
implicit restart with exact shifts): after ``ncv`` steps the basis is compressed in place to the ``kk`` wanted Ritz vectors, the
residual vector becomes row ``kk`` and the projected matrix becomes ``diag(theta)`` plus an arrow of couplings ``beta s``.

Stopping rule.  A wanted pair is converged when ``beta |s_last| <= tol_eff * max|theta|`` (``tol_eff = tol``, or machine epsilon
when ``tol == 0``).  ARPACK measures against ``tol * max(eps^(2/3), |theta|)`` instead; that bound never converges on Hamiltonians
whose norm is many orders of magnitude above the wanted eigenvalues (the 1-D deuteron: ``||H|| = 2.7e5`` and eigenvalues of
order 1), so the scale here is ``max|theta|``, the norm estimate of the run.

Probe.  A single-vector Krylov method can miss a copy of a degenerate eigenvalue.  When all wanted pairs have converged, the loop
locks them, adds one random direction orthogonal to the basis and asks for one more converged pair than before; it stops only
when the lowest ``k`` wanted values are unchanged between two such rounds.

Band.  ``block_size=b`` runs the loop in Ruhe's band form (``trl_band``): ``b`` start vectors, basis row ``r`` made from ``A V[r - b]``, so
copies of an eigenvalue up to multiplicity ``b`` appear without a probe and the device orthogonalises ``b`` vectors per walk over the
basis; the bookkeeping stays that of single rows.

Complex.  A complex Hermitian ``A`` runs the same loop (``trl``) on the same backends, which then call ``lz_ztrl_*``: ``T`` is Hermitian, the small
problem is ``eigh((T + T^H) / 2)``, the restart's arrow ``T[kk, :kk] = beta S[m - 1, keep]`` has its conjugate in the column, and
start and probe vectors are complex.  For a real backend nothing changes, bit for bit.  ``ncv <= 64`` there.

Breakdown.  When a ``beta`` falls below ``10 eps max|theta|`` the Krylov space is invariant: the loop goes on from a fresh random
vector orthogonal to the basis with a zero coupling instead of dividing by ``beta``.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse
from scipy.sparse.linalg import ArpackNoConvergence

_WHICH = ("LM", "SM", "LA", "SA", "BE")
_EPS = np.finfo(np.float64).eps
_MAX_NCV = 128  # rows of the restart's S held in LDS (lz_trl.hip)
_MAX_NCV_COMPLEX = 64  # complex A: the restart runs on the real form of S, twice the rows and columns in the same LDS (lz_ztrl_api.hip)
_SEED = 0x5EED  # the private generator of start and probe vectors: the same call gives the same bits


def _order(theta, which):
    """indices of theta, most wanted first"""
    if which == "SA":
        return np.argsort(theta, kind="stable")
    if which == "LA":
        return np.argsort(-theta, kind="stable")
    if which == "SM":
        return np.argsort(np.abs(theta), kind="stable")
    return np.argsort(-np.abs(theta), kind="stable")


class NumpyBackend:
    """The calls of the device backend (``lz_trl_*``; ``lz_ztrl_*`` for a complex Hermitian ``A``) in NumPy: what the host tests drive
    the outer loop with.  ``<x, y> = sum conj(x) y`` on a complex matrix; the band, the polynomials and ``rayleigh`` are real-only, as
    on the device."""

    def __init__(self, A, force_second_pass=False, block_size=None):
        self.A = A
        self.n = A.shape[0]
        self.is_complex = is_complex_matrix(A)
        self.dtype = np.complex128 if self.is_complex else np.float64
        self.force = force_second_pass
        self.block_size = block_size
        self.filter = None
        self.series = None

    def _real_only(self, what):
        if self.is_complex:
            raise NotImplementedError(f"{what} with a complex matrix: built for the real basis only")

    def set_filter(self, coefficients, c=0.0):
        """``coefficients``: the (a_i, b_i) of ``ChebFilter.coefficients()``; None: ``extend`` multiplies by A itself again"""
        self._real_only("set_filter")
        self.filter = None if coefficients is None else (np.asarray(coefficients, dtype=np.float64).reshape(-1, 2), float(c))
        self.series = None

    def set_series(self, coefficients, c=0.0, e=1.0):
        """``coefficients``: the ``degree + 1`` values of ``SeriesFilter.coefficients()``; None: ``extend`` multiplies by A itself again"""
        self._real_only("set_series")
        self.series = None if coefficients is None else SeriesFilter.from_coefficients(coefficients, c, e)
        self.filter = None

    def _op(self, x):
        if self.series is not None:
            return self.series.apply(lambda v: self.A @ v, x)
        if self.filter is None:
            return self.A @ x
        coef, c = self.filter
        prev, cur = x, x
        for a, b in coef:  # z = a (A y - c y) - b x, as k_cheb_step forms it
            prev, cur = cur, a * (self.A @ cur - c * cur) - b * prev
        return cur

    def rayleigh(self, k):
        self._real_only("rayleigh")
        Y = self.V[:k]
        return Y @ np.stack([self.A @ Y[i] for i in range(k)]).T

    def begin(self, m, v0):
        self.V = np.zeros((m + 1, self.n), dtype=self.dtype)
        self.V[0] = v0 / np.linalg.norm(v0)

    def _dots(self, k, x):
        """``<V_i, x>``, ``i < k``"""
        return (self.V[:k].conj() if self.is_complex else self.V[:k]) @ x

    def _norm2(self, w):
        return np.vdot(w, w).real if self.is_complex else np.dot(w, w)

    def _cgs(self, w, j):
        c = self._dots(j + 1, w)
        return w - c @ self.V[: j + 1], c

    def extend(self, k, m):
        proj = np.zeros((m, m), dtype=self.dtype)
        beta = np.zeros(m)
        for j in range(k, m):
            w = self._op(self.V[j])
            w0 = self._norm2(w)
            w, c = self._cgs(w, j)
            if self.force or self._norm2(w) < 0.5 * w0:  # DGKS: the second pass only when the first cancelled more than half of |w|
                w, c2 = self._cgs(w, j)
                c = c + c2
            proj[j, : j + 1] = c
            beta[j] = np.linalg.norm(w)
            self.V[j + 1] = w / beta[j]
        return proj, beta

    def begin_band(self, m, X):
        """the band form of ``begin``: ``m + b`` rows, rows ``0..b`` the rows of ``X`` orthonormalised one by one (``probe``)"""
        self._real_only("begin_band")
        X = np.asarray(X, dtype=np.float64)
        self.V = np.zeros((m + len(X), self.n))
        for i in range(len(X)):
            self.probe(i, X[i])

    def extend_band(self, k, m):
        """the band form of ``extend``: step ``j`` makes row ``j + b`` from ``Op V[j]``, orthogonalised against every row below it by two
        CGS passes (no gate).  Returns ``proj`` (``m x (m + b)``: row ``j`` holds the coefficients on rows ``0..j+b``) and ``beta`` (``m``)."""
        self._real_only("extend_band")
        b = len(self.V) - m
        proj = np.zeros((m, m + b))
        beta = np.zeros(m)
        for j in range(k, m):
            w = self._op(self.V[j])
            w, c = self._cgs(w, j + b - 1)
            w, c2 = self._cgs(w, j + b - 1)
            proj[j, : j + b] = c + c2
            beta[j] = np.linalg.norm(w)
            with np.errstate(divide="ignore", invalid="ignore"):
                self.V[j + b] = w / beta[j]
        return proj, beta

    def restart(self, m, kk, S):
        nb = len(self.V) - m  # 1, or the band width: the residual rows move down behind the kept ones
        self.V[:kk] = S.T @ self.V[:m]
        self.V[kk: kk + nb] = self.V[m: m + nb].copy()

    def probe(self, k, x):
        for _ in range(2):
            x = x - self._dots(k, x) @ self.V[:k]
        self.V[k] = x / np.linalg.norm(x)

    def get_vectors(self, k):
        return self.V[:k].T.copy()

    def residuals(self, k, theta):
        return np.array([np.linalg.norm(self.A @ self.V[i] - theta[i] * self.V[i]) for i in range(k)])


ComplexNumpyBackend = NumpyBackend  # the name the complex host twin had while it was a class of its own: callers written for it still import


def _check_problem(n, k, which, M=None, sigma=None, Minv=None, OPinv=None, mode="normal"):
    """SciPy's argument errors for everything but ``ncv``"""
    if M is not None or sigma is not None or Minv is not None or OPinv is not None:
        raise NotImplementedError("eigsh on the device solves the standard problem only: M, sigma, Minv and OPinv must be None")
    if mode != "normal":
        raise NotImplementedError(f"mode={mode!r}: only mode='normal' is implemented")
    if which not in _WHICH:
        raise ValueError(f"which must be one of {' '.join(_WHICH)}")
    if which == "BE":
        raise NotImplementedError("which='BE' is not implemented")
    if k <= 0:
        raise ValueError("k must be greater than 0.")
    if k >= n:
        raise TypeError(f"k >= N for an N x N matrix (k={k}, N={n}): reduce k")


def check_args(n, k, which, ncv, M=None, sigma=None, Minv=None, OPinv=None, mode="normal", complex_A=False):
    """SciPy's argument errors, plus this solver's own limits.  Returns ncv.  ``complex_A``: the cap of the complex solver."""
    _check_problem(n, k, which, M, sigma, Minv, OPinv, mode)
    if ncv is None:
        ncv = min(n, max(2 * k + 1, 20))
    ncv = min(int(ncv), n)  # (as SciPy does)
    if complex_A and not k + 3 <= ncv <= min(n, _MAX_NCV_COMPLEX):
        raise ValueError(f"ncv must be k+3<=ncv<=min(n, {_MAX_NCV_COMPLEX}) for a complex Hermitian matrix, ncv={ncv} (the complex cap: the "
                         f"restart kernel holds the real form of S, 2 ncv rows, where a real matrix may have {_MAX_NCV}; pass a smaller ncv or k)")
    if not k + 3 <= ncv <= min(n, _MAX_NCV):
        raise ValueError(f"ncv must be k+3<=ncv<=min(n, {_MAX_NCV}), ncv={ncv} (stricter than SciPy's k<ncv<=n: the thick restart keeps "
                         "two spare basis rows and one more for the probe direction)")
    return ncv


def _start(n, tol, v0, rng, cplx=False):
    """``(rng, tol_eff, v0)``: the generator, the effective tolerance and the checked start vector (drawn only when none is given;
    ``cplx``: real and imaginary part, in that order, from the same generator)"""
    rng = np.random.default_rng(_SEED) if rng is None else rng
    tol_eff = float(tol) if tol > 0 else _EPS
    if cplx:
        v0 = rng.uniform(-1.0, 1.0, n) + 1j * rng.uniform(-1.0, 1.0, n) if v0 is None else np.asarray(v0, dtype=np.complex128).reshape(-1)
    else:
        v0 = rng.uniform(-1.0, 1.0, n) if v0 is None else np.asarray(v0, dtype=np.float64).reshape(-1)
    if v0.shape != (n,) or not np.linalg.norm(v0) > 0:
        raise ValueError("v0 must be a non-zero vector of length n")
    return rng, tol_eff, v0


def _probe_vector(rng, n, cplx):
    """the random direction of a probe or of the fresh start behind a breakdown"""
    return rng.standard_normal(n) + 1j * rng.standard_normal(n) if cplx else rng.standard_normal(n)


def _fill(T, proj, beta, j0, j1, couplings=True):
    """columns ``j0 .. j1 - 1`` of the projected matrix ``T`` (and their rows) from what ``extend`` returned; ``couplings``: the
    ``beta`` beside the diagonal as well.  A complex ``T`` is Hermitian: ``proj[j, i] = <V_i, A V_j>`` is column ``j``, the row its conjugate."""
    cplx = np.iscomplexobj(T)
    for j in range(j0, j1):
        T[: j + 1, j] = proj[j, : j + 1]
        T[j, : j + 1] = np.conj(proj[j, : j + 1]) if cplx else proj[j, : j + 1]
        if couplings and j + 1 < len(T):
            T[j + 1, j] = T[j, j + 1] = beta[j]


def trl(backend, n, k, which="LM", ncv=None, maxiter=None, tol=0.0, v0=None, probe=True, rng=None):
    """The thick-restart outer loop over a backend (``NumpyBackend`` or ``DeviceBackend``).

    Returns ``(theta, info)``: the ``k`` wanted eigenvalues in ascending order (``backend.V[0..k)`` then holds their vectors) and
    ``{"matvecs", "cycles", "probes", "breakdowns", "anorm"}`` (anorm: max|theta| over the run, the norm estimate).  Raises ``ArpackNoConvergence`` after ``maxiter`` cycles."""
    cplx = bool(getattr(backend, "is_complex", False))  # a complex Hermitian backend: T Hermitian, complex start and probe vectors
    dt = np.complex128 if cplx else np.float64
    m = check_args(n, k, which, ncv, complex_A=cplx)
    maxiter = n * 10 if maxiter is None else int(maxiter)
    rng, tol_eff, v0 = _start(n, tol, v0, rng, cplx)
    backend.begin(m, v0)
    T = np.zeros((m, m), dtype=dt)
    kcur, nw, last = 0, k, None
    anorm = 0.0
    info = {"matvecs": 0, "cycles": 0, "probes": 0, "breakdowns": 0}
    while True:
        j0 = kcur
        while True:  # one extension of the basis to m rows; a breakdown restarts it behind the invariant subspace
            proj, beta = backend.extend(j0, m)
            info["matvecs"] += m - j0
            _fill(T, proj, beta, j0, m)
            scale = max(anorm, np.abs(T).max())
            bad = [j for j in range(j0, m - 1) if not beta[j] > 10 * _EPS * scale]
            if not bad:
                break
            jb = bad[0]
            info["breakdowns"] += 1
            T[jb + 1:, :] = 0.0
            T[:, jb + 1:] = 0.0
            _fill(T, proj, beta, j0, jb + 1, couplings=False)
            backend.probe(jb + 1, _probe_vector(rng, n, cplx))
            j0 = jb + 1
        info["cycles"] += 1
        b_last = beta[m - 1]
        theta, S = np.linalg.eigh((T + T.conj().T) / 2 if cplx else (T + T.T) / 2)
        anorm = max(np.abs(theta).max(), anorm)
        res = b_last * np.abs(S[m - 1])
        order = _order(theta, which)
        want = order[:nw]
        ok = res <= tol_eff * anorm
        dead = not b_last > 10 * _EPS * anorm  # the last residual vanished: V[m] is noise, replace it after the restart
        done = ok[want].all()
        if done:
            top = order[:k]
            cur = np.sort(theta[top])
            if not probe or (last is not None and np.abs(cur - last).max() <= 1e3 * tol_eff * anorm):
                sel = top[np.argsort(theta[top], kind="stable")]
                backend.restart(m, k, np.ascontiguousarray(S[:, sel]))
                info["anorm"] = anorm
                return theta[sel], info
        if info["cycles"] >= maxiter:
            conv = sorted((i for i in order[:k] if ok[i]), key=lambda i: theta[i])
            vecs = np.zeros((n, 0), dtype=dt)
            if conv:
                backend.restart(m, len(conv), np.ascontiguousarray(S[:, conv]))
                vecs = backend.get_vectors(len(conv))
            err = ArpackNoConvergence(f"No convergence ({info['cycles']} iterations, {len(conv)}/{k} eigenvectors converged)",
                                      theta[conv], vecs)
            err.info = info  # the counts of the run that gave up
            raise err
        if done:
            last = cur
            backend.restart(m, nw, np.ascontiguousarray(S[:, want]))
            backend.probe(nw, _probe_vector(rng, n, cplx))
            info["probes"] += 1
            T = np.zeros((m, m), dtype=dt)
            T[np.arange(nw), np.arange(nw)] = theta[want]
            kcur, nw = nw, min(nw + 1, m - 3)
        else:
            nconv = int(ok[want].sum())
            kk = min(m - 2, nw + max(nconv, (m - nw) // 2))
            keep = order[:kk]
            backend.restart(m, kk, np.ascontiguousarray(S[:, keep]))
            T = np.zeros((m, m), dtype=dt)
            T[np.arange(kk), np.arange(kk)] = theta[keep]
            if dead:
                backend.probe(kk, _probe_vector(rng, n, cplx))
            elif cplx:  # A Y_k = theta_k Y_k + beta S[m-1, k] V[m]: the arrow's row, its conjugate in the column
                T[kk, :kk] = b_last * S[m - 1, keep]
                T[:kk, kk] = np.conj(T[kk, :kk])
            else:
                T[:kk, kk] = T[kk, :kk] = b_last * S[m - 1, keep]
            kcur = kk


_MAX_BLOCK = 8  # the widest band the device kernels are built for (lz_trl.hip)


def check_block_size(block_size):
    """``block_size`` as an int; ``ValueError`` unless it is an integer ``2 .. 8``"""
    if isinstance(block_size, bool) or not isinstance(block_size, (int, np.integer)) or not 2 <= block_size <= _MAX_BLOCK:
        raise ValueError(f"block_size must be None or an integer 2 <= block_size <= {_MAX_BLOCK}, got {block_size!r}")
    return int(block_size)


def check_band_args(n, k, which, ncv, block_size, M=None, sigma=None, Minv=None, OPinv=None, mode="normal"):
    """``check_args`` for the band loop: the same errors for everything but ``ncv``, which must leave ``b`` residual rows behind the
    basis and ``2 b + 1`` free rows in front of them.  Returns ``(ncv, b)``."""
    b = check_block_size(block_size)
    if sigma is not None:
        raise NotImplementedError("block_size with sigma: the interior mode's certificate is defined for the single-vector loop only")
    _check_problem(n, k, which, M, sigma, Minv, OPinv, mode)
    top = min(n - b, _MAX_NCV)
    if ncv is None:
        ncv = min(top, max(2 * k + 1, 20, k + 2 * b + 1))
    ncv = int(ncv)
    if not k + 2 * b + 1 <= ncv <= top:
        raise ValueError(f"ncv must be k+2b+1<=ncv<=min(n-b, {_MAX_NCV}) with block_size b={b}, ncv={ncv}: the band restart keeps b residual "
                         "rows behind the basis and needs b + 1 free rows in front of them, and the probe one more pair")
    return ncv, b


def _start_block(n, b, v0, rng):
    """the ``b`` start vectors of the band loop: ``v0`` if given, the rest uniform(-1, 1) from the private generator"""
    X = rng.uniform(-1.0, 1.0, (b, n))
    if v0 is not None:
        X[0] = v0
    return X


def trl_band(backend, n, k, which="LM", block_size=2, ncv=None, maxiter=None, tol=0.0, v0=None, probe=True, rng=None):
    """The thick-restart outer loop in Ruhe's band form: ``b = block_size`` start vectors, basis row ``r`` made from ``Op V[r - b]``.

    The basis has ``m + b`` rows (``m = ncv``).  ``F`` (``m x (m + b)``) holds in row ``j`` the coefficients of ``Op V[j]`` on the
    basis: what ``extend_band`` measured (``F[j, j + b] = beta[j]``) or, for a kept Ritz vector, its value and its couplings to the
    ``b`` residual rows.  ``T[i, j] = F[j, i]`` (``i <= j``) is the projected matrix, ``Rl[r, jj] = F[m - b + jj, m + r]`` the ``b x b``
    upper triangle that couples the last ``b`` rows to the residual rows: the residual of Ritz pair ``i`` is exactly
    ``|Rl S[m-b..m, i]|``.  A copy of an eigenvalue of multiplicity up to ``b`` needs no probe.  A breakdown is still one tiny
    ``beta`` (``<= 10 eps scale (j + b)``, see below) and one replaced row (deflation is exact: only the deficient direction is replaced, so no part of a residual is
    hidden from the estimate, which replacing a whole block would do).

    Returns ``(theta, info)`` as ``trl`` does, ``info["block_size"] = b``."""
    m, b = check_band_args(n, k, which, ncv, block_size)
    maxiter = n * 10 if maxiter is None else int(maxiter)
    rng = np.random.default_rng(_SEED) if rng is None else rng
    tol_eff = float(tol) if tol > 0 else _EPS
    if v0 is not None:
        v0 = np.asarray(v0, dtype=np.float64).reshape(-1)
        if v0.shape != (n,) or not np.linalg.norm(v0) > 0:
            raise ValueError("v0 must be a non-zero vector of length n")
    backend.begin_band(m, _start_block(n, b, v0, rng))
    F = np.zeros((m, m + b))
    kcur, nw, last = 0, k, None
    anorm = 0.0
    info = {"matvecs": 0, "cycles": 0, "probes": 0, "breakdowns": 0, "block_size": b}
    steps = np.arange(m)
    while True:
        j0 = kcur
        while True:  # one extension of the basis to m + b rows; a breakdown replaces one row and goes on behind it
            proj, beta = backend.extend_band(j0, m)
            info["matvecs"] += m - j0
            F[j0:] = proj[j0:]
            F[steps[j0:], steps[j0:] + b] = beta[j0:]
            # the first breakdown: a row behind it is made from a normalised rounding error, so neither it nor any later step of this
            # extension may enter the scale (the device went on without a synchronisation: those steps hold anything, NaN included)
            # The bound is 10 eps scale times the j + b rows the step subtracted: a sum of r rounded terms errs by up to r eps of their
            # size, and that error is what is left of w when the Krylov space has run out.  (10 eps scale alone, the single-vector
            # loop's bound, lies below the device's rounding from about ten rows on: on diag(1, 2, 3) x 10 with b = 4 steps 16 .. 18
            # left 7e-16, 2e-15 and 1.3e-14 against 6.7e-15, and the row made of the last one cost all orthogonality.)
            scale = max(anorm, np.abs(F[:j0]).max()) if j0 else anorm
            jb = None
            for j in range(j0, m):
                scale = max(scale, np.abs(F[j, : j + b]).max())
                if not beta[j] > 10 * _EPS * scale * (j + b):
                    jb = j
                    break
            if jb is None or jb == m - 1:
                break
            info["breakdowns"] += 1
            F[jb + 1:] = 0.0
            F[jb, jb + b] = 0.0
            backend.probe(jb + b, rng.standard_normal(n))
            j0 = jb + 1
        info["cycles"] += 1
        dead = jb is not None  # the last residual vanished: row m + b - 1 is noise, replaced after the restart
        if dead:
            F[m - 1, m + b - 1] = 0.0
        T = np.triu(F[:, :m].T)
        T = T + np.triu(T, 1).T
        theta, S = np.linalg.eigh(T)
        anorm = max(np.abs(theta).max(), anorm)
        Rl = F[m - b:, m:].T
        C = Rl @ S[m - b:]  # column i: the coefficients of pair i's residual on the b residual rows
        res = np.linalg.norm(C, axis=0)
        order = _order(theta, which)
        want = order[:nw]
        ok = res <= tol_eff * anorm
        done = ok[want].all()
        if done:
            top = order[:k]
            cur = np.sort(theta[top])
            if not probe or (last is not None and np.abs(cur - last).max() <= 1e3 * tol_eff * anorm):
                sel = top[np.argsort(theta[top], kind="stable")]
                backend.restart(m, k, np.ascontiguousarray(S[:, sel]))
                info["anorm"] = anorm
                return theta[sel], info
        if info["cycles"] >= maxiter:
            conv = sorted((i for i in order[:k] if ok[i]), key=lambda i: theta[i])
            vecs = np.zeros((n, 0))
            if conv:
                backend.restart(m, len(conv), np.ascontiguousarray(S[:, conv]))
                vecs = backend.get_vectors(len(conv))
            err = ArpackNoConvergence(f"No convergence ({info['cycles']} iterations, {len(conv)}/{k} eigenvectors converged)",
                                      theta[conv], vecs)
            err.info = info
            raise err
        if done:  # probe round: lock the wanted pairs, swap the last residual row for a random direction, ask for one pair more
            last = cur
            kk, keep = nw, want
        else:
            nconv = int(ok[want].sum())
            kk = min(m - b - 1, nw + max(nconv, (m - nw) // 2))
            keep = order[:kk]
        backend.restart(m, kk, np.ascontiguousarray(S[:, keep]))
        F = np.zeros((m, m + b))
        F[np.arange(kk), np.arange(kk)] = theta[keep]
        F[:kk, kk: kk + b] = C[:, keep].T
        if done:
            backend.probe(kk + b - 1, rng.standard_normal(n))
            F[:, kk + b - 1] = 0.0
            info["probes"] += 1
            nw = min(nw + 1, m - 2 * b - 1)
        elif dead:
            backend.probe(kk + b - 1, rng.standard_normal(n))
            F[:, kk + b - 1] = 0.0
        kcur = kk


class ChebFilter:
    """The scaled Chebyshev polynomial ``p`` of degree ``degree`` that damps ``[lo, hi]`` and has ``p(anchor) = 1``:
    ``p(t) = T_d((t - c) / e) / T_d((anchor - c) / e)`` with ``c = (lo + hi) / 2``, ``e = (hi - lo) / 2``.  ``anchor`` lies outside the
    interval, on the side of the wanted eigenvalues; between the anchor and the far end of the interval ``|p| <= 1``, and ``p`` grows
    monotonically from the near edge to the anchor.  ``ChebFilter(..., A=A) @ x`` is ``p(A) x``, so ``NumpyBackend`` takes it as a matrix."""

    def __init__(self, lo, hi, anchor, degree, A=None):
        self.lo, self.hi, self.anchor, self.degree = float(lo), float(hi), float(anchor), int(degree)
        if not self.lo < self.hi or self.lo <= self.anchor <= self.hi or self.degree < 1:
            raise ValueError("ChebFilter needs lo < hi, an anchor outside [lo, hi] and degree >= 1")
        self.c = (self.lo + self.hi) / 2
        self.e = (self.hi - self.lo) / 2
        self.A = A
        self.shape = None if A is None else A.shape

    def apply(self, matvec, x):
        """``p(A) x`` by the scaled three-term recurrence (Saad; Zhou & Saad 2007); ``matvec(v)`` is ``A v``"""
        c, e = self.c, self.e
        s1 = e / (self.anchor - c)
        s = s1
        y = (s1 / e) * (matvec(x) - c * x)
        for _ in range(2, self.degree + 1):
            s2 = 1.0 / (2.0 / s1 - s)
            z = 2.0 * (s2 / e) * (matvec(y) - c * y) - (s * s2) * x
            x, y, s = y, z, s2
        return y

    def __matmul__(self, x):
        return self.apply(lambda v: self.A @ v, x)

    def poly(self, lam):
        """``p(lam)`` in closed form"""
        d = self.degree

        def cheb(t):
            t = np.asarray(t, dtype=np.float64)
            inside = np.abs(t) <= 1
            out = np.cos(d * np.arccos(np.clip(t, -1, 1)))
            big = np.cosh(d * np.arccosh(np.maximum(np.abs(t), 1))) * np.where((t < 0) & (d % 2 == 1), -1.0, 1.0)
            return np.where(inside, out, big)

        return cheb((np.asarray(lam, dtype=np.float64) - self.c) / self.e) / cheb((self.anchor - self.c) / self.e)

    def coefficients(self):
        """The ``degree`` pairs ``(a_i, b_i)`` of ``z = a_i (A y - c y) - b_i x`` as a ``(degree, 2)`` array: what the device takes as data"""
        c, e = self.c, self.e
        s1 = e / (self.anchor - c)
        s = s1
        out = [(s1 / e, 0.0)]
        for _ in range(2, self.degree + 1):
            s2 = 1.0 / (2.0 / s1 - s)
            out.append((2.0 * (s2 / e), s * s2))
            s = s2
        return np.array(out)


_RANGE_CAP = 1e4  # the filter may spread the k wanted eigenvalues of p(A) over at most this ratio (see filter_plan)


def _check_degree(filter_degree):
    if isinstance(filter_degree, bool) or not isinstance(filter_degree, (int, np.integer)) or filter_degree < 2:
        raise ValueError(f"filter_degree must be an integer >= 2, got {filter_degree!r}")
    return int(filter_degree)


def check_filter_args(which, filter_degree):
    """The filter's own argument errors (``check_args`` keeps SciPy's).  Returns the degree as an int."""
    degree = _check_degree(filter_degree)
    if which not in ("SA", "LA"):
        raise ValueError(f"filter_degree needs which='SA' or 'LA' (got {which!r}): the Chebyshev filter serves one end of the spectrum; "
                         "for the eigenvalues nearest a point inside it pass sigma= with which='LM' (sigma=0.0 for 'SM')")
    return degree


def _outer_bounds(theta, S_last, b_last):
    """``(lo, hi)`` that hold the spectrum, from Ritz values ``theta`` (ascending), the last row of their vectors and the last ``beta``:
    see ``filter_plan``"""
    width = theta[-1] - theta[0]
    hi = theta[-1] + b_last * abs(S_last[-1]) + 1e-3 * width
    lo = theta[0] - b_last * abs(S_last[0]) - 1e-3 * width
    return lo, hi


def _stage0(backend, m, v0):
    """Stage 0 of the filtered drivers: ``m`` plain steps from ``v0``.  Returns the Ritz values, the last row of their vectors, the
    last ``beta`` and the outer bounds ``(lo, hi)`` of the spectrum."""
    backend.begin(m, v0)
    backend.set_filter(None)  # (clears a series as well)
    T = np.zeros((m, m))
    proj, beta = backend.extend(0, m)
    _fill(T, proj, beta, 0, m)
    if not beta[: m - 1].min() > 10 * _EPS * np.abs(T).max():
        # the Krylov space of v0 is invariant before ncv steps: its Ritz values bound only that subspace, not the spectrum, so no safe
        # filter can be built from them (the unfiltered loop handles such a start by itself)
        raise ValueError("filter_degree: the start vector's Krylov space is invariant after fewer than ncv steps (breakdown in the "
                         "bounds stage); run without filter_degree, or with another v0")
    theta, S = np.linalg.eigh((T + T.T) / 2)
    return theta, S[m - 1], beta[m - 1], _outer_bounds(theta, S[m - 1], beta[m - 1])


def _ritz_in_A(backend, m, kc, pick=None):
    """Rayleigh-Ritz with ``A`` itself on ``V[0..kc)``.  ``pick(lam)``: the indices of the ascending eigenvalues ``lam`` to keep
    (None: all); the rows kept are rotated in place to ``V[0..len)``.  Returns their eigenvalues and residuals."""
    G = backend.rayleigh(kc)
    lam, Q = np.linalg.eigh((G + G.T) / 2)
    if pick is not None:
        sel = pick(lam)
        lam, Q = lam[sel], Q[:, sel]
    if not len(lam):
        return lam, np.zeros(0)
    S = np.zeros((m, len(lam)))
    S[:kc] = Q
    backend.restart(m, len(lam), S)
    return lam, backend.residuals(len(lam), lam)


def filter_plan(theta, S_last, b_last, k, which, degree):
    """The filter for ``which`` from stage 0's Ritz values ``theta`` (ascending), the last row of their vectors and the last ``beta``.

    Outer bounds: ``theta_max + beta |s_max|`` and ``theta_min - beta |s_min|`` (an eigenvalue lies within ``beta |s|`` of a Ritz
    value), each widened by 1e-3 of the width.  Inner edge: the Ritz value with index ``max(m // 2, k + 2)`` counted from the wanted
    end - Ritz values never lie beyond the eigenvalues of the same index, so the ``k`` wanted ones stay outside the damped interval.
    Range cap: the loop converges residuals of ``B = p(A)`` to ``eps |B|``; a wanted eigenvalue of ``B`` at ``rho |B|`` then has a
    vector good to ``eps / rho`` only.  With ``t_a``, ``t_k`` the images ``|lam - c| / e`` of the anchor and of the ``k``-th wanted Ritz
    value (which errs towards the damped interval), ``p(lam_k) >= ~exp(-d (acosh t_a - acosh t_k))``: the degree used is the largest
    ``d' <= degree``, at least 2, that keeps this above 1e-4, i.e. true residuals near 1e-12 |A|."""
    m = len(theta)
    bottom, top = _outer_bounds(theta, S_last, b_last)
    idx = max(m // 2, k + 2)
    if which == "SA":
        lo, hi, anchor, th_k = theta[idx], top, bottom, theta[k - 1]
    else:
        lo, hi, anchor, th_k = bottom, theta[m - 1 - idx], top, theta[m - k]
    c, e = (lo + hi) / 2, (hi - lo) / 2
    gap = np.arccosh(abs(anchor - c) / e) - np.arccosh(max(abs(th_k - c) / e, 1.0))
    used = degree if gap * degree <= np.log(_RANGE_CAP) else int(np.log(_RANGE_CAP) / gap)
    return ChebFilter(lo, hi, anchor, max(2, min(degree, used)))


def trl_filtered(backend, n, k, which, degree, ncv=None, maxiter=None, tol=0.0, v0=None, probe=True, rng=None, block_size=None):
    """Thick-restart Lanczos on ``B = p(A)``, ``p`` a Chebyshev filter that damps the unwanted part of the spectrum (Zhou & Saad's
    filtered Lanczos): ``B`` has ``A``'s eigenvectors and its wanted eigenvalues are far better separated, so the loop takes far fewer
    Gram-Schmidt steps at ``degree`` products with ``A`` each.

    Stage 0: ``ncv`` plain steps give the bounds of the spectrum and the filter (``filter_plan``); a breakdown there (an invariant
    Krylov space: ``ncv = n``, a handful of distinct eigenvalues) raises ``ValueError`` - the unfiltered loop is the one for such input.  Then the unchanged ``trl`` runs on
    ``B`` for its largest eigenvalues, and one Rayleigh-Ritz step with ``A`` itself on the ``k`` vectors gives the eigenvalues of ``A``.
    Acceptance is in ``A``-space: a pair whose true residual exceeds ``1e3 tol_eff 1e4 |A|`` (the range cap's error model with the
    loop's factor 1e3) is not returned; ``ArpackNoConvergence`` then carries the pairs that pass.

    ``block_size=b``: stage 0 runs single-vector as without it, then ``trl_band`` runs on ``B`` (``ncv`` follows the band's rule).

    Returns ``(theta, info)`` as ``trl`` does; ``info`` has ``"steps"`` (Gram-Schmidt steps, stage 0 included), ``"matvecs"`` (products
    with ``A``: stage 0, ``degree`` per filtered step, Rayleigh-Ritz), ``"filter"`` and ``trl``'s other counts."""
    degree = check_filter_args(which, degree)
    m = check_args(n, k, which, ncv) if block_size is None else check_band_args(n, k, which, ncv, block_size)[0]
    rng, tol_eff, v0 = _start(n, tol, v0, rng)
    theta0, s_last, b_last, _ = _stage0(backend, m, v0)
    filt = filter_plan(theta0, s_last, b_last, k, which, degree)
    anorm = max(abs(filt.anchor), abs(filt.hi), abs(filt.lo))
    res_bound = 1e3 * tol_eff * _RANGE_CAP * anorm
    # the loop on B = p(A): the wanted images are positive and the largest, the anchor lies on their side
    if block_size is not None:  # (a basis of another size drops the device's filter: size it before the filter is set)
        backend.begin_band(m, _start_block(n, block_size, v0, np.random.default_rng(_SEED)))
    backend.set_filter(filt.coefficients(), filt.c)
    try:
        if block_size is None:
            _, run = trl(backend, n, k, "LA", ncv=m, maxiter=maxiter, tol=tol, v0=v0, probe=probe, rng=rng)
        else:
            _, run = trl_band(backend, n, k, "LA", block_size, ncv=m, maxiter=maxiter, tol=tol, v0=v0, probe=probe, rng=rng)
    except ArpackNoConvergence as e:  # its pairs are those of B: hand on what they give for A
        kc = len(e.eigenvalues)
        backend.set_filter(None)
        lam, res = _ritz_in_A(backend, m, kc) if kc else (np.zeros(0), np.zeros(0))
        ok = res <= res_bound
        vecs = backend.get_vectors(kc)[:, ok] if kc else np.zeros((n, 0))
        raise ArpackNoConvergence(e.args[0], lam[ok], vecs) from None
    backend.set_filter(None)
    lam, res = _ritz_in_A(backend, m, k)
    ok = res <= res_bound
    info = dict(run)
    info["steps"] = m + run["matvecs"]
    info["matvecs"] = m + run["matvecs"] * filt.degree + k
    info["anorm"] = anorm
    info["filter"] = {"requested": degree, "degree": filt.degree, "lo": filt.lo, "hi": filt.hi, "anchor": filt.anchor}
    if not ok.all():
        raise ArpackNoConvergence(f"No convergence ({int(ok.sum())}/{k} eigenvectors pass the residual test of the filtered run)",
                                  lam[ok], backend.get_vectors(k)[:, ok])
    return lam, info


class SeriesFilter:
    """The Chebyshev series ``p`` of degree ``degree`` that peaks at ``sigma`` inside ``[lo, hi]``: the Jackson-damped expansion of a
    delta function, ``p(t) = sum_i g_i mu_i T_i(t) / norm`` with ``t = (lam - c) / e``, ``mu_i = (2 - delta_i0) cos(i acos s)``,
    ``s = (sigma - c) / e``, ``g_i`` the Jackson coefficients of ``degree + 1`` terms (Weisse et al., "The kernel polynomial method",
    2006) and ``norm`` such that ``p(sigma) = 1``.  In the angle ``phi = acos t`` this is ``(J(phi - phi_s) + J(phi + phi_s)) / 2`` of
    the positive Jackson kernel ``J``, a lobe of width about ``pi / (degree + 2)``.  With ``sigma`` at the centre of the interval the
    maximum is at ``sigma`` and ``|p| <= 1`` on ``[lo, hi]``; elsewhere the mirror lobe's slope moves the maximum a fraction of a lobe
    off ``sigma`` and above one - by 1e-8 several lobes from an end, by up to 0.2 within a lobe of it (measured, degrees 2 to 256) -
    which the interior solver's window certificate (``trl_interior``) does not mind.
    ``SeriesFilter(..., A=A) @ x`` is ``p(A) x``."""

    def __init__(self, lo, hi, sigma, degree, A=None):
        self.lo, self.hi, self.sigma, self.degree = float(lo), float(hi), float(sigma), int(degree)
        if not self.lo < self.hi or not self.lo <= self.sigma <= self.hi or self.degree < 1:
            raise ValueError("SeriesFilter needs lo < hi, sigma inside [lo, hi] and degree >= 1")
        self.c = (self.lo + self.hi) / 2
        self.e = (self.hi - self.lo) / 2
        d = self.degree
        i = np.arange(d + 1)
        phi = np.arccos(np.clip((self.sigma - self.c) / self.e, -1.0, 1.0))
        mu = np.where(i == 0, 1.0, 2.0) * np.cos(i * phi)
        q = np.pi / (d + 2)
        g = ((d + 2 - i) * np.cos(i * q) + np.sin(i * q) / np.tan(q)) / (d + 2)
        coef = g * mu
        self.coef = coef / np.dot(coef, np.cos(i * phi))
        self.A = A
        self.shape = None if A is None else A.shape

    @classmethod
    def from_coefficients(cls, coefficients, c, e):
        """the series with these ``degree + 1`` coefficients on ``[c - e, c + e]`` (what a backend is handed)"""
        self = cls.__new__(cls)
        self.coef = np.asarray(coefficients, dtype=np.float64).reshape(-1).copy()
        self.degree = len(self.coef) - 1
        self.c, self.e = float(c), float(e)
        if self.degree < 1 or not self.e > 0:
            raise ValueError("a series needs at least two coefficients and e > 0")
        self.lo, self.hi, self.sigma, self.A, self.shape = self.c - self.e, self.c + self.e, None, None, None
        return self

    def coefficients(self):
        """The ``degree + 1`` coefficients of ``T_0 .. T_degree``: what the device takes as data (with ``c`` and ``e``)"""
        return self.coef.copy()

    def apply(self, matvec, x):
        """``p(A) x`` by the three-term recurrence ``T_1 = (A x - c x) / e``, ``T_{i+1} = (2 / e)(A T_i - c T_i) - T_{i-1}``, every term
        added to the sum as it is formed (k_cheb_series_step's order); ``matvec(v)`` is ``A v``"""
        c, inv_e, mu = self.c, 1.0 / self.e, self.coef
        y = inv_e * (matvec(x) - c * x)
        acc = mu[0] * x + mu[1] * y
        for i in range(2, self.degree + 1):
            z = (2.0 * inv_e) * (matvec(y) - c * y) - x
            acc = acc + mu[i] * z
            x, y = y, z
        return acc

    def __matmul__(self, x):
        return self.apply(lambda v: self.A @ v, x)

    def poly(self, lam):
        """``p(lam)`` in closed form (``lam`` inside ``[lo, hi]``; clipped to it)"""
        phi = np.arccos(np.clip((np.asarray(lam, dtype=np.float64) - self.c) / self.e, -1.0, 1.0))
        return np.cos(np.multiply.outer(phi, np.arange(self.degree + 1))) @ self.coef

    def window_min(self, a, b, points):
        """the smallest ``p`` on a grid of ``points`` values between ``a`` and ``b``, equispaced in ``acos t``, ends included"""
        t = np.clip((np.array([a, b]) - self.c) / self.e, -1.0, 1.0)
        pa, pb = np.arccos(t)
        return float(self.poly(self.c + self.e * np.cos(np.linspace(pa, pb, int(points)))).min())


def check_interior_args(which, sigma, filter_degree):
    """The argument rules of the interior mode.  Returns ``None`` without ``sigma`` (``check_args`` and ``check_filter_args`` then
    decide as before), else ``(sigma, degree)``: ``sigma`` needs ``which="LM"`` - SciPy's meaning, the eigenvalues nearest ``sigma`` -
    and ``filter_degree``."""
    if sigma is None:
        return None
    if filter_degree is None:
        raise NotImplementedError("sigma: there is no shift-invert on the device; pass filter_degree=d (an integer >= 2) and the "
                                  "eigenvalues nearest sigma are found through a Chebyshev series of A of at most that degree")
    if which != "LM":
        raise NotImplementedError(f"sigma with which={which!r}: only which='LM' (the eigenvalues nearest sigma) is implemented")
    degree = _check_degree(filter_degree)
    if isinstance(sigma, (bool, str)) or not np.isscalar(sigma) or not np.isreal(sigma) or not np.isfinite(sigma):
        raise ValueError(f"sigma must be a finite real number, got {sigma!r}")
    return float(sigma), degree


def trl_interior(backend, n, k, sigma, degree, ncv=None, maxiter=None, tol=0.0, v0=None, probe=True, rng=None, _certify=True):
    """The ``k`` eigenvalues of ``A`` nearest ``sigma`` by thick-restart Lanczos on ``B = p(A)``, ``p`` a ``SeriesFilter`` that peaks
    at ``sigma``: the interior of ``A``'s spectrum is the top of ``B``'s, where Lanczos converges fast.

    Stage 0: ``ncv`` plain steps bound the spectrum as in ``trl_filtered`` (same ``ValueError`` on a breakdown); ``sigma`` outside the
    bounds is an extremal problem and raises ``ValueError``.  Then the unchanged ``trl`` finds the ``kb = k + max(4, k // 4)`` largest
    eigenvalues of ``B``, one Rayleigh-Ritz step with ``A`` itself on the ``kb`` vectors gives eigenvalues of ``A``, and the ``k``
    nearest ``sigma`` are moved to ``V[0..k)`` in ascending order.

    Certificate.  ``p`` is not monotone in the distance from ``sigma`` (side lobes; a maximum pulled towards a near end of the
    spectrum), so the ``kb`` largest of ``B`` need not contain the ``k`` nearest.  With ``p_min`` the smallest converged eigenvalue of
    ``B``, every eigenvalue ``lam`` of ``A`` with ``p(lam) > p_min`` is among the ``kb`` found; so if ``p > p_min`` on the whole window
    ``[sigma - d_k, sigma + d_k]`` (``d_k``: the distance of the ``k``-th nearest value found; the window clipped to the bounds and
    sampled at ``16 degree + 64`` points equispaced in ``acos t``, 16 per oscillation of ``p`` at least), nothing inside the window was
    missed and the ``k`` nearest found are the ``k`` nearest.  The margin is the loop's own convergence bound, ``1e3 tol_b |B|``
    (``tol_b = max(tol, 4 eps)``: the loop on ``B`` is not asked for residuals below the rounding of ``p(A) x`` itself).
    The ``k`` pairs must also pass ``trl_filtered``'s residual test in ``A``-space.  An attempt that fails either is run again at
    half the degree (a wider lobe), down to 2, from the same start vector; then ``ArpackNoConvergence`` carries the pairs that pass
    the residual test and lie inside the widest certified window of the last attempt.  Nothing uncertified is returned.

    Returns ``(theta, info)``; ``info``: ``"steps"`` (Gram-Schmidt steps), ``"matvecs"`` (products with ``A``), both over stage 0 and all
    attempts, ``"filter"`` (``requested``, ``degree``, ``lo``, ``hi``, ``sigma``, ``attempts``) and ``trl``'s counts of the last attempt."""
    check_args(n, k, "LM", None)
    degree, sigma = _check_degree(degree), float(sigma)
    extra = max(4, k // 4)

    def sizes(extra):  # kb and ncv of an attempt with this many extra pairs
        kb = k + extra if ncv is not None else min(k + extra, min(n, _MAX_NCV) - 3)
        return kb, check_args(n, kb, "LA", min(n, _MAX_NCV, max(2 * kb + 1, 20)) if ncv is None else ncv)

    kb, m = sizes(extra)
    rng, tol_eff, v0 = _start(n, tol, v0, rng)
    _, _, _, (lo, hi) = _stage0(backend, m, v0)
    if not lo <= sigma <= hi:
        raise ValueError(f"sigma={sigma!r} lies outside the spectrum (bounds {lo!r} .. {hi!r}): the eigenvalues nearest to it are an "
                         "end of the spectrum, use which='SA' or which='LA'")
    anorm = max(abs(lo), abs(hi))
    res_bound = 1e3 * tol_eff * _RANGE_CAP * anorm
    tol_b = max(float(tol), 4 * _EPS)  # B's own products are rounded at several eps |B|: residual estimates of B stall below that
    tie = 1e-10 * anorm  # values this close in distance count as equally near: either copy of such a pair is a right answer
    steps, matvecs = m, m
    attempts = []
    d = degree
    while True:
        filt = SeriesFilter(lo, hi, sigma, d)
        backend.begin(m, v0)  # (a basis of another size drops the device's series: size it before the series is set; trl begins again)
        backend.set_series(filt.coefficients(), filt.c, filt.e)
        att = {"degree": d, "pairs": kb, "steps": 0, "converged": False, "certified": False, "residuals_ok": False}
        attempts.append(att)
        try:
            thB, run = trl(backend, n, kb, "LA", ncv=m, maxiter=maxiter, tol=tol_b, v0=v0, probe=probe, rng=rng)
            att["converged"] = True
        except ArpackNoConvergence as err:  # its pairs are those of B: what they certify for A is all this attempt can give
            thB, run = np.asarray(err.eigenvalues), err.info
        kc = len(thB)
        backend.set_series(None)
        att["steps"] = run["matvecs"]  # (trl counts its steps there: the loop's operator is one product to it)
        steps += att["steps"]
        matvecs += att["steps"] * d + kc
        theta, ok = np.zeros(0), np.zeros(0, dtype=bool)
        if kc:
            att["p_min"] = p_min = float(np.min(thB))
            margin = 1e3 * tol_b * float(np.abs(thB).max())

            def pick(lam):  # the values nearest sigma that the attempt certifies, as ascending indices
                near = np.argsort(np.abs(lam - sigma), kind="stable")
                dist = np.abs(lam - sigma)[near]

                def certified(j):  # is p above p_min on the whole window of the j nearest values found?
                    r = dist[j - 1] - tie
                    return r < 0 or filt.window_min(max(lo, sigma - r), min(hi, sigma + r), 16 * d + 64) > p_min + margin

                if not _certify:
                    nsel, att["certified"] = min(k, kc), kc >= k
                elif att["converged"] and certified(k):
                    nsel, att["certified"] = k, True
                elif att["converged"]:  # the most of the nearest values found that a window certifies
                    nsel = next((j for j in range(k - 1, 0, -1) if certified(j)), 0)
                else:  # trl gave up: its converged pairs need not be the top of B without a gap, so p_min bounds nothing
                    nsel = 0
                return np.sort(near[:nsel])

            theta, res = _ritz_in_A(backend, m, kc, pick)
            if len(theta):
                ok = res <= res_bound
                att["residuals_ok"] = bool(ok.all())
        if att["certified"] and att["residuals_ok"]:
            break
        if d == 2:
            err = ArpackNoConvergence(f"No convergence ({int(ok.sum())}/{k} eigenvectors are certified nearest to sigma and pass the residual "
                                      f"test after {len(attempts)} attempts)", theta[ok], backend.get_vectors(len(theta))[:, ok] if len(theta) else np.zeros((n, 0)))
            err.info = {"steps": steps, "matvecs": matvecs,
                        "filter": {"requested": degree, "degree": d, "lo": lo, "hi": hi, "sigma": sigma, "attempts": attempts}}
            raise err
        # a lobe narrower than the wanted set, or a degenerate cluster cut by the kb-th pair: half the degree and twice the spare pairs
        d = max(2, d // 2)
        extra *= 2
        kb, m = sizes(extra)
    info = dict(run)
    info["steps"] = steps
    info["matvecs"] = matvecs
    info["anorm"] = anorm
    info["filter"] = {"requested": degree, "degree": d, "lo": lo, "hi": hi, "sigma": sigma, "attempts": attempts}
    return theta, info


class DeviceBackend:
    """The ``lz_trl_*`` calls - ``lz_ztrl_*`` with ``is_complex`` - on one ``_capi.Handle`` that already holds the matrix.  The band,
    the polynomials and ``rayleigh`` exist for a real matrix only (on a complex one the handle answers that no matrix is set)."""

    def __init__(self, handle, n, force_second_pass=False, block_size=None, is_complex=False):
        self.h = handle
        self.n = n
        self.block_size = block_size
        self.is_complex = is_complex
        self._prefix = "ztrl_" if is_complex else "trl_"  # of begin, extend, restart, probe, get_vectors and residuals
        if force_second_pass:
            from ._capi import FLAG_TRL_PASS2_ALWAYS

            handle.set_options(FLAG_TRL_PASS2_ALWAYS)

    def _call(self, name, *args):
        return getattr(self.h, self._prefix + name)(*args)

    def begin(self, m, v0):
        self._call("begin", m, v0)

    def extend(self, k, m):
        return self._call("extend", k, m)

    def begin_band(self, m, X):
        self.h.trl_begin_band(m, X)

    def extend_band(self, k, m):
        return self.h.trl_extend_band(k, m)

    def restart(self, m, kk, S):
        self._call("restart", m, kk, S)

    def probe(self, k, x):
        self._call("probe", k, x)

    def get_vectors(self, k):
        return self._call("get_vectors", k)

    def residuals(self, k, theta):
        return self._call("residuals", k, theta)

    def set_filter(self, coefficients, c=0.0):
        self.h.trl_set_filter(coefficients, c)

    def set_series(self, coefficients, c=0.0, e=1.0):
        self.h.trl_set_series(coefficients, c, e)

    def rayleigh(self, k):
        return self.h.trl_rayleigh(k)


def is_complex_matrix(A):
    """does ``A`` (SciPy sparse or ndarray) have a complex dtype?  That alone sends ``eigsh`` down the complex path."""
    return np.dtype(getattr(A, "dtype", np.float64)).kind == "c"


def upload_complex_matrix(h, A):
    """complex ``A`` (SciPy sparse of any format or a dense ndarray; complex64 is converted) -> the handle; returns n.  Dense input that
    is not C-contiguous is copied: the memory of an F-ordered Hermitian array, read by rows, is the conjugate."""
    if scipy.sparse.issparse(A):
        A = A.tocsr().astype(np.complex128, copy=False)
        if A.nnz >= 2**31 or A.shape[0] >= 2**31:
            raise ValueError("matrix too large for int32 CSR indices")
        h.set_csr_cplx(A.shape[0], A.indptr, A.indices, A.data)
    else:
        h.set_dense_cplx(np.ascontiguousarray(A, dtype=np.complex128))
    return int(A.shape[0])


def upload_matrix(h, A):
    """A (SciPy sparse of any format, dense ndarray, ``synthetic.CSR`` or ``StencilOperator``) -> the handle; returns n."""
    if hasattr(A, "dims") and hasattr(A, "points"):  # StencilOperator: assembled on the device, as LanczosBase._upload_matrix does
        h.build_stencil3d_block(A.dims, A.points, A.T_factor, A.weights4, 0, A.shape[0], (), potential=A.potential,
                                potential_params=A.potential_params, negate_T=A.negate_T)
        return int(A.shape[0])
    from ._solver import _pack_matrix

    if scipy.sparse.issparse(A) and A.shape[0] != A.shape[1]:
        raise ValueError(f"expected square matrix (shape={A.shape})")
    packed = _pack_matrix(A)
    if packed[0] == "csr":
        n = len(packed[1]) - 1
        h.set_csr(n, 0, packed[1], packed[2], packed[3])
    else:
        n = packed[1].shape[0]
        h.set_dense(packed[1])
    return int(n)


def eigsh(A, k=6, M=None, sigma=None, which="LM", v0=None, ncv=None, maxiter=None, tol=0, return_eigenvectors=True, Minv=None,
          OPinv=None, mode="normal", device_id=0, handle=None, info=None, filter_degree=None, block_size=None):
    """Find ``k`` eigenvalues and eigenvectors of the real symmetric or complex Hermitian matrix ``A`` -
    ``scipy.sparse.linalg.eigsh``'s signature and defaults, solved by thick-restart Lanczos on the GPU.

    Complex ``A`` (a SciPy sparse matrix or a dense ndarray of a complex dtype; complex64 is converted; Hermitian-ness is assumed, not
    checked, as SciPy does): the same loop on the complex kernels (``lz_ztrl_*``).  Eigenvalues come back ascending as float64,
    eigenvectors as ``(n, k)`` complex128; ``v0`` may be real or complex; ``k + 3 <= ncv <= min(n, 64)``, and a default ``ncv`` above 64
    raises ``ValueError``; ``filter_degree``, ``sigma`` and ``block_size`` raise ``NotImplementedError``.  Everything else below holds.

    ``which``: ``"LM"``, ``"SM"``, ``"LA"`` or ``"SA"`` (``"BE"``, ``M``, ``Minv``, ``OPinv``, other modes and ``sigma`` without
    ``filter_degree`` raise ``NotImplementedError``).  ``ncv`` (default ``min(n, max(2k + 1, 20))``) must satisfy ``k + 3 <= ncv <= min(n, 128)``.
    ``A``: any SciPy sparse format, a dense ndarray, ``synthetic.CSR`` or ``StencilOperator`` (assembled on the device).
    Eigenvalues come back in ascending order.  Start and probe vectors come from a private seeded generator (NumPy's global
    RNG is never touched).  After ``maxiter`` restart cycles (default ``10 n``) ``ArpackNoConvergence`` carries the converged pairs.
    Convergence: ``beta |s_last| <= tol * max|theta|`` (machine epsilon for ``tol = 0``), see the module docstring for why this
    differs from ARPACK's ``tol * max(eps^(2/3), |theta|)``.
    ``handle``: an open ``_capi.Handle`` to run on (its matrix is replaced); ``info``: a dict that receives the run's counts.
    ``filter_degree`` (an integer >= 2, ``which`` ``"SA"`` or ``"LA"`` only; default None: no filter): run the loop on a Chebyshev
    polynomial of ``A`` of at most this degree (``trl_filtered``) - several times fewer Gram-Schmidt steps for somewhat more products
    with ``A``, which pays when a pass over the basis costs many products (long vectors, large ``ncv``, clustered wanted ends).
    ``sigma`` with ``which="LM"`` and ``filter_degree``: the ``k`` eigenvalues nearest ``sigma`` (SciPy's meaning, without a
    factorisation; ``sigma=0.0`` is the interior form of ``"SM"``), ascending, by Lanczos on a Chebyshev series of ``A`` that peaks at
    ``sigma`` (``trl_interior``); the result is certified complete or ``ArpackNoConvergence`` is raised.  ``ncv`` then counts against
    ``k + max(4, k // 4)`` pairs.
    ``block_size`` (an integer ``2 .. 8``; default None: the single-vector loop): band Lanczos with that many start vectors
    (``trl_band``) - every copy of an eigenvalue of multiplicity up to ``block_size`` is found without the probe's help, and the device
    orthogonalises ``block_size`` new vectors in one walk over the basis.  ``ncv`` (default ``min(n - b, 128, max(2k + 1, 20, k + 2b + 1))``)
    must then satisfy ``k + 2b + 1 <= ncv <= min(n - b, 128)``.  Combines with ``which`` and with ``filter_degree``; with ``sigma`` it
    raises ``NotImplementedError``."""
    from . import _capi

    n = int(A.shape[0])
    if len(A.shape) != 2 or A.shape[1] != n:
        raise ValueError(f"expected square matrix (shape={A.shape})")
    cplx = is_complex_matrix(A)
    interior = None
    if cplx:
        if filter_degree is not None:
            raise NotImplementedError("filter_degree with a complex matrix: the polynomial filter is built for the real basis only")
        if sigma is not None:
            raise NotImplementedError("sigma with a complex matrix: there is no shift-invert and no interior filter on the complex path")
        if block_size is not None:
            raise NotImplementedError("block_size with a complex matrix: the band form is built for the real basis only")
        check_args(n, k, which, ncv, M, sigma, Minv, OPinv, mode, complex_A=True)
    else:
        if block_size is not None:
            check_block_size(block_size)
            if sigma is not None:
                raise NotImplementedError("block_size with sigma: the interior mode's certificate is defined for the single-vector loop only")
        if M is None and Minv is None and OPinv is None:
            interior = check_interior_args(which, sigma, filter_degree)
        if interior is not None:
            check_args(n, k, which, None, M, None, Minv, OPinv, mode)  # (ncv is measured against the k + extra pairs of trl_interior)
        else:
            if block_size is None:
                check_args(n, k, which, ncv, M, sigma, Minv, OPinv, mode)
            else:
                check_band_args(n, k, which, ncv, block_size, M, sigma, Minv, OPinv, mode)
            if filter_degree is not None:
                check_filter_args(which, filter_degree)
    h = handle if handle is not None else _capi.Handle(device_id)
    try:
        (upload_complex_matrix if cplx else upload_matrix)(h, A)
        backend = DeviceBackend(h, n, block_size=block_size, is_complex=cplx)
        if interior is not None:
            theta, run = trl_interior(backend, n, k, interior[0], interior[1], ncv=ncv, maxiter=maxiter, tol=tol, v0=v0)
        elif filter_degree is None and block_size is None:
            theta, run = trl(backend, n, k, which=which, ncv=ncv, maxiter=maxiter, tol=tol, v0=v0)
        elif filter_degree is None:
            theta, run = trl_band(backend, n, k, which, block_size, ncv=ncv, maxiter=maxiter, tol=tol, v0=v0)
        else:
            theta, run = trl_filtered(backend, n, k, which, filter_degree, ncv=ncv, maxiter=maxiter, tol=tol, v0=v0, block_size=block_size)
        if info is not None:
            info.update(run)
            info["residuals"] = backend.residuals(k, theta)
        if not return_eigenvectors:
            return theta
        return theta, backend.get_vectors(k)
    finally:
        if handle is None:
            h.close()
