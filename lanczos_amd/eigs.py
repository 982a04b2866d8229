"""``eigs``: converged eigenpairs of a real non-symmetric matrix by Krylov-Schur on the GPU.

The device side is the thick-restart solver's (``lz_trl_*`` in include/lanczos_hip.h), unchanged: on a non-symmetric matrix
``lz_trl_extend`` is an Arnoldi step - ``w = A V[j]``, classical Gram-Schmidt against every row behind the DGKS gate, all measured
coefficients returned - and ``lz_trl_restart`` rotates the basis by any ``m x kk`` matrix.  The host keeps the ``(m + 1) x m`` projected
matrix ``H`` (``A V_m^T = V_{m+1}^T H``) and runs the outer loop below.  The one new device call is ``lz_trl_residuals_cplx``:
``|A x - lambda x|`` for complex ``lambda`` with ``x`` held as two real rows.

Krylov-Schur (Stewart, 2001) is what ``scipy.sparse.linalg.eigs`` does in another form (ARPACK's implicit restart with exact shifts):
after ``ncv`` steps ``H[:m] = Q R Q^T`` (real Schur form), the wanted 1x1 and 2x2 diagonal blocks of ``R`` are moved to the front
(LAPACK's ``dtrsen``), the basis is compressed in place to its first ``kk`` Schur vectors, the residual vector becomes row ``kk`` and
``H`` becomes ``R[:kk, :kk]`` over the spike row ``beta Q[m - 1, :kk]``.  The restart is on a real Schur form because a conjugate
pair cannot be split: ``kk`` never cuts a 2x2 block.

Total order.  Eigenvalues are ranked by an exact lexicographic sort on ``(primary key of which, -|lambda|, -Re lambda, -Im lambda)``
applied to the blocks of ``R`` (a pair is ranked by its positive-imaginary member, which comes first; an exact tie keeps ``R``'s
order).  Selection is by that rank and ``dtrsen``, never by a threshold: ``which="LI"`` on a real spectrum is one big tie, which the
secondary keys break as ``"LM"`` would.

Stopping rule.  The estimate of eigenpair ``(lambda, z)`` of ``R`` is ``|beta (Q[m - 1] z)| / |z|``; a pair is converged when it is
``<= tol_eff * max|theta|`` (``tol_eff = tol``, or machine epsilon when ``tol == 0``; ``max|theta|`` over the run), as in ``eigsh``.
The loop stops when every pair of the leading block (``k`` rows, ``k + 1`` when the ``k``-th value is half of a pair) has converged.

Breakdown.  A ``beta_j <= 10 eps scale (j + 1)`` (the band loop's bound) means the Krylov space is invariant: the loop goes on from a
fresh random vector orthogonal to the basis with a zero coupling.  There is no probe for copies of a degenerate eigenvalue and no
certificate for interior values: ``"SM"`` and ``"SI"`` are refused.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg
from scipy.linalg.lapack import dtrsen
from scipy.sparse.linalg import ArpackNoConvergence

from .eigsh import _EPS, _MAX_NCV, _SEED, DeviceBackend, NumpyBackend, _start, upload_matrix

_WHICH = ("LM", "LR", "SR", "LI")
_REFUSED = ("SM", "SI")


def _key(lam, which):
    """the sort key of one eigenvalue under the total order: ascending keys, most wanted first"""
    primary = {"LM": -abs(lam), "LR": -lam.real, "SR": lam.real, "LI": -abs(lam.imag)}[which]
    return (primary, -abs(lam), -lam.real, -lam.imag)


def total_order(lam, which):
    """indices of the eigenvalues ``lam``, most wanted first.  Exact conjugates are adjacent, the positive-imaginary member first,
    unless another eigenvalue equals one of them bit for bit."""
    lam = np.asarray(lam, dtype=np.complex128)
    return np.array(sorted(range(len(lam)), key=lambda i: _key(lam[i], which) + (i,)), dtype=np.int64)


def _blocks(R):
    """the diagonal blocks of the quasi-triangular ``R`` as ``[(start, size, lambda)]``; a 2x2 block carries its positive-imaginary
    eigenvalue (a 2x2 block with real eigenvalues, which a standardised Schur form does not have, is read as two 1x1 blocks)"""
    out = []
    m = len(R)
    i = 0
    while i < m:
        if i + 1 < m and R[i + 1, i] != 0.0:
            a, b, c, d = R[i, i], R[i, i + 1], R[i + 1, i], R[i + 1, i + 1]
            disc = (a - d) * (a - d) / 4 + b * c
            if disc < 0:
                out.append((i, 2, complex((a + d) / 2, np.sqrt(-disc))))
                i += 2
                continue
        out.append((i, 1, complex(R[i, i], 0.0)))
        i += 1
    return out


def _front(R, Q, blocks, chosen):
    """``(R, Q)`` with the blocks ``chosen`` (indices into ``blocks``) moved to the front by ``dtrsen``, their order in ``R`` kept"""
    select = np.zeros(len(R), dtype=np.int32)
    for b in chosen:
        select[blocks[b][0]: blocks[b][0] + blocks[b][1]] = 1
    out = dtrsen(select, R, Q, job="N", wantq=1)
    if out[-1] != 0:
        raise RuntimeError(f"eigs: dtrsen could not reorder the Schur form (info={out[-1]})")
    return out[0], out[1]


def _rank(blocks, which):
    """indices of ``blocks``, most wanted first"""
    return sorted(range(len(blocks)), key=lambda b: _key(blocks[b][2], which) + (b,))


def _take(blocks, ranked, count):
    """the leading entries of ``ranked`` that hold at least ``count`` rows, and how many rows that is (``count``, or ``count + 1`` when
    the last block taken is a pair)"""
    chosen, rows = [], 0
    for b in ranked:
        if rows >= count:
            break
        chosen.append(b)
        rows += blocks[b][1]
    return chosen, rows


def _leading_pairs(R, kq, q_last, b_last):
    """The eigenpairs of ``R[:kq, :kq]`` as items ``(lambda, z, estimate)``, one per real eigenvalue and one per conjugate pair (its
    positive-imaginary member); ``z`` has unit norm and ``estimate = |b_last (q_last[:kq] z)|``."""
    lam, Z = np.linalg.eig(R[:kq, :kq])
    lam, Z = np.asarray(lam, dtype=np.complex128), np.asarray(Z, dtype=np.complex128)
    items = []
    for i in range(kq):
        if lam[i].imag < 0:
            continue
        z = Z[:, i] / np.linalg.norm(Z[:, i])
        if lam[i].imag == 0:
            z = z.real / np.linalg.norm(z.real)
        items.append((complex(lam[i]), z, abs(b_last * np.dot(q_last[:kq], z))))
    return items


def _real_form(items):
    """``(W, lam)``: the eigenvectors of ``items`` in real form - one column ``z`` for a real eigenvalue, two adjacent columns
    ``Re z``, ``Im z`` for a pair - and the eigenvalue of every column (the pair's: positive-imaginary, then its conjugate)"""
    cols, lam = [], []
    for l, z, _ in items:
        if l.imag == 0:
            cols.append(z.real)
            lam.append(l)
        else:
            cols += [z.real, z.imag]
            lam += [l, l.conjugate()]
    return np.ascontiguousarray(np.array(cols).T), np.array(lam, dtype=np.complex128)


def _complex_vectors(rows, lam):
    """``(n, len(lam))`` complex eigenvectors from basis rows in real form (``rows``: ``(n, len(lam))``)"""
    X = np.zeros(rows.shape, dtype=np.complex128)
    i = 0
    while i < len(lam):
        if lam[i].imag == 0:
            X[:, i] = rows[:, i]
            i += 1
        else:
            X[:, i] = rows[:, i] + 1j * rows[:, i + 1]
            X[:, i + 1] = rows[:, i] - 1j * rows[:, i + 1]
            i += 2
    return X


def check_args(n, k, which, ncv, M=None, sigma=None, Minv=None, OPinv=None, OPpart=None):
    """SciPy's argument errors, plus this solver's own limits.  Returns ncv."""
    if M is not None or sigma is not None or Minv is not None or OPinv is not None or OPpart is not None:
        raise NotImplementedError("eigs on the device solves the standard problem only: M, sigma, Minv, OPinv and OPpart must be None")
    if which in _REFUSED:
        raise NotImplementedError(f"which={which!r} is not implemented: a plain Krylov space misconverges on interior eigenvalues and "
                                  "there is no certificate for the non-symmetric case")
    if which not in _WHICH:
        raise ValueError(f"which must be one of {' '.join(_WHICH + _REFUSED)}")
    if k <= 0:
        raise ValueError(f"k={k} must be greater than 0.")
    if k >= n - 1:
        raise TypeError(f"k >= N - 1 for an N x N matrix (k={k}, N={n}): reduce k")
    if ncv is None:
        ncv = min(n, max(2 * k + 1, 20))
    ncv = int(ncv)
    if not k + 3 <= ncv <= min(n, _MAX_NCV):
        raise ValueError(f"ncv must be k+3<=ncv<=min(n, {_MAX_NCV}), ncv={ncv} (stricter than SciPy's k+1<ncv<=n: the restart keeps a "
                         "conjugate pair whole and two spare basis rows)")
    return ncv


class NumpyCplxBackend(NumpyBackend):
    """``NumpyBackend`` with the complex residuals of ``lz_trl_residuals_cplx``: what the host tests drive ``krylov_schur`` with"""

    def residuals_cplx(self, k, re, im):
        re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
        out = np.zeros(k)
        i = 0
        while i < k:
            if im[i] == 0:
                out[i] = np.linalg.norm(self.A @ self.V[i] - re[i] * self.V[i])
                i += 1
                continue
            if not (im[i] > 0 and i + 1 < k and re[i + 1] == re[i] and im[i + 1] == -im[i]):
                raise ValueError("residuals_cplx: a positive im[i] needs its conjugate at i + 1")
            xr, xi = self.V[i], self.V[i + 1]
            tr = self.A @ xr - re[i] * xr + im[i] * xi
            ti = self.A @ xi - im[i] * xr - re[i] * xi
            out[i] = out[i + 1] = np.sqrt(np.dot(tr, tr) + np.dot(ti, ti))
            i += 2
        return out


class DeviceCplxBackend(DeviceBackend):
    """``DeviceBackend`` with ``lz_trl_residuals_cplx``"""

    def residuals_cplx(self, k, re, im):
        return self.h.trl_residuals_cplx(k, re, im)


def krylov_schur(backend, n, k, which="LM", ncv=None, maxiter=None, tol=0.0, v0=None, rng=None):
    """The Krylov-Schur outer loop over a backend with ``begin``, ``extend``, ``restart``, ``probe`` and ``get_vectors``.

    Returns ``(lam, info)``: ``lam`` (``kq`` complex values, ``kq = k`` or ``k + 1``) are the eigenvalues of basis rows ``0 .. kq - 1``,
    which hold the eigenvectors in real form - a real eigenvalue's row is its vector, a pair's two adjacent rows are ``Re x`` and
    ``Im x`` of the positive-imaginary member, listed first.  ``info``: ``{"matvecs", "cycles", "breakdowns", "anorm"}``.  Raises
    ``ArpackNoConvergence`` after ``maxiter`` cycles with the converged wanted pairs (a half-converged pair counts as not converged)."""
    m = check_args(n, k, which, ncv)
    maxiter = n * 10 if maxiter is None else int(maxiter)
    rng, tol_eff, v0 = _start(n, tol, v0, rng)
    backend.begin(m, v0)
    backend.set_filter(None)  # the loop multiplies by A itself
    H = np.zeros((m + 1, m))
    kcur = 0
    anorm = 0.0
    info = {"matvecs": 0, "cycles": 0, "breakdowns": 0}
    while True:
        j0 = kcur
        while True:  # one extension of the basis to m rows; a breakdown restarts it behind the invariant subspace
            proj, beta = backend.extend(j0, m)
            info["matvecs"] += m - j0
            # the device went on without a synchronisation behind a breakdown: nothing from there on may enter H or the scale
            scale = max(anorm, np.abs(H[:, :j0]).max()) if j0 else anorm
            jb = None
            for j in range(j0, m):
                H[:, j] = 0.0
                H[: j + 1, j] = proj[j, : j + 1]
                scale = max(scale, np.abs(H[: j + 1, j]).max())
                if not beta[j] > 10 * _EPS * scale * (j + 1):
                    jb = j
                    break
                H[j + 1, j] = beta[j]
            if jb is None or jb == m - 1:
                break
            info["breakdowns"] += 1
            H[:, jb + 1:] = 0.0
            backend.probe(jb + 1, rng.standard_normal(n))
            j0 = jb + 1
        info["cycles"] += 1
        dead = jb is not None  # the last residual vanished: the Krylov space is exhausted and V[m] is noise
        b_last = 0.0 if dead else beta[m - 1]
        R, Q = scipy.linalg.schur(H[:m], output="real")
        blocks = _blocks(R)
        anorm = max(anorm, max(abs(b[2]) for b in blocks))
        chosen, kq = _take(blocks, _rank(blocks, which), k)
        R, Q = _front(R, Q, blocks, chosen)
        items = _leading_pairs(R, kq, Q[m - 1], b_last)
        ok = [it[2] <= tol_eff * anorm for it in items]
        if all(ok):
            W, lam = _real_form(items)
            backend.restart(m, kq, np.ascontiguousarray(Q[:, :kq] @ W))
            info["anorm"] = anorm
            return lam, info
        if info["cycles"] >= maxiter:
            conv = [it for it, good in zip(items, ok) if good]
            conv = [conv[i] for i in total_order([it[0] for it in conv], which)]
            lam, vecs = np.zeros(0, dtype=np.complex128), np.zeros((n, 0), dtype=np.complex128)
            if conv:
                W, lam = _real_form(conv)
                backend.restart(m, len(lam), np.ascontiguousarray(Q[:, :kq] @ W))
                vecs = _complex_vectors(backend.get_vectors(len(lam)), lam)  # (at most k columns: one item of the block is missing)
            err = ArpackNoConvergence(f"No convergence ({info['cycles']} iterations, {len(lam)}/{k} eigenvectors converged)", lam, vecs)
            info["anorm"] = anorm
            err.info = info  # the counts of the run that gave up
            raise err
        nconv = sum(1 if it[0].imag == 0 else 2 for it, good in zip(items, ok) if good)
        blocks = _blocks(R)  # (the leading kq rows are the wanted blocks; the rest are ranked again)
        lead = [b for b in range(len(blocks)) if blocks[b][0] < kq]
        rest = [b for b in _rank(blocks, which) if blocks[b][0] >= kq]
        extra, kk = _take(blocks, rest, min(m - 3, k + max(nconv, (m - k) // 2)) - kq)
        kk += kq
        R, Q = _front(R, Q, blocks, lead + extra)
        backend.restart(m, kk, np.ascontiguousarray(Q[:, :kk]))
        H[:] = 0.0
        H[:kk, :kk] = R[:kk, :kk]
        if dead:
            backend.probe(kk, rng.standard_normal(n))
        else:
            H[kk, :kk] = b_last * Q[m - 1, :kk]
        kcur = kk


def _eigs(backend, n, k, which, ncv, maxiter, tol, v0, return_eigenvectors, info):
    lam, run = krylov_schur(backend, n, k, which, ncv=ncv, maxiter=maxiter, tol=tol, v0=v0)
    sel = total_order(lam, which)[:k]  # most wanted first; a split pair gives its positive-imaginary member
    if info is not None:
        info.update(run)
        info["residuals"] = np.asarray(backend.residuals_cplx(len(lam), lam.real.copy(), lam.imag.copy()))[sel]
    if not return_eigenvectors:
        return lam[sel]
    return lam[sel], _complex_vectors(backend.get_vectors(len(lam)), lam)[:, sel]


def eigs(A, k=6, M=None, sigma=None, which="LM", v0=None, ncv=None, maxiter=None, tol=0, return_eigenvectors=True, Minv=None, OPinv=None,
         OPpart=None, device_id=0, handle=None, info=None):
    """Find ``k`` eigenvalues and eigenvectors of the real square matrix ``A`` - ``scipy.sparse.linalg.eigs``'s signature and defaults,
    solved by Krylov-Schur on the GPU (see the module docstring).

    ``A``: any SciPy sparse format, a dense ndarray, ``synthetic.CSR`` or ``StencilOperator`` (assembled on the device); complex input
    raises ``NotImplementedError``, as do ``M``, ``sigma``, ``Minv``, ``OPinv`` and ``OPpart``.
    ``which``: ``"LM"``, ``"LR"``, ``"SR"`` or ``"LI"`` (largest ``|Im lambda|``: ARPACK's meaning for a real matrix); ``"SM"`` and
    ``"SI"`` raise ``NotImplementedError``, anything else ``ValueError``.  ``k >= n - 1`` raises ``TypeError`` as SciPy does.
    ``ncv`` (default ``min(n, max(2k + 1, 20))``) must satisfy ``k + 3 <= ncv <= min(n, 128)``.
    Returns ``(w, X)`` - ``w`` ``complex128`` of length ``k``, ``X`` ``(n, k)`` ``complex128`` with unit 2-norm columns - or ``w``
    alone with ``return_eigenvectors=False``, most wanted first under the module's total order; when ``k`` splits a conjugate pair the
    positive-imaginary member is returned.  Start and breakdown vectors come from a private seeded generator (NumPy's global RNG is
    never touched).  After ``maxiter`` restart cycles (default ``10 n``) ``ArpackNoConvergence`` carries the converged pairs.
    ``handle``: an open ``_capi.Handle`` to run on (its matrix is replaced); ``info``: a dict that receives ``matvecs``, ``cycles``,
    ``breakdowns``, ``anorm`` and ``residuals`` (``k`` values of ``|A x - lambda x|`` measured on the device)."""
    from . import _capi

    if len(A.shape) != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"expected square matrix (shape={A.shape})")
    n = int(A.shape[0])
    dtype = getattr(A, "dtype", None)
    if (dtype is not None and np.dtype(dtype).kind == "c") or (v0 is not None and np.iscomplexobj(v0)):
        raise NotImplementedError("eigs on the device takes a real matrix and a real v0: complex input is not implemented")
    check_args(n, k, which, ncv, M, sigma, Minv, OPinv, OPpart)
    h = handle if handle is not None else _capi.Handle(device_id)
    try:
        upload_matrix(h, A)
        return _eigs(DeviceCplxBackend(h, n), n, k, which, ncv, maxiter, tol, v0, return_eigenvectors, info)
    finally:
        if handle is None:
            h.close()
