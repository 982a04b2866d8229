"""``cg``: solve ``A x = b`` for a real symmetric positive definite ``A`` on the GPU, with an optional diagonal preconditioner.

Conjugate gradients (Hestenes & Stiefel 1952) keeps four vectors (``x``, ``r``, ``p``, ``q``) and needs one product and two
reductions per iteration.  The loop is ``scipy.sparse.linalg.cg``'s, scalar for scalar.  With ``atol_eff = max(atol, rtol |b|)``,
``r = b - A x0`` and ``z = M r`` (``M`` diagonal: ``z = d o r``; no ``M``: ``z = r``), iteration ``k = 0, 1, ...`` is

    |r| < atol_eff -> 0                                                                           (the head test)
    rho = r . z;   p = z + (rho / rho_prev) p                                                      (k = 0: p = z)
    q = A p;   alpha = rho / (p . q);   x += alpha p;   r -= alpha q;   rho_prev = rho;   callback(x)

Four deliberate deviations from SciPy.  The head test of iteration ``k + 1`` runs at the end of iteration ``k``, so when the last
permitted iteration ends with ``|r| < atol_eff`` the answer is 0 (SciPy tests only at the head of the next iteration and reports
``maxiter``).  A ``p . q`` that is zero, or an ``alpha`` or ``rho`` that is not finite, ends the solve with code -1 (``"breakdown"``)
where SciPy divides and carries on with NaNs.  A ``p . q <= 0`` does not stop the solve - SciPy carries on and CG sometimes survives
- but the first iteration at which it happened is recorded in ``info["indefinite_at"]``.  ``callback(xk)`` is honoured by running one
iteration per synchronisation.

On the device (``lz_cg_*`` in include/lanczos_hip.h) the scalars never leave it inside a chunk of
``check_every`` iterations: one-block kernels form ``alpha``, ``rho`` and ``beta`` and set a flag that gates the rest of the chunk.
``solve`` below is the host loop over chunks; it runs on ``DeviceCgBackend`` and on ``NumpyCgBackend``, a host restatement of the same
calls, which the host tests drive.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse

from .bicgstab import check_bicgstab_args
from .eigsh import upload_matrix
from .expm import _as_operator, _entry00


class NumpyCgBackend:
    """The calls of ``DeviceCgBackend`` in NumPy - ``begin`` / ``set_state`` leave the head test to the first ``run``, which knows
    ``atol_eff``, and ``run`` applies the head test of the next iteration at the end of each - : what the host tests drive ``solve``
    with.  ``dot``: the inner product (the tests' reference runs pass other summation orders)."""

    launches_per_iteration = None

    def __init__(self, A, dot=None):
        self.A = _as_operator(A)
        self.n = self.A.shape[0]
        self.dot = dot if dot is not None else (lambda a, b: float(a @ b))

    def _z(self):
        return self.r if self.d is None else self.d * self.r

    def _fresh(self, k, x, r, p, d, rho):
        self.x, self.r, self.d = x, r, d
        self.p = self._z().copy() if p is None else p
        self.q = np.zeros(self.n)
        self.rho = self.dot(self.r, self._z()) if rho is None else float(rho)
        self.rho_prev, self.alpha, self.beta, self.pq = 0.0, 0.0, 0.0, 0.0
        self.rnorm = float(np.sqrt(self.dot(self.r, self.r)))
        self.steps, self.done, self.code, self.exit, self.head, self.fresh = int(k), False, 0, None, False, True
        self.indefinite_at = None
        self.hist = {}

    def begin(self, b, x0, d=None):
        b = np.asarray(b, dtype=np.float64)
        x = np.zeros(self.n) if x0 is None else np.array(x0, dtype=np.float64)
        r = b.copy() if x0 is None else b - self.A @ x
        self._fresh(0, x, r, None, None if d is None else np.array(d, dtype=np.float64), None)

    def set_state(self, k, x, r, p, d, scalars):
        x, r, p = (np.array(a, dtype=np.float64) for a in (x, r, p))
        self._fresh(k, x, r, p, None if d is None else np.array(d, dtype=np.float64), scalars[0])

    def _head(self, atol):
        """the head test of iteration ``steps`` -> may the iteration run?"""
        self.hist[self.steps] = self.rnorm
        if self.rnorm < atol:
            self.done, self.code, self.exit, self.head = True, 0, "converged", True
        elif not np.isfinite(self.rho):
            self.done, self.code, self.exit, self.head = True, -1, "breakdown", True
        return not self.done

    def run(self, iters, atol):
        with np.errstate(all="ignore"):  # (a breakdown divides by a vanished p . q, as the device does)
            if self.fresh:
                self.fresh = False
                self._head(atol)
            for _ in range(int(iters)):
                if self.done:
                    break
                self.q = np.asarray(self.A @ self.p)
                self.pq = self.dot(self.p, self.q)
                alpha = float(np.float64(self.rho) / np.float64(self.pq))
                if self.pq == 0.0 or not np.isfinite(alpha):
                    self.done, self.code, self.exit, self.head = True, -1, "breakdown", False
                    break
                self.alpha = alpha
                if self.pq <= 0.0 and self.indefinite_at is None:
                    self.indefinite_at = self.steps
                self.r = self.r - self.alpha * self.q
                z = self._z()
                self.rho_prev, self.rho = self.rho, self.dot(self.r, z)
                self.rnorm = float(np.sqrt(self.dot(self.r, self.r)))
                self.steps += 1
                self.x = self.x + self.alpha * self.p  # (the exit iteration's update included)
                if self._head(atol):
                    self.beta = float(np.float64(self.rho) / np.float64(self.rho_prev))
                    self.p = z + self.beta * self.p
        return self._state()

    def _state(self):
        return {"iterations": self.steps, "done": bool(self.done), "code": self.code, "exit": self.exit, "head": self.head,
                "rnorm": self.rnorm, "rho": self.rho, "rho_prev": self.rho_prev, "alpha": self.alpha, "beta": self.beta, "pq": self.pq,
                "indefinite_at": self.indefinite_at}

    def history(self, count):
        return np.array([self.hist.get(i, 0.0) for i in range(int(count))], dtype=np.float64)

    def solution(self):
        return self.x.copy()

    def get(self, which):
        return getattr(self, which).copy()


class DeviceCgBackend:
    """The ``lz_cg_*`` calls on one ``_capi.Handle`` that already holds the matrix."""

    def __init__(self, handle, n):
        self.h = handle
        self.n = n
        self.launches_per_iteration = handle.cg_info()["launches_per_iteration"]

    def begin(self, b, x0, d=None):
        self.h.cg_begin(b, x0, d)

    def set_state(self, k, x, r, p, d, scalars):
        self.h.cg_set_state(k, x, r, p, d, scalars)

    def run(self, iters, atol):
        return self.h.cg_run(iters, atol)

    def history(self, count):
        return self.h.cg_history(count)

    def solution(self):
        return self.h.cg_get("x")

    def get(self, which):
        return self.h.cg_get(which)


def finish(backend, st, maxiter, first=0, extra_products=0, chunks=0, atol_eff=0.0, d=None, info=None):
    """``(x, info_int)`` of a backend whose last ``run`` returned ``st``, and the run's counts into ``info``.  A breakdown that a head
    test found after the last permitted iteration is SciPy's ``maxiter``: it never enters the iteration that would have divided."""
    done, code, kind = st["done"], st["code"], st["exit"]
    ran = st["iterations"] - first
    if done and st["head"] and code < 0 and ran >= maxiter:
        done = False
    if not done:
        code, kind = int(maxiter), "maxiter"
    products = ran + (1 if kind == "breakdown" and not st["head"] else 0) + extra_products
    x = backend.solution()
    if info is not None:
        info.update({"iterations": ran, "code": int(code), "exit": kind, "residual_norm": st["rnorm"], "atol_effective": float(atol_eff),
                     "products": int(products), "chunks": chunks, "launches_per_iteration": backend.launches_per_iteration,
                     "preconditioner": None if d is None else "diagonal", "indefinite_at": st["indefinite_at"],
                     "history": backend.history(st["iterations"] + 1)[first:]})
    return x, int(code)


def solve(backend, b, x0, atol_eff, maxiter, check_every, callback=None, info=None, d=None, begun=False):
    """The loop over chunks on a backend (``NumpyCgBackend`` or ``DeviceCgBackend``) -> ``(x, info_int)``.  With a ``callback`` a chunk
    is one iteration and ``x`` is fetched behind each.  ``begun``: the backend holds a state already (``set_state``), which ``maxiter``
    more iterations continue."""
    if not begun:
        backend.begin(b, x0, d)
    chunk = 1 if callback is not None else int(check_every)
    st = backend.run(0, atol_eff)
    first = st["iterations"]
    chunks = 0
    while not st["done"] and st["iterations"] - first < maxiter:
        before = st["iterations"]
        st = backend.run(min(chunk, maxiter - (st["iterations"] - first)), atol_eff)
        chunks += 1
        if callback is not None and st["iterations"] > before:
            callback(backend.solution())
    return finish(backend, st, maxiter, first, 0 if (begun or x0 is None) else 1, chunks, atol_eff, d, info)


_ONLY_DIAGONAL = ("cg: only diagonal preconditioners are built (M: a diagonal SciPy sparse matrix, a diagonal dense array or "
                  "\"jacobi\")")


def _host_diagonal(A):
    if scipy.sparse.issparse(A):
        return np.asarray(A.diagonal(), dtype=np.float64)
    if isinstance(A, np.ndarray):
        return np.array(np.diagonal(A), dtype=np.float64)
    raise NotImplementedError("cg: M=\"jacobi\" needs a SciPy sparse or dense A (synthetic.CSR and StencilOperator have no host diagonal)")


def preconditioner_diagonal(A, M, n):
    """``d`` (``(n,)`` float64, finite and positive) of a diagonal ``M``, ``1 / A.diagonal()`` for ``"jacobi"``, None for None; every
    other ``M`` is the error the docstring of ``cg`` names"""
    if M is None:
        return None
    if isinstance(M, str):
        if M != "jacobi":
            raise ValueError(f"cg: unknown preconditioner {M!r} (the only named one is \"jacobi\")")
        with np.errstate(all="ignore"):
            d = 1.0 / _host_diagonal(A)
    elif scipy.sparse.issparse(M):
        if M.shape != (n, n):
            raise ValueError(f"shapes of A {(n, n)} and M {M.shape} are incompatible")
        if np.dtype(M.dtype).kind == "c":
            raise NotImplementedError("cg: complex M is not implemented")
        C = M.tocoo()
        if np.any(C.data[C.row != C.col] != 0):
            raise NotImplementedError(_ONLY_DIAGONAL)
        d = np.asarray(M.diagonal(), dtype=np.float64)
    elif isinstance(M, np.ndarray):
        if M.shape != (n, n):
            raise ValueError(f"shapes of A {(n, n)} and M {M.shape} are incompatible")
        if np.iscomplexobj(M):
            raise NotImplementedError("cg: complex M is not implemented")
        d = np.array(np.diagonal(M), dtype=np.float64)
        if np.count_nonzero(M) != np.count_nonzero(d):
            raise NotImplementedError(_ONLY_DIAGONAL)
    else:  # a LinearOperator, a callable, ...
        raise NotImplementedError(_ONLY_DIAGONAL)
    if d.shape != (n,) or not np.all(np.isfinite(d)) or not np.all(d > 0.0):
        raise ValueError("cg: the preconditioner's diagonal must be finite and strictly positive")
    return np.ascontiguousarray(d)


def check_cg_args(A, b, x0, M, maxiter, check_every, rtol, atol):
    """``(n, b as (n,) float64, x0 as (n,) float64 or None, maxiter, d as (n,) float64 or None)`` or the error of a bad call - before
    any device is asked for.  ``A``, ``b``, ``x0``, ``maxiter``, ``rtol`` and ``atol`` by ``check_bicgstab_args``."""
    try:
        n, b, x0, maxiter = check_bicgstab_args(A, b, x0, None, maxiter, check_every, rtol, atol)
    except NotImplementedError as e:
        raise NotImplementedError(str(e).replace("bicgstab:", "cg:")) from None
    return n, b, x0, maxiter, preconditioner_diagonal(A, M, n)


def cg(A, b, x0=None, *, rtol=1e-5, atol=0.0, maxiter=None, M=None, callback=None, check_every=8, device_id=0, handle=None, info=None,
       _backend=None):
    """Solve ``A x = b`` for a real symmetric positive definite ``A`` - ``scipy.sparse.linalg.cg``'s signature, defaults and loop - by
    conjugate gradients on the GPU.  Returns ``(x, info_int)``: ``x`` is ``(n,)`` float64; ``info_int`` is 0 on convergence,
    ``maxiter`` when the iterations ran out and -1 on a breakdown.

    ``A``: what ``minres`` takes - any SciPy sparse format, a dense ndarray, ``synthetic.CSR`` or ``StencilOperator``; real.  Symmetry
    and definiteness are assumed and not tested.  ``b``: ``(n,)`` or ``(n, 1)``, real.  ``b = 0`` returns zeros and 0, as SciPy does.
    ``x0``: the starting guess (an all-zero one is no guess: ``r = b`` without a product).  Convergence: ``|r| < max(atol, rtol |b|)``
    on the recurrence's residual, tested at the head of every iteration, as SciPy tests.  ``maxiter``: default ``10 n``.

    ``M``: the preconditioner, an approximation of the inverse of ``A``.  None; or a DIAGONAL matrix - a SciPy sparse matrix of any
    format or a dense ``(n, n)`` ndarray whose off-diagonal stored entries are all zero, such as ``scipy.sparse.diags(1 /
    A.diagonal())`` -, whose diagonal is taken on the host and must be finite and strictly positive (``ValueError`` otherwise, and for
    a wrong shape); or the string ``"jacobi"``: ``d = 1 / A.diagonal()`` of a SciPy sparse or dense ``A`` (``NotImplementedError`` for
    ``synthetic.CSR`` and ``StencilOperator``, which have no host diagonal).  Every other ``M`` - a matrix with an off-diagonal entry,
    a ``LinearOperator``, a callable - raises ``NotImplementedError``: only diagonal preconditioners are built.  On the device ``z =
    d o r`` is formed inside the two passes that run anyway and never stored: one more read each, no launch.

    Four deliberate deviations from SciPy.  When the last permitted iteration ends with ``|r| < atol_eff`` the answer is 0: SciPy
    tests only at the head of the next iteration and reports ``maxiter``.  A ``p . q`` that is zero, or an ``alpha`` or ``rho`` that is
    not finite, ends the solve with code -1 and ``info["exit"] = "breakdown"``: SciPy divides and carries on with NaNs.  A ``p . q <= 0``
    does NOT stop the solve - SciPy carries on and CG sometimes survives -; the first iteration at which it happened is recorded in
    ``info["indefinite_at"]`` (None otherwise).  ``callback(xk)`` is honoured by running ONE iteration per synchronisation and
    downloading ``x`` behind each, the slow path.

    Complex ``A`` / ``b`` / ``x0`` / ``M`` and a ``LinearOperator`` ``A`` raise ``NotImplementedError``; shape and value errors raise
    ``ValueError``; all of them before any device is asked for.  ``n == 1`` is answered on the host.
    ``check_every`` (default 8, the fastest of 8 / 32 / 128 measured, profiles/r31/cg_probe.json): iterations enqueued between two
    host synchronisations; past the exit the rest of a chunk is gated off on the device, but its products still run - up to
    ``check_every - 1`` wasted products.  ``x`` does not depend on it, bit for bit.
    ``handle``: an open ``_capi.Handle`` to run on (its square matrix is replaced); ``info``: a dict that receives ``iterations``,
    ``code``, ``exit`` (``"converged"``, ``"breakdown"`` or ``"maxiter"``), ``residual_norm`` (the recurrence's ``|r|`` at the last
    test), ``atol_effective``, ``products``, ``chunks``, ``launches_per_iteration``, ``preconditioner`` (None or ``"diagonal"``),
    ``indefinite_at`` and ``history`` (``|r|`` at every head test)."""
    n, b, x0, maxiter, d = check_cg_args(A, b, x0, M, maxiter, check_every, rtol, atol)
    bnorm = float(np.linalg.norm(b))
    atol_eff = max(float(atol), float(rtol) * bnorm)
    if x0 is not None and not np.any(x0):
        x0 = None
    run = {"iterations": 0, "code": 0, "exit": "converged", "residual_norm": 0.0, "atol_effective": atol_eff, "products": 0, "chunks": 0,
           "launches_per_iteration": None, "preconditioner": None if d is None else "diagonal", "indefinite_at": None,
           "history": np.zeros(0)}
    if bnorm == 0.0:
        x, code = np.zeros(n), 0
    elif n == 1:
        x, code = b / float(_entry00(A)), 0
        if callback is not None:
            callback(x.copy())
    elif _backend is not None:  # the host tests' way in: a NumpyCgBackend
        x, code = solve(_backend, b, x0, atol_eff, maxiter, check_every, callback, run, d)
    else:
        from . import _capi

        h = handle if handle is not None else _capi.Handle(device_id)
        try:
            upload_matrix(h, A)
            x, code = solve(DeviceCgBackend(h, n), b, x0, atol_eff, maxiter, check_every, callback, run, d)
        finally:
            if handle is None:
                h.close()
    if info is not None:
        info.update(run)
    return np.asarray(x, dtype=np.float64).reshape(n), code
