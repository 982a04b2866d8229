"""``bicgstab``: solve ``A x = b`` for a real square ``A``, symmetric or not, on the GPU.

BiCGSTAB (van der Vorst 1992) needs no basis and no product with the transpose: two products with ``A`` and a handful of vector
updates per iteration.  The loop is ``scipy.sparse.linalg.bicgstab``'s, scalar for scalar.  With ``atol_eff = max(atol, rtol |b|)``,
``rhotol = omegatol = eps^2``, ``r = b - A x0``, ``rtilde = r`` and ``rho = rtilde . r``, iteration ``k = 0, 1, ...`` is

    |r| < atol_eff -> 0;   |rho| < rhotol -> -10;   k > 0 and |omega| < omegatol -> -11          (the head tests, in this order)
    p = (p - omega v) beta + r,   beta = (rho / rho_prev)(alpha / omega)                           (k = 0: p = r)
    v = A p;   rv = rtilde . v;   rv == 0 -> -11;   alpha = rho / rv
    s = r - alpha v;   |s| < atol_eff -> x += alpha p, 0                                           (the half-step exit; the residual kept is s)
    t = A s;   omega = (t . s) / (t . t);   x = (x + alpha p) + omega s;   r = s - omega t;   rho_prev = rho;   rho = rtilde . r

Two deliberate deviations from SciPy: the head tests of iteration ``k + 1`` run at the end of iteration ``k``, so when the last
permitted iteration ends with ``|r| < atol_eff`` the answer is 0 (SciPy tests only at the head of the next iteration and reports
``maxiter``); and ``callback(xk)`` is honoured by running one iteration per synchronisation.  As in SciPy the callback is not called
for a half-step exit.

On the device (``lz_bicgstab_*`` in include/lanczos_hip.h) the scalars never leave it inside a chunk of
``check_every`` iterations: one-block kernels form ``alpha``, ``omega``, ``rho`` and ``beta`` and set a flag that gates the rest of the
chunk.  ``solve`` below is the host loop over chunks; it runs on ``DeviceBicgstabBackend`` and on ``NumpyBicgstabBackend``, a host
restatement of the same calls, which the host tests drive.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse

from .eigsh import _EPS, is_complex_matrix, upload_matrix
from .expm import _as_operator, _entry00

_TINY = _EPS * _EPS  # rhotol = omegatol (SciPy's values: the exit codes depend on them)


class NumpyBicgstabBackend:
    """The calls of ``DeviceBicgstabBackend`` in NumPy - ``begin`` / ``set_state`` leave the head tests to the first ``run``, which
    knows ``atol_eff``, and ``run`` applies the head tests of the next iteration at the end of each - : what the host tests drive
    ``solve`` with.  ``dot``: the inner product (the tests' reference runs pass other summation orders)."""

    launches_per_iteration = None

    def __init__(self, A, dot=None):
        self.A = _as_operator(A)
        self.n = self.A.shape[0]
        self.dot = dot if dot is not None else (lambda a, b: float(a @ b))

    def _fresh(self, k, x, r, rtilde, p, v, rho_prev, alpha, omega):
        self.x, self.r, self.rtilde, self.p, self.v = x, r, rtilde, p, v
        self.t = np.zeros(self.n)
        self.rho_prev, self.alpha, self.omega, self.beta = float(rho_prev), float(alpha), float(omega), 0.0
        self.rho = self.dot(self.rtilde, self.r)
        self.rnorm = float(np.sqrt(self.dot(self.r, self.r)))
        self.snorm = 0.0
        self.steps, self.done, self.code, self.exit, self.head, self.fresh = int(k), False, 0, None, False, True
        self.hist = {}

    def begin(self, b, x0):
        b = np.asarray(b, dtype=np.float64)
        x = np.zeros(self.n) if x0 is None else np.array(x0, dtype=np.float64)
        r = b.copy() if x0 is None else b - self.A @ x
        self._fresh(0, x, r, r.copy(), np.zeros(self.n), np.zeros(self.n), 1.0, 1.0, 1.0)

    def set_state(self, k, x, r, rtilde, p, v, scalars):
        self._fresh(k, *(np.array(a, dtype=np.float64) for a in (x, r, rtilde, p, v)), *scalars)

    def _head(self, atol):
        """the head tests of iteration ``steps``; ``beta`` for its ``p``"""
        if self.rnorm < atol:
            self.done, self.code, self.exit, self.head = True, 0, "full", True
        elif abs(self.rho) < _TINY:
            self.done, self.code, self.exit, self.head = True, -10, "breakdown", True
        elif self.steps > 0 and abs(self.omega) < _TINY:
            self.done, self.code, self.exit, self.head = True, -11, "breakdown", True
        elif self.steps > 0:
            self.beta = (self.rho / self.rho_prev) * (self.alpha / self.omega)

    def run(self, iters, atol):
        with np.errstate(all="ignore"):  # (a stagnating run divides by a vanished t . t, as the device does)
            if self.fresh:
                self.fresh = False
                self._head(atol)
            for _ in range(int(iters)):
                if self.done:
                    break
                k = self.steps
                self.p = self.r.copy() if k == 0 else (self.p - self.omega * self.v) * self.beta + self.r
                self.v = np.asarray(self.A @ self.p)
                rv = self.dot(self.rtilde, self.v)
                if rv == 0.0:
                    self.done, self.code, self.exit, self.head = True, -11, "breakdown", False
                    break
                self.alpha = self.rho / rv
                self.r = self.r - self.alpha * self.v  # s, in place
                self.snorm = float(np.sqrt(self.dot(self.r, self.r)))
                self.t = np.asarray(self.A @ self.r)
                if self.snorm < atol:
                    self.x = self.x + self.alpha * self.p
                    self.omega, self.rnorm = 0.0, self.snorm
                    self.hist[k] = (self.snorm, self.snorm)
                    self.steps = k + 1
                    self.done, self.code, self.exit, self.head = True, 0, "half", False
                    break
                self.omega = self.dot(self.t, self.r) / self.dot(self.t, self.t)
                self.x = (self.x + self.alpha * self.p) + self.omega * self.r
                self.r = self.r - self.omega * self.t
                self.rho_prev, self.rho = self.rho, self.dot(self.rtilde, self.r)
                self.rnorm = float(np.sqrt(self.dot(self.r, self.r)))
                self.hist[k] = (self.snorm, self.rnorm)
                self.steps = k + 1
                self._head(atol)
        return self._state()

    def _state(self):
        return {"iterations": self.steps, "done": bool(self.done), "code": self.code, "exit": self.exit, "head": self.head,
                "rnorm": self.rnorm, "rho": self.rho, "rho_prev": self.rho_prev, "alpha": self.alpha, "omega": self.omega,
                "beta": self.beta, "snorm": self.snorm}

    def history(self, count):
        return np.array([self.hist.get(i, (0.0, 0.0)) for i in range(int(count))], dtype=np.float64).reshape(int(count), 2)

    def solution(self):
        return self.x.copy()

    def get(self, which):
        return getattr(self, which).copy()


class DeviceBicgstabBackend:
    """The ``lz_bicgstab_*`` calls on one ``_capi.Handle`` that already holds the matrix."""

    def __init__(self, handle, n):
        self.h = handle
        self.n = n
        self.launches_per_iteration = handle.bicgstab_info()["launches_per_iteration"]

    def begin(self, b, x0):
        self.h.bicgstab_begin(b, x0)

    def set_state(self, k, x, r, rtilde, p, v, scalars):
        self.h.bicgstab_set_state(k, x, r, rtilde, p, v, scalars)

    def run(self, iters, atol):
        return self.h.bicgstab_run(iters, atol)

    def history(self, count):
        return self.h.bicgstab_history(count)

    def solution(self):
        return self.h.bicgstab_get("x")

    def get(self, which):
        return self.h.bicgstab_get(which)


def finish(backend, st, maxiter, first=0, extra_products=0, chunks=0, atol_eff=0.0, info=None):
    """``(x, info_int)`` of a backend whose last ``run`` returned ``st``, and the run's counts into ``info``.  A breakdown that a head
    test found after the last permitted iteration is SciPy's ``maxiter``: it never enters the iteration that would have tested."""
    done, code, kind = st["done"], st["code"], st["exit"]
    if done and st["head"] and code < 0 and st["iterations"] - first >= maxiter:
        done = False
    if not done:
        code, kind = int(maxiter), "maxiter"
    ran = st["iterations"] - first
    products = 2 * ran - (1 if kind == "half" else 0) + (1 if kind == "breakdown" and not st["head"] else 0) + extra_products
    x = backend.solution()
    if info is not None:
        info.update({"iterations": ran, "code": int(code), "exit": kind, "residual_norm": st["rnorm"], "atol_effective": float(atol_eff),
                     "products": int(products), "chunks": chunks, "launches_per_iteration": backend.launches_per_iteration,
                     "history": backend.history(st["iterations"])[first:]})
    return x, int(code)


def solve(backend, b, x0, atol_eff, maxiter, check_every, callback=None, info=None, begun=False):
    """The loop over chunks on a backend (``NumpyBicgstabBackend`` or ``DeviceBicgstabBackend``) -> ``(x, info_int)``.  With a
    ``callback`` a chunk is one iteration and ``x`` is fetched behind each that ended with its full step.  ``begun``: the backend holds
    a state already (``set_state``), which ``maxiter`` more iterations continue."""
    if not begun:
        backend.begin(b, x0)
    chunk = 1 if callback is not None else int(check_every)
    st = backend.run(0, atol_eff)
    first = st["iterations"]
    chunks = 0
    while not st["done"] and st["iterations"] - first < maxiter:
        before = st["iterations"]
        st = backend.run(min(chunk, maxiter - (st["iterations"] - first)), atol_eff)
        chunks += 1
        if callback is not None and st["iterations"] > before and st["exit"] != "half":
            callback(backend.solution())
    return finish(backend, st, maxiter, first, 0 if (begun or x0 is None) else 1, chunks, atol_eff, info)


def check_bicgstab_args(A, b, x0, M, maxiter, check_every, rtol, atol):
    """``(n, b as (n,) float64, x0 as (n,) float64 or None, maxiter)`` or the error of a bad call - before any device is asked for"""
    if M is not None:
        raise NotImplementedError("bicgstab: preconditioning (M) is not implemented")
    if not scipy.sparse.issparse(A) and not isinstance(A, np.ndarray) and hasattr(A, "matvec"):
        raise NotImplementedError("bicgstab: LinearOperator input is not implemented (a SciPy sparse matrix, a dense array, synthetic.CSR or StencilOperator)")
    if not hasattr(A, "shape"):
        A = np.asarray(A)
    if len(A.shape) != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"expected square matrix (shape={A.shape})")
    if is_complex_matrix(A):
        raise NotImplementedError("bicgstab: complex A is not implemented (real matrices only)")
    n = int(A.shape[0])
    if n < 1:
        raise ValueError(f"expected a matrix with at least one row (shape={A.shape})")
    b = np.asarray(b)
    if np.iscomplexobj(b):
        raise NotImplementedError("bicgstab: complex b is not implemented")
    if not (b.shape == (n,) or b.shape == (n, 1)):
        raise ValueError(f"shapes of A {A.shape} and b {b.shape} are incompatible")
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(n)
    if x0 is not None:
        x0 = np.asarray(x0)
        if np.iscomplexobj(x0):
            raise NotImplementedError("bicgstab: complex x0 is not implemented")
        if not (x0.shape == (n,) or x0.shape == (n, 1)):
            raise ValueError(f"shapes of A {A.shape} and x0 {x0.shape} are incompatible")
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(n)
    if maxiter is None:
        maxiter = 10 * n
    maxiter = int(maxiter)
    if maxiter < 0:
        raise ValueError("maxiter must be non-negative")
    if int(check_every) < 1:
        raise ValueError("check_every must be at least 1")
    if not float(rtol) >= 0.0 or not float(atol) >= 0.0:
        raise ValueError("rtol and atol must be non-negative")
    return n, b, x0, maxiter


def bicgstab(A, b, x0=None, *, rtol=1e-5, atol=0.0, maxiter=None, M=None, callback=None, check_every=8, device_id=0, handle=None,
             info=None, _backend=None):
    """Solve ``A x = b`` for a real square ``A``, symmetric or not - ``scipy.sparse.linalg.bicgstab``'s signature, defaults and loop - by
    BiCGSTAB on the GPU.  Returns ``(x, info_int)``: ``x`` is ``(n,)`` float64; ``info_int`` is 0 on convergence, ``maxiter`` when the
    iterations ran out, -10 when ``rho = rtilde . r`` vanished and -11 when ``omega`` or ``rtilde . v`` did (SciPy's breakdown codes).

    ``A``: what ``eigs`` takes for a real matrix - any SciPy sparse format, a dense ndarray, ``synthetic.CSR`` or ``StencilOperator``.
    ``b``: ``(n,)`` or ``(n, 1)``, real.  ``b = 0`` returns zeros and 0, as SciPy does.  ``x0``: the starting guess (an all-zero one is
    no guess: ``r = b`` without a product).  Convergence: ``|r| < max(atol, rtol |b|)`` on the recurrence's residual, tested at the head
    of every iteration and on ``s`` at the half step, as SciPy tests.  ``maxiter``: default ``10 n``.

    Two deliberate deviations from SciPy.  When the last permitted iteration ends with ``|r| < atol_eff`` the answer is 0: SciPy tests
    only at the head of the next iteration and reports ``maxiter``.  ``callback(xk)`` is honoured by running ONE iteration per
    synchronisation and downloading ``x`` behind each, the slow path; as in SciPy it is not called for a half-step exit.

    ``M`` (preconditioning), complex ``A`` / ``b`` / ``x0`` and a ``LinearOperator`` raise ``NotImplementedError``; shape and value
    errors raise ``ValueError``; all of them before any device is asked for.  ``n == 1`` is answered on the host.
    ``check_every`` (default 8, the fastest of 8 / 32 / 128 measured, profiles/r29/bicgstab_probe.json): iterations enqueued between two
    host synchronisations; past the exit the rest of a chunk is gated off on the device, but its products still run - up to
    ``2 check_every - 1`` wasted products, which is what a long chunk costs where the product is most of an iteration.  ``x`` does not
    depend on it.
    ``handle``: an open ``_capi.Handle`` to run on (its square matrix is replaced); ``info``: a dict that receives ``iterations``,
    ``code``, ``exit`` (``"half"``, ``"full"``, ``"breakdown"`` or ``"maxiter"``), ``residual_norm`` (the recurrence's ``|r|`` or
    ``|s|``), ``atol_effective``, ``products``, ``chunks``, ``launches_per_iteration`` and ``history`` (``|s|`` and ``|r|`` of every
    iteration, two per row)."""
    n, b, x0, maxiter = check_bicgstab_args(A, b, x0, M, maxiter, check_every, rtol, atol)
    bnorm = float(np.linalg.norm(b))
    atol_eff = max(float(atol), float(rtol) * bnorm)
    if x0 is not None and not np.any(x0):
        x0 = None
    run = {"iterations": 0, "code": 0, "exit": "full", "residual_norm": 0.0, "atol_effective": atol_eff, "products": 0, "chunks": 0,
           "launches_per_iteration": None, "history": np.zeros((0, 2))}
    if bnorm == 0.0:
        x, code = np.zeros(n), 0
    elif n == 1:
        x, code = b / float(_entry00(A)), 0
        if callback is not None:
            callback(x.copy())
    elif _backend is not None:  # the host tests' way in: a NumpyBicgstabBackend
        x, code = solve(_backend, b, x0, atol_eff, maxiter, check_every, callback, run)
    else:
        from . import _capi

        h = handle if handle is not None else _capi.Handle(device_id)
        try:
            upload_matrix(h, A)
            x, code = solve(DeviceBicgstabBackend(h, n), b, x0, atol_eff, maxiter, check_every, callback, run)
        finally:
            if handle is None:
                h.close()
    if info is not None:
        info.update(run)
    return np.asarray(x, dtype=np.float64).reshape(n), code
