"""``minres``: solve ``(A - shift I) x = b`` for a real symmetric ``A``, definite or not, on the GPU.

MINRES (Paige & Saunders 1975) is the Lanczos method for linear systems: the three-term recurrence of ``lz_run`` with no basis kept,
and the solution updated from the QR factorisation of the tridiagonal matrix, which one Givens rotation per step maintains.  With
normalised Lanczos vectors and SciPy's sign convention (``cs = -1, sn = 0`` at the start) step ``k = 1, 2, ...`` is

    y = A v_k                       alpha = v_k . y - shift
    r = y - (alpha + shift) v_k - beta_k v_{k-1}          beta_{k+1} = |r|
    tnorm2 += alpha^2 + beta_k^2 + beta_{k+1}^2
    oldeps = epsln;  delta = cs dbar + sn alpha;  gbar = sn dbar - cs alpha;  epsln = sn beta_{k+1};  dbar = -cs beta_{k+1}
    gamma = max(hypot(gbar, beta_{k+1}), eps);  cs = gbar / gamma;  sn = beta_{k+1} / gamma;  phi = cs phibar;  phibar = sn phibar
    w_k = (v_k - oldeps w_{k-2} - delta w_{k-1}) / gamma;      x += phi w_k;      v_{k+1} = r / beta_{k+1}

from ``r0 = b - (A - shift I) x0``, ``beta_1 = |r0|``, ``v_1 = r0 / beta_1``, ``phibar = beta_1`` and zeros elsewhere.  ``phibar`` after
step ``k`` is ``|b - (A - shift I) x_k|`` in exact arithmetic.

Stopping rule: after the first step with ``phibar <= rtol * beta_1`` (``info = 0``) or after ``maxiter`` steps (``info = maxiter``).
A ``beta_{k+1}`` that is zero or not finite (an invariant subspace: ``phibar`` is then 0) stops behind that step's update.  The test
is ``|r| <= rtol |b|`` (``|r0|`` with an ``x0``), deliberately stricter than SciPy's ``|r| <= rtol |A| |x|``, which needs a norm of ``x``
at every step.

On the device (``lz_minres_*`` in include/lanczos_hip.h) the scalars never leave it inside a chunk of
``check_every`` steps: a one-block kernel does the rotation and sets a flag that gates the rest of the chunk, and the update of ``w``
and ``x`` rides one step behind in the streaming pass that forms ``r``, because its scalars are not known before ``beta_{k+1}`` is.  The
pending update is applied when a chunk ends.  ``solve`` below is the host loop over chunks; it runs on ``DeviceMinresBackend`` and on
``NumpyMinresBackend``, a host restatement of the same calls with the same lag, which the host tests drive.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse

from .eigsh import _EPS, is_complex_matrix, upload_matrix
from .expm import _as_operator, _entry00


class NumpyMinresBackend:
    """The calls of ``DeviceMinresBackend`` in NumPy, the lag of the update and the flush included: what the host tests drive ``solve``
    with.  ``v_k`` is formed on read as ``r / nu``; between two calls the pending update is applied."""

    launches_per_iteration = None

    def __init__(self, A):
        self.A = _as_operator(A)
        self.n = self.A.shape[0]

    def begin(self, b, x0, shift):
        n = self.n
        self.shift = float(shift)
        self.x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
        b = np.asarray(b, dtype=np.float64)
        self.r = b.copy() if x0 is None else b - (self.A @ self.x - self.shift * self.x)
        self.v = [np.zeros(n), np.zeros(n)]  # v_j in v[j & 1]
        self.w = [np.zeros(n), np.zeros(n)]  # w_j in w[j & 1]
        self.nrm2 = float(self.r @ self.r)
        self.beta1 = self.beta = float(np.sqrt(self.nrm2))
        self.cs, self.sn, self.dbar, self.epsln, self.phibar, self.tnorm2, self.alpha = -1.0, 0.0, 0.0, 0.0, self.beta1, 0.0, 0.0
        self.lag = (0.0, 0.0, 1.0, 0.0)  # oldeps, delta, gamma, phi of the step whose update is pending
        self.steps = 0
        self.done = not (self.beta1 > 0.0 and np.isfinite(self.beta1))
        self.hist = []

    def _update(self):
        """the end of step ``j = steps``: ``w_j`` and ``x += phi_j w_j``"""
        j = self.steps
        oldeps, delta, gamma, phi = self.lag
        w = ((self.v[j & 1] - oldeps * self.w[j & 1]) - delta * self.w[(j + 1) & 1]) / gamma
        self.w[j & 1] = w
        self.x = self.x + phi * w

    def run(self, iters, rtol):
        first = self.steps
        with np.errstate(all="ignore"):  # (a breakdown divides by a vanished beta, as the device does)
            for i in range(int(iters) if not self.done else 0):
                nu = np.sqrt(self.nrm2)
                vk = self.r / nu
                y = self.A @ vk
                self.alpha = float(vk @ y) - self.shift
                a, b = self.alpha + self.shift, self.beta
                j = self.steps
                r = (y - a * vk) - b * self.v[j & 1]
                if i > 0:
                    self._update()  # the step kernel ends step j in the pass that forms r
                self.v[(j + 1) & 1] = vk
                self.r = r
                nrm2 = float(r @ r)
                beta = float(np.sqrt(nrm2))
                self.tnorm2 += (self.alpha * self.alpha + self.beta * self.beta) + beta * beta
                oldeps = self.epsln
                delta = self.cs * self.dbar + self.sn * self.alpha
                gbar = self.sn * self.dbar - self.cs * self.alpha
                self.epsln = self.sn * beta
                self.dbar = -self.cs * beta
                gamma = float(np.hypot(gbar, beta))
                if not gamma >= _EPS and gamma == gamma:
                    gamma = _EPS
                self.cs, self.sn = gbar / gamma, beta / gamma
                phi = self.cs * self.phibar
                self.phibar = self.sn * self.phibar
                self.nrm2, self.beta = nrm2, beta
                self.lag = (oldeps, delta, gamma, phi)
                self.steps += 1
                self.hist.append(self.phibar)
                if not self.phibar > rtol * self.beta1 or not beta > 0.0 or not np.isfinite(beta):
                    self.done = True
                    break
            if self.steps > first:
                self._update()  # the flush: the update of the last step that ran
        return self._state()

    def _state(self):
        return {"iterations": self.steps, "done": bool(self.done), "phibar": self.phibar, "beta1": self.beta1,
                "anorm": float(np.sqrt(self.tnorm2)), "alpha": self.alpha, "beta": self.beta}

    def history(self, count):
        return np.array(self.hist[:count])

    def solution(self):
        return self.x.copy()

    def spmv(self, x):
        return self.A @ x


class DeviceMinresBackend:
    """The ``lz_minres_*`` calls on one ``_capi.Handle`` that already holds the matrix."""

    def __init__(self, handle, n):
        self.h = handle
        self.n = n
        self.launches_per_iteration = handle.minres_info()["launches_per_iteration"]

    def begin(self, b, x0, shift):
        self.h.minres_begin(b, x0, shift)

    def run(self, iters, rtol):
        return self.h.minres_run(iters, rtol)

    def history(self, count):
        return self.h.minres_history(count)

    def solution(self):
        return self.h.minres_get("x")

    def spmv(self, x):
        return self.h.spmv_host(x)


def check_symmetry(backend, b):
    """SciPy's test: with ``y = A b`` and ``w = A y``, ``|y . y - b . w|`` must stay below ``eps^(1/3) max(y . y, |b . w|)``"""
    y = backend.spmv(b)
    w = backend.spmv(y)
    s, t = float(y @ y), float(b @ w)
    if abs(s - t) > (max(s, abs(t)) + _EPS) * _EPS ** (1.0 / 3.0):
        raise ValueError("non-symmetric matrix")


def solve(backend, b, x0, shift, rtol, maxiter, check_every, callback=None, show=False, check=False, info=None):
    """The loop over chunks on a backend (``NumpyMinresBackend`` or ``DeviceMinresBackend``) -> ``(x, info_int)``.  With a ``callback`` a
    chunk is one step and ``x`` is fetched behind each."""
    if check:
        check_symmetry(backend, b)
    backend.begin(b, x0, shift)
    chunk = 1 if callback is not None else int(check_every)
    st = backend.run(0, rtol)
    chunks = 0
    while not st["done"] and st["iterations"] < maxiter:
        st = backend.run(min(chunk, maxiter - st["iterations"]), rtol)
        chunks += 1
        if show:
            print(f"minres: chunk {chunks:5d}  iterations {st['iterations']:7d}  phibar {st['phibar']:.3e}  phibar / beta1 {st['phibar'] / st['beta1']:.3e}")
        if callback is not None:
            callback(backend.solution())
    x = backend.solution()
    if info is not None:
        info.update({"iterations": st["iterations"], "residual_estimate": st["phibar"], "beta1": st["beta1"], "anorm_estimate": st["anorm"],
                     "chunks": chunks, "launches_per_iteration": backend.launches_per_iteration,
                     "history": backend.history(st["iterations"])})
    return x, (0 if st["done"] else int(maxiter))


def check_minres_args(A, b, x0, M, maxiter, check_every, rtol):
    """``(n, b as (n,) float64, x0 as (n,) float64 or None, maxiter)`` or the error of a bad call - before any device is asked for"""
    if M is not None:
        raise NotImplementedError("minres: preconditioning (M) is not implemented")
    if len(A.shape) != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"expected square matrix (shape={A.shape})")
    if is_complex_matrix(A):
        raise NotImplementedError("minres: complex A is not implemented (real symmetric matrices only)")
    n = int(A.shape[0])
    b = np.asarray(b)
    if np.iscomplexobj(b):
        raise NotImplementedError("minres: complex b is not implemented")
    if not (b.shape == (n,) or b.shape == (n, 1)):
        raise ValueError(f"shapes of A {A.shape} and b {b.shape} are incompatible")
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(n)
    if x0 is not None:
        x0 = np.asarray(x0)
        if np.iscomplexobj(x0):
            raise NotImplementedError("minres: complex x0 is not implemented")
        if not (x0.shape == (n,) or x0.shape == (n, 1)):
            raise ValueError(f"shapes of A {A.shape} and x0 {x0.shape} are incompatible")
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(n)
    if maxiter is None:
        maxiter = 5 * n
    maxiter = int(maxiter)
    if maxiter < 0:
        raise ValueError("maxiter must be non-negative")
    if int(check_every) < 1:
        raise ValueError("check_every must be at least 1")
    if not float(rtol) >= 0.0:
        raise ValueError("rtol must be non-negative")
    return n, b, x0, maxiter


def minres(A, b, x0=None, *, rtol=1e-5, shift=0.0, maxiter=None, M=None, callback=None, show=False, check=False, check_every=8,
           device_id=0, handle=None, info=None, _backend=None):
    """Solve ``(A - shift I) x = b`` for a real symmetric ``A`` - ``scipy.sparse.linalg.minres``'s signature - by MINRES on the GPU.
    Returns ``(x, info_int)``: ``x`` is ``(n,)`` float64, ``info_int`` 0 on convergence and ``maxiter`` when the steps ran out.

    ``A``: what ``eigsh`` takes for a real matrix - any SciPy sparse format, a dense ndarray, ``synthetic.CSR`` or ``StencilOperator``;
    symmetry is assumed unless ``check=True``, which runs SciPy's two-product test on the device's product and raises ``ValueError``.
    ``b``: ``(n,)`` or ``(n, 1)``, real.  ``b = 0`` returns ``x0`` (or zeros) and 0.  ``x0``: the starting guess; the residual it starts
    from is ``b - (A - shift I) x0`` - SciPy itself forms ``b - A x0`` there and forgets the shift, which is not copied.
    ``rtol``: stop after the first step with ``phibar <= rtol |r0|`` (``|r0| = |b|`` without ``x0``), where ``phibar`` is the recurrence's
    estimate of ``|b - (A - shift I) x|``.  This is stricter than SciPy's ``|r| <= rtol |A| |x|``.  ``maxiter``: default ``5 n``.
    ``M`` (preconditioning), complex ``A`` and complex ``b`` raise ``NotImplementedError``; argument errors are raised before any
    device is asked for.  ``check_every`` (default 8, the fastest of 8 / 32 / 128 measured, profiles/r27/minres_probe.json): steps enqueued between two host
    synchronisations; past convergence the rest of a chunk is gated off on the device, but its products still run - up to
    ``check_every - 1`` wasted products, which is what a long chunk costs where the product is most of a step.  ``x`` does not depend
    on it.  ``callback(xk)`` is honoured by running ONE
    step per synchronisation and downloading ``x`` behind each: the slow path.  ``show``: one line per chunk.  ``n == 1`` is answered
    on the host.  ``handle``: an open ``_capi.Handle`` to run on (its matrix is replaced); ``info``: a dict that receives
    ``iterations``, ``residual_estimate`` (``phibar``), ``beta1``, ``anorm_estimate``, ``chunks``, ``launches_per_iteration`` and
    ``history`` (``phibar`` per step).
    Consistent singular systems are solved; an inconsistent one is MINRES-QLP's job and is not detected."""
    n, b, x0, maxiter = check_minres_args(A, b, x0, M, maxiter, check_every, rtol)
    rtol, shift = float(rtol), float(shift)
    run = {"iterations": 0, "residual_estimate": 0.0, "beta1": 0.0, "anorm_estimate": 0.0, "chunks": 0, "launches_per_iteration": None,
           "history": np.zeros(0)}
    if not np.any(b):
        x, code = (np.zeros(n) if x0 is None else x0.copy()), 0
    elif n == 1:
        d = float(_entry00(A)) - shift
        x, code = b / d, 0
        if callback is not None:
            callback(x.copy())
        run["beta1"] = float(abs(b[0]))
    elif _backend is not None:  # the host tests' way in: a NumpyMinresBackend
        x, code = solve(_backend, b, x0, shift, rtol, maxiter, check_every, callback, show, check, run)
    else:
        from . import _capi

        h = handle if handle is not None else _capi.Handle(device_id)
        try:
            upload_matrix(h, A)
            x, code = solve(DeviceMinresBackend(h, n), b, x0, shift, rtol, maxiter, check_every, callback, show, check, run)
        finally:
            if handle is None:
                h.close()
    if info is not None:
        info.update(run)
    return np.asarray(x, dtype=np.float64).reshape(n), code
