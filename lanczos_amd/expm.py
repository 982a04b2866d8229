"""``expm_multiply``: the action of a matrix exponential, ``exp(a t A) b``, for a real symmetric or complex Hermitian ``A`` on the GPU.

The method is the short-iterative Lanczos propagator (Park & Light 1986; error estimate: Saad 1992).  From the current state ``psi``
at time ``t`` it takes ``m = ncv`` Lanczos steps with full re-orthogonalisation, which give an orthonormal basis ``V`` of the Krylov
space of ``psi`` and the small projected matrix ``T = V A V^H``, and then

    psi(t + tau) = |psi| V^T exp(a tau T) e_1

for a step ``tau`` that the error estimate allows; then it repeats from the new state.  The basis, both products and every pass over
the basis live on the device (``lz_expm_*`` in include/lanczos_hip.h); the host keeps ``T`` and runs the loop below.  The state never
leaves the device between substeps: only the requested outputs are downloaded.

Routes, chosen from the dtypes alone: ``A``, ``b`` and ``a`` all real - a real basis and the real product; ``A`` real and ``b`` or
``a`` complex (a real Hamiltonian in Schroedinger time, ``a = -1j``) - a planar complex basis and the mixed product of a real matrix
with a complex vector, which reads the matrix once for both planes where that pays; ``A`` complex - the planar
basis and the complex product.

Substep.  ``theta, S = eigh(T[:mm, :mm])`` and ``c(tau) = S (exp(a tau theta) * conj(S[0]))`` are the coefficients of the propagated
state in the basis.  The estimate of its error is ``est(tau) = beta[mm - 1] |c(tau)[mm - 1]| |psi|``, the weight that has reached the
last basis vector times its coupling to what lies outside the space.  The step accepted is the largest ``tau`` - the whole way to
the last pending time of the current direction first, then shrunk by factors of 0.7 - with ``est(tau) <= tol |psi| |tau| / T_total``,
where ``T_total`` is the length of the whole path: the budget is spread evenly over the path and is relative to the CURRENT norm, so
the result errs by about ``tol`` relative to its own norm whether the solution grows or decays.  The search is host arithmetic on
``mm`` numbers.  Every output time inside the step is produced from the same basis: one rotation ``C^T V`` in place on the device makes
the new state (row 0) and the outputs (the rows behind it).  An output at the very end of the step is the new state itself.  The
rotation takes fewer columns than rows, so a step reaches at most ``mm - 1`` output times; the next step serves the rest.

Breakdown.  ``beta[j] <= 10 eps |T|`` means the Krylov space of ``psi`` is invariant after ``mm = j + 1`` vectors: the substep is
truncated to them and is exact for any ``tau`` (``est = 0``), and so is a basis that fills the whole space (``mm = n``).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse

from .eigsh import _EPS, _MAX_NCV_COMPLEX, _fill, is_complex_matrix, upload_complex_matrix, upload_matrix

_MAX_SUBSTEPS = 10000
_SHRINK = 0.7


def _as_operator(A):
    """what the NumPy backend multiplies by: a SciPy sparse matrix or an ndarray (``synthetic.CSR`` / ``StencilOperator`` are materialised)"""
    if scipy.sparse.issparse(A) or isinstance(A, np.ndarray):
        return A
    if hasattr(A, "to_scipy"):
        return A.to_scipy()
    return np.asarray(A)


class NumpyExpmBackend:
    """The calls of ``DeviceExpmBackend`` in NumPy: what the host tests drive ``propagate`` with.  ``cplx``: a complex basis (the mixed
    and the complex route); ``<x, y> = sum conj(x) y``."""

    def __init__(self, A, cplx, force_second_pass=False):
        self.A = _as_operator(A)
        self.n = self.A.shape[0]
        self.cplx = bool(cplx)
        self.dtype = np.complex128 if self.cplx else np.float64
        self.force = force_second_pass
        self.state_norm = 0.0

    def begin(self, m, v):
        self.m = int(m)
        self.V = np.zeros((m + 1, self.n), dtype=self.dtype)
        self.state_norm = float(np.linalg.norm(v))
        self.V[0] = np.asarray(v, dtype=self.dtype) / self.state_norm

    def _cgs(self, w, j):
        c = self.V[: j + 1].conj() @ w
        return w - c @ self.V[: j + 1], c

    def extend(self, k0, k1):
        m = self.m
        proj = np.zeros((m, m), dtype=self.dtype)
        beta = np.zeros(m)
        with np.errstate(divide="ignore", invalid="ignore"):  # (a breakdown divides by a vanished beta, as the device does)
            for j in range(k0, k1):
                w = self.A @ self.V[j]
                w0 = np.vdot(w, w).real
                w, c = self._cgs(w, j)
                if self.force or not np.vdot(w, w).real >= 0.5 * w0:  # DGKS: the second pass only when the first cancelled more than half of |w|^2
                    w, c2 = self._cgs(w, j)
                    c = c + c2
                proj[j, : j + 1] = c
                beta[j] = np.linalg.norm(w)
                self.V[j + 1] = w / beta[j]
        return proj, beta

    def combine(self, mm, C):
        C = np.asarray(C, dtype=self.dtype)
        ncols = C.shape[1]
        Y = C.T @ self.V[:mm]  # rows >= mm are never read
        self.state_norm = float(np.linalg.norm(Y[0]))
        self.V[0] = Y[0] / self.state_norm
        self.V[1:ncols] = Y[1:]
        return Y[1:].copy()

    def state(self):
        return self.V[0].copy()


class DeviceExpmBackend:
    """The ``lz_expm_*`` calls on one ``_capi.Handle`` that already holds the matrix.  ``cplx``: the planar complex basis."""

    def __init__(self, handle, n, cplx):
        self.h = handle
        self.n = n
        self.cplx = bool(cplx)
        self.dtype = np.complex128 if self.cplx else np.float64
        self.state_norm = 0.0

    def begin(self, m, v):
        self.state_norm = float(np.linalg.norm(v))
        self.h.expm_begin(m, v, self.cplx)

    def extend(self, k0, k1):
        return self.h.expm_extend(k0, k1)

    def combine(self, mm, C):
        C = np.asarray(C, dtype=self.dtype)
        self.state_norm = self.h.expm_combine(mm, C)
        if C.shape[1] == 1:
            return np.zeros((0, self.n), dtype=self.dtype)
        return self.h.expm_get_rows(1, C.shape[1] - 1)

    def state(self):
        return self.h.expm_get_rows(0, 1)[0]


def _krylov(backend, m, n):
    """``m`` Lanczos steps from row 0 -> ``(theta, S, beta_last, mm)``: the eigen-decomposition of the projected matrix on the first
    ``mm`` rows and the coupling of row ``mm - 1`` to what lies outside them (0: the space is invariant or full)"""
    proj, beta = backend.extend(0, m)
    T = np.zeros((m, m), dtype=backend.dtype)
    mm, scale, broke = m, 0.0, False
    for j in range(m):
        scale = max(scale, float(np.abs(proj[j, : j + 1]).max()))
        if not beta[j] > 10 * _EPS * scale:  # (also a NaN)
            mm, broke = j + 1, True
            break
        scale = max(scale, float(beta[j]))
    with np.errstate(invalid="ignore"):
        _fill(T, proj, beta, 0, mm)
    T = T[:mm, :mm]
    theta, S = np.linalg.eigh((T + T.conj().T) / 2)
    return theta, S, (0.0 if broke or mm == n else float(beta[mm - 1])), mm


def propagate(backend, n, b, a, times, ncv, tol, info=None):
    """The propagator's loop over a backend (``NumpyExpmBackend`` or ``DeviceExpmBackend``): ``exp(a t A) b`` for every ``t`` of
    ``times``, visited in the order given (from 0 to ``times[0]``, then from each to the next).  Returns ``(len(times), n)`` in the
    backend's dtype and fills ``info`` with ``substeps``, ``matvecs``, ``ncv`` and ``err_est`` (the sum of the accepted estimates)."""
    times = [float(t) for t in times]
    out = np.zeros((len(times), n), dtype=backend.dtype)
    run = {"substeps": 0, "matvecs": 0, "ncv": int(ncv), "err_est": 0.0}
    path = [0.0] + times
    T_total = float(sum(abs(path[i + 1] - path[i]) for i in range(len(times))))
    b = np.asarray(b, dtype=backend.dtype)
    b_norm = float(np.linalg.norm(b))
    if T_total == 0.0 or b_norm == 0.0:
        out[:] = b
        if info is not None:
            info.update(run)
        return out
    real = backend.dtype == np.float64
    backend.begin(ncv, b)
    t, k = 0.0, 0  # the state's time; the first pending output
    while k < len(times):
        if times[k] == t:  # a leg of length zero: the state as it stands
            out[k] = b if run["substeps"] == 0 else backend.state_norm * backend.state()
            k += 1
            continue
        if run["substeps"] >= _MAX_SUBSTEPS:
            raise RuntimeError(f"expm_multiply: no convergence after {_MAX_SUBSTEPS} substeps (t = {t} of a path of length {T_total})")
        theta, S, beta_last, mm = _krylov(backend, ncv, n)
        run["substeps"] += 1
        run["matvecs"] += ncv
        norm = backend.state_norm
        s0 = S[0].conj()

        def coef(tau):
            e = np.exp((a.real if real else a) * tau * theta)
            return S @ (e * s0)

        # the pending times that lie one behind the other in the direction of this leg; a step serves at most mm - 1 of them
        sign = 1.0 if times[k] > t else -1.0
        reach = k + 1
        while reach < len(times) and sign * (times[reach] - times[reach - 1]) > 0:
            reach += 1
        reach = min(reach, k + max(mm - 1, 1))
        leg = times[reach - 1] - t
        tau = leg
        while True:
            c = coef(tau)
            est = beta_last * abs(c[mm - 1]) * norm
            if est <= tol * norm * abs(tau) / T_total:
                break
            tau *= _SHRINK
            if not abs(tau) > 1e-12 * abs(leg):
                raise RuntimeError(f"expm_multiply: no convergence, the step underflows at t = {t} (estimate {est:.3e}, ncv = {ncv})")
        run["err_est"] += float(est)
        inside = [i for i in range(k, reach) if abs(times[i] - t) < abs(tau)]  # outputs within the step ...
        at_end = len(inside) < reach - k and times[k + len(inside)] - t == tau  # ... and the one it ends on, which is the new state
        C = norm * np.stack([c] + [coef(times[i] - t) for i in inside], axis=1)
        rows = backend.combine(mm, C.real if real else C)
        for q, i in enumerate(inside):
            out[i] = rows[q]
        k += len(inside)
        t = times[k] if at_end else t + tau
        if at_end:
            out[k] = backend.state_norm * backend.state()
            k += 1
    if info is not None:
        info.update(run)
    return out


def _is_complex_scalar(a):
    return np.iscomplexobj(a)


def _time_grid(start, stop, num, endpoint):
    """SciPy's rule: no grid argument at all means ``t = 1`` and a result of ``B``'s shape, else ``np.linspace`` of the ones given"""
    if start is None and stop is None and num is None and endpoint is None:
        return None
    kw = {key: v for key, v in (("start", start), ("stop", stop), ("num", num), ("endpoint", endpoint)) if v is not None}
    return np.linspace(**kw)


def _entry00(A):
    if scipy.sparse.issparse(A):
        return A.tocsr()[0, 0]
    if hasattr(A, "to_scipy"):
        return A.to_scipy()[0, 0]
    return np.asarray(A)[0, 0]


def check_expm_args(A, B, ncv, a):
    """``(n, B as an ndarray, ncv)`` or the error of a bad call - before any device is asked for"""
    if len(A.shape) != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"expected square matrix (shape={A.shape})")
    n = int(A.shape[0])
    B = np.asarray(B)
    if B.ndim not in (1, 2) or B.shape[0] != n:
        raise ValueError(f"shapes of matrices A {A.shape} and B {B.shape} are incompatible")
    if B.ndim == 2 and B.shape[1] != 1:
        raise NotImplementedError("expm_multiply: B with more than one column (one propagation per column; call once per column)")
    if np.ndim(a) != 0:
        raise ValueError("a must be a scalar")
    if n == 1:
        return n, B, 1
    if ncv is None:
        ncv = min(n, 30)
    ncv = int(ncv)
    if ncv < 2 or ncv > min(n, _MAX_NCV_COMPLEX):
        raise ValueError(f"ncv must satisfy 2 <= ncv <= min(n, {_MAX_NCV_COMPLEX}) (n = {n}, ncv = {ncv})")
    return n, B, ncv


def route_of(A, B, a):
    """``"real"``, ``"mixed"`` or ``"complex"``: from the dtypes alone"""
    if is_complex_matrix(A):
        return "complex"
    return "mixed" if np.iscomplexobj(B) or _is_complex_scalar(a) else "real"


def expm_multiply(A, B, start=None, stop=None, num=None, endpoint=None, traceA=None, *, a=1.0, ncv=None, tol=None, device_id=0,
                  handle=None, info=None, _backend=None):
    """``exp(a t A) B`` for a real symmetric or complex Hermitian ``A`` - ``scipy.sparse.linalg.expm_multiply``'s positional
    signature and meaning, computed by the short-iterative Lanczos propagator on the GPU.

    With none of ``start``, ``stop``, ``num``, ``endpoint`` given ``t = 1`` and the result has ``B``'s shape; otherwise the times are
    ``np.linspace`` of the ones given and the result has shape ``(num,) + B.shape``.  ``traceA`` is accepted and ignored.

    ``A``: what ``eigsh`` takes - any SciPy sparse format, a dense ndarray, ``synthetic.CSR`` or ``StencilOperator`` for a real ``A``;
    complex64 / float32 are converted.  Hermitian-ness is assumed, not checked.  ``a``: a real or complex scalar; ``-1j`` is
    Schroedinger time, ``-1.0`` imaginary time (heat), ``1.0`` SciPy's meaning.  ``B``: ``(n,)`` or ``(n, 1)``, real or complex; more
    columns raise ``NotImplementedError``.  The result is float64 if ``A``, ``B`` and ``a`` are all real, else complex128.
    ``ncv``: Lanczos steps per substep (default ``min(n, 30)``; ``2 <= ncv <= min(n, 64)``).  ``tol`` (default ``1e-12``): the error
    target relative to the norm of the state (see the module docstring).  ``n == 1`` is answered on the host.
    ``handle``: an open ``_capi.Handle`` to run on (its matrix is replaced); ``info``: a dict that receives ``route`` (``"real"``,
    ``"mixed"``, ``"complex"``), ``product`` (the mixed route's product: ``"two-plane"`` or ``"two-launch"``; else None),
    ``substeps``, ``matvecs``, ``ncv`` and ``err_est``.
    Raises ``RuntimeError`` when the step underflows or after 10 000 substeps."""
    n, B, ncv = check_expm_args(A, B, ncv, a)
    tol = 1e-12 if tol is None else float(tol)
    grid = _time_grid(start, stop, num, endpoint)
    times = np.array([1.0]) if grid is None else np.asarray(grid, dtype=np.float64)
    route = route_of(A, B, a)
    dtype = np.float64 if route == "real" else np.complex128
    a = complex(a)
    b = np.asarray(B, dtype=dtype).reshape(n)
    run = {"route": route, "product": None}
    if n == 1:
        lam = _entry00(A)
        e = np.exp(a * times * complex(lam))
        res = (e.real if route == "real" else e)[:, None] * b[None, :]
        run.update({"substeps": 0, "matvecs": 0, "ncv": 1, "err_est": 0.0})
    elif _backend is not None:  # the host tests' way in: a NumpyExpmBackend
        res = propagate(_backend, n, b, a, times, ncv, tol, run)
    else:
        from . import _capi

        h = handle if handle is not None else _capi.Handle(device_id)
        try:
            (upload_complex_matrix if route == "complex" else upload_matrix)(h, A)
            res = propagate(DeviceExpmBackend(h, n, route != "real"), n, b, a, times, ncv, tol, run)
            if route == "mixed":
                run["product"] = h.expm_info()["product"]
        finally:
            if handle is None:
                h.close()
    if info is not None:
        info.update(run)
    res = np.asarray(res, dtype=dtype).reshape((len(times),) + B.shape)
    return res[0] if grid is None else res
