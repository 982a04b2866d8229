"""``gmres``: solve ``A x = b`` for a real square ``A`` by restarted GMRES on the GPU.

GMRES (Saad & Schultz 1986) keeps an orthonormal basis of the Krylov space of the residual and minimises ``|b - A x|`` over it, so it
does not stagnate or break down where ``bicgstab`` does (strongly non-normal matrices), at the price of ``restart + 1`` vectors and a
Gram-Schmidt step per product.  The rules are ``scipy.sparse.linalg.gmres``' (1.15): with ``atol_eff = max(atol, rtol |b|)``, a cycle is

    V[0] = r / |r|;  S = |r| e_0
    for j = 0 .. restart - 1:  w = A V[j];  h0 = |w|;  w against V[0 .. j] (the Hessenberg column);  h1 = |w|;  V[j + 1] = w / h1
        breakdown where h1 <= eps h0;  the stored rotations on the column, the new one (LAPACK lartg);  presid = |S[j + 1]|
        the inner exit on presid <= ptol or on breakdown
    y = the pseudo-solve of the cols x cols triangle (a zero last pivot zeroes its S entry);  x += y . V[:cols];  r = b - A x
    |r| <= atol_eff -> 0;  behind a breakdown the solve ends;  ptol_max_factor = max(eps, 0.25 f) where the inner test passed but the
    outer one did not, else min(1, 1.5 f);  ptol = presid min(f, atol_eff / |r|)

with the first test ``|r| < atol_eff`` and the first ``ptol = |b| min(1, atol_eff / |b|)``.

On the device (``lz_gmres_*`` in include/lanczos_hip.h) the inner step is the thick-restart solver's Arnoldi step
and everything around it - the rotations, the tests, the triangular solve, the update of ``x``, the true residual, the tolerance rule
and the restart - runs in kernels of its own, so a chunk of ``check_every`` inner steps, cycle ends included, is enqueued without
the host seeing a scalar.  ``solve`` below is the host loop over chunks; it runs on ``DeviceGmresBackend`` and on
``NumpyGmresBackend``, a host restatement of the same calls, which the host tests drive.
"""
from __future__ import annotations

import math
import warnings

import numpy as np

from .bicgstab import check_bicgstab_args
from .eigsh import _EPS, upload_matrix
from .expm import _as_operator, _entry00

MAX_RESTART = 128  # the basis layer holds at most 128 + 1 rows

_SAFMIN, _SAFMAX, _RTMIN, _RTMAX = 2.0 ** -1022, 2.0 ** 1022, 2.0 ** -511, math.sqrt(2.0 ** 1021)


def lartg(f, g):
    """LAPACK 3.10's ``dlartg`` -> ``(c, s, r)`` with ``c f + s g = r``: the signs and the scaling SciPy's binding gives, bit for bit"""
    f, g = float(f), float(g)
    f1, g1 = abs(f), abs(g)
    if g == 0.0:
        return 1.0, 0.0, f
    if f == 0.0:
        return 0.0, math.copysign(1.0, g), g1
    if _RTMIN < f1 < _RTMAX and _RTMIN < g1 < _RTMAX:
        d = math.sqrt(f * f + g * g)
        r = math.copysign(d, f)
        return f1 / d, g / r, r
    u = min(_SAFMAX, max(_SAFMIN, f1, g1))
    fs, gs = f / u, g / u
    d = math.sqrt(fs * fs + gs * gs)
    r = math.copysign(d, f)
    return abs(fs) / d, gs / r, r * u


def pseudo_solve(R, S, cols):
    """SciPy's triangular pseudo-solve on column-stored ``R`` (``R[j, :j + 1]`` is column ``j``): zeroes ``S[cols - 1]`` behind a zero
    last pivot, returns ``y`` (``cols`` entries)"""
    col = cols - 1
    if R[col, col] == 0:
        S[col] = 0
    y = np.array(S[:cols], dtype=R.dtype)
    with np.errstate(all="ignore"):
        for k in range(col, 0, -1):
            if y[k] != 0:
                y[k] = y[k] / R[k, k]
                y[:k] = y[:k] - y[k] * R[k, :k]
        if y[0] != 0:
            y[0] = y[0] / R[0, 0]
    return y


class NumpyGmresBackend:
    """The calls of ``DeviceGmresBackend`` in NumPy, the device's bookkeeping included: the steps behind an inner exit change nothing
    until the cycle end the host foresees (``cols == restart``) or the next call, and the Gram-Schmidt step is the basis layer's -
    classical, with a second pass when ``|w|`` fell below ``|w_before| / sqrt 2`` (DGKS).  ``dot``: the inner product (the tests'
    reference runs pass other summation orders)."""

    launches_per_step = None

    def __init__(self, A, dot=None):
        self.A = _as_operator(A)
        self.n = self.A.shape[0]
        self.dot = dot if dot is not None else (lambda a, b: float(a @ b))

    def _alloc(self, restart):
        m = self.m = int(restart)
        self.V = np.zeros((max(m, 2) + 1, self.n))
        self.R = np.zeros((m, m))
        self.gc, self.gs, self.S, self.y = np.zeros(m), np.zeros(m), np.zeros(m + 1), np.zeros(m)
        self.ptol = self.factor = self.presid = self.rnorm = self.bnorm = 0.0
        self.done = self.inner = self.breakdown = self.converged = False
        self.cols = self.iters = self.cycles = self.hcol = 0
        self.fresh = False
        self.hist, self.chist = [], []

    def begin(self, restart, b, x0):
        self._alloc(restart)
        self.b = np.asarray(b, dtype=np.float64).copy()
        self.bnorm = math.sqrt(self.dot(self.b, self.b))
        self.x = np.zeros(self.n) if x0 is None else np.array(x0, dtype=np.float64)
        self.w = self.b.copy() if x0 is None else self.b - np.asarray(self.A @ self.x)
        self.fresh = True

    def set_state(self, restart, x, b, w, rows, small):
        """``small``: the dict ``get("small")`` returns"""
        self._alloc(restart)
        self.x, self.b, self.w = (np.array(a, dtype=np.float64)[: self.n] for a in (x, b, w))
        rows = np.asarray(rows, dtype=np.float64)
        self.V[: rows.shape[0]] = rows[:, : self.n]
        for k in ("R", "gc", "gs", "S"):
            getattr(self, k)[...] = small[k]
        for k in ("ptol", "factor", "presid", "rnorm", "bnorm"):
            setattr(self, k, float(small[k]))
        for k in ("inner", "breakdown", "done", "converged"):
            setattr(self, k, bool(small[k]))
        self.cols, self.iters, self.cycles = int(small["cols"]), int(small["iters"]), int(small["cycles"])
        self.hcol = self.cols
        self.hist, self.chist = [0.0] * self.iters, [(0.0, 0.0, 0.0)] * self.cycles

    def _v0(self):
        rr = self.dot(self.w, self.w)
        self.rnorm = math.sqrt(rr)
        return rr

    def _first(self, atol):
        self._v0()
        if self.rnorm < atol:
            self.done = self.converged = True
            return
        self.factor = 1.0
        self.ptol = self.bnorm * min(1.0, atol / self.bnorm)
        self._restart()

    def _restart(self):
        self.V[0] = self.w / self.rnorm
        self.S[:] = 0.0
        self.S[0] = self.rnorm
        self.gc[:] = 0.0
        self.gs[:] = 0.0
        self.cols, self.inner = 0, False

    def _step(self, j):
        V, dot = self.V, self.dot
        w = np.asarray(self.A @ V[j], dtype=np.float64)
        h0sq = dot(w, w)
        proj = np.array([dot(V[i], w) for i in range(j + 1)])
        w = w - proj @ V[: j + 1]
        nrm2 = dot(w, w)
        if nrm2 < 0.5 * h0sq:  # DGKS: pass 1 cancelled more than half of |w|^2
            c2 = np.array([dot(V[i], w) for i in range(j + 1)])
            w = w - c2 @ V[: j + 1]
            nrm2 = dot(w, w)
            proj = proj + c2
        h1 = math.sqrt(nrm2)
        with np.errstate(all="ignore"):
            V[j + 1] = w / h1
        self.w = w
        brk = h1 <= _EPS * math.sqrt(h0sq)
        if brk:
            h1 = 0.0
        col = np.append(proj, h1)
        for k in range(j):
            c, s, n0, n1 = self.gc[k], self.gs[k], col[k], col[k + 1]
            col[k], col[k + 1] = c * n0 + s * n1, -s * n0 + c * n1
        c, s, mag = lartg(col[j], h1)
        self.gc[j], self.gs[j] = c, s
        col[j] = mag
        self.R[j, : j + 1] = col[: j + 1]
        tmp = -s * self.S[j]
        self.S[j], self.S[j + 1] = c * self.S[j], tmp
        self.presid = abs(tmp)
        self.hist.append(self.presid)
        self.iters += 1
        self.cols = j + 1
        self.breakdown = self.breakdown or bool(brk)
        if self.presid <= self.ptol or brk:
            self.inner = True

    def _end_cycle(self, atol):
        self.hcol = 0
        if self.done:
            return
        if self.cols >= 1:
            self.y[:] = 0.0
            self.y[: self.cols] = pseudo_solve(self.R, self.S, self.cols)
            with np.errstate(all="ignore"):
                self.x = self.x + self.y[: self.cols] @ self.V[: self.cols]
        self.w = self.b - np.asarray(self.A @ self.x)
        self._v0()
        self.chist.append((self.rnorm, float(self.cols), self.ptol))
        self.cycles += 1
        if self.rnorm <= atol:
            self.done = self.converged = True
        elif self.breakdown:
            self.done = True
        else:
            self.factor = max(_EPS, 0.25 * self.factor) if self.presid <= self.ptol else min(1.0, 1.5 * self.factor)
            self.ptol = self.presid * min(self.factor, atol / self.rnorm)
            self._restart()

    def _head(self, atol):
        if self.fresh:
            self.fresh = False
            self._first(atol)
        if self.inner and not self.done:
            self._end_cycle(atol)

    def run(self, steps, atol):
        if not (self.done and not self.fresh):
            self._head(atol)
            for _ in range(int(steps)):
                j = self.hcol
                if not (self.done or self.inner):
                    self._step(j)
                self.hcol = j + 1
                if self.hcol == self.m:
                    self._end_cycle(atol)
        return self._state()

    def end_cycle(self, atol):
        if not (self.done and not self.fresh):
            self._head(atol)
            if self.hcol > 0:
                self._end_cycle(atol)
        return self._state()

    def _state(self):
        return {"iterations": self.iters, "done": bool(self.done), "converged": bool(self.converged), "breakdown": bool(self.breakdown),
                "inner": bool(self.inner), "cols": self.cols, "cycles": self.cycles, "presid": self.presid, "ptol": self.ptol,
                "factor": self.factor, "rnorm": self.rnorm, "bnorm": self.bnorm, "hcol": self.hcol}

    def history(self, count, ncycles):
        h = (self.hist + [0.0] * int(count))[: int(count)]
        c = (self.chist + [(0.0, 0.0, 0.0)] * int(ncycles))[: int(ncycles)]
        return np.array(h, dtype=np.float64), np.array(c, dtype=np.float64).reshape(int(ncycles), 3)

    def solution(self):
        return self.x.copy()

    def get(self, which):
        if which == "small":
            return {"R": self.R.copy(), "gc": self.gc.copy(), "gs": self.gs.copy(), "S": self.S.copy(), "cols": self.cols, "ptol": self.ptol,
                    "factor": self.factor, "presid": self.presid, "rnorm": self.rnorm, "bnorm": self.bnorm, "inner": self.inner,
                    "breakdown": self.breakdown, "done": self.done, "converged": self.converged, "iters": self.iters, "cycles": self.cycles}
        if which == "rows":
            return self.V[: self.m + 1].copy()
        return getattr(self, which).copy()


class DeviceGmresBackend:
    """The ``lz_gmres_*`` calls on one ``_capi.Handle`` that already holds the matrix."""

    def __init__(self, handle, n):
        self.h = handle
        self.n = n
        self.launches_per_step = handle.gmres_info()["launches_per_step"]

    def begin(self, restart, b, x0):
        self.h.gmres_begin(restart, b, x0)

    def set_state(self, restart, x, b, w, rows, small):
        self.h.gmres_set_state(restart, x, b, w, rows, small)

    def run(self, steps, atol):
        return self.h.gmres_run(steps, atol)

    def end_cycle(self, atol):
        return self.h.gmres_end_cycle(atol)

    def history(self, count, ncycles):
        return self.h.gmres_history(count, ncycles)

    def solution(self):
        return self.h.gmres_get("x")

    def get(self, which):
        return self.h.gmres_get(which)


def solve(backend, b, x0, atol_eff, restart, maxiter, check_every, callback=None, callback_type=None, bnorm=1.0, info=None):
    """The loop over chunks on a backend (``NumpyGmresBackend`` or ``DeviceGmresBackend``) -> ``(x, info_int)``.  ``maxiter`` counts
    restart cycles, or with ``callback_type == 'legacy'`` inner steps.  ``'pr_norm'`` and ``'legacy'`` callbacks receive the backend's
    ``presid / bnorm`` in order, a chunk at a time; ``'x'`` runs one cycle per chunk and fetches ``x`` behind each."""
    m = int(restart)
    legacy = callback_type == "legacy"
    backend.begin(m, b, x0)
    st = backend.run(0, atol_eff)
    chunks = delivered = 0

    def deliver(st):
        nonlocal delivered
        if callback_type in ("legacy", "pr_norm") and st["iterations"] > delivered:
            hist, _ = backend.history(st["iterations"], 0)
            for v in hist[delivered:]:
                callback(v / bnorm)
            delivered = st["iterations"]

    while not st["done"]:
        pending = st["inner"]  # the next call begins with the end of the cycle under way
        if legacy:
            room = maxiter - st["iterations"]
        else:
            room = (maxiter - st["cycles"] - (1 if pending else 0)) * m - (0 if pending else st["hcol"])
            if st["cycles"] >= maxiter:
                break
        if legacy and room <= 0:
            st = backend.end_cycle(atol_eff)  # SciPy's legacy exit: the cycle ends where the count ran out
            chunks += 1
            break
        want = (0 if pending else m - st["hcol"]) if callback_type == "x" else int(check_every)
        before = st["cycles"]
        st = backend.run(max(0, min(want, room)), atol_eff)
        chunks += 1
        deliver(st)
        if callback_type == "x" and st["cycles"] > before:
            callback(backend.solution())
    code = 0 if st["converged"] else int(maxiter)
    kind = "converged" if st["converged"] else "breakdown" if st["breakdown"] and st["done"] else "maxiter"
    x = backend.solution()
    if info is not None:
        hist, chist = backend.history(st["iterations"], st["cycles"])
        info.update({"iterations": st["iterations"], "cycles": st["cycles"], "code": code, "exit": kind, "residual_norm": st["rnorm"],
                     "atol_effective": float(atol_eff), "products": st["iterations"] + st["cycles"] + (0 if x0 is None else 1),
                     "chunks": chunks, "launches_per_step": backend.launches_per_step, "history": hist, "cycle_history": chunk_rows(chist)})
    return x, code


def chunk_rows(chist):
    """``cycle_history``: one dict per cycle"""
    return [{"rnorm": float(r), "cols": int(c), "ptol": float(p)} for r, c, p in np.asarray(chist).reshape(-1, 3)]


def check_gmres_args(A, b, x0, M, restart, maxiter, check_every, rtol, atol, callback, callback_type):
    """``(n, b, x0, restart, maxiter, check_every, callback_type)`` or the error of a bad call - before any device is asked for.  The
    checks of ``A``, ``b``, ``x0``, ``M``, ``maxiter``, ``rtol`` and ``atol`` are ``check_bicgstab_args``'."""
    try:
        n, b, x0, maxiter = check_bicgstab_args(A, b, x0, M, maxiter, 1, rtol, atol)
    except NotImplementedError as e:
        raise NotImplementedError(str(e).replace("bicgstab:", "gmres:")) from None
    if callback is not None and callback_type is None:
        warnings.warn("lanczos_amd.gmres called without specifying `callback_type`. SciPy's default value will be changed in a future "
                      "release. For compatibility, specify a value for `callback_type` explicitly, e.g., "
                      "``gmres(..., callback_type='pr_norm')``, or to retain the old behavior ``gmres(..., callback_type='legacy')``",
                      category=DeprecationWarning, stacklevel=3)
    if callback_type is None:
        callback_type = "legacy"
    if callback_type not in ("x", "pr_norm", "legacy"):
        raise ValueError(f"Unknown callback_type: {callback_type!r}")
    if callback is None:
        callback_type = None
    restart = 20 if restart is None else int(restart)
    if restart < 1:
        raise ValueError("restart must be at least 1")
    restart = min(restart, n)
    if restart > MAX_RESTART:
        raise ValueError(f"restart must be at most {MAX_RESTART} (the basis holds {MAX_RESTART} + 1 rows)")
    check_every = min(restart, 4) if check_every is None else int(check_every)
    if check_every < 1:
        raise ValueError("check_every must be at least 1")
    return n, b, x0, restart, maxiter, check_every, callback_type


def gmres(A, b, x0=None, *, rtol=1e-5, atol=0.0, restart=None, maxiter=None, M=None, callback=None, callback_type=None, check_every=None,
          device_id=0, handle=None, info=None, _backend=None):
    """Solve ``A x = b`` for a real square ``A`` by restarted GMRES on the GPU - ``scipy.sparse.linalg.gmres``' signature, defaults,
    return value and rules (SciPy 1.15).  Returns ``(x, info_int)``: ``x`` is ``(n,)`` float64; ``info_int`` is 0 when the true residual
    met ``|b - A x| <= max(atol, rtol |b|)`` and ``maxiter`` otherwise.

    ``A``: what ``bicgstab`` takes - any SciPy sparse format, a dense ndarray, ``synthetic.CSR`` or ``StencilOperator``.  ``b``: ``(n,)``
    or ``(n, 1)``, real; ``b = 0`` returns zeros and 0.  ``x0``: the starting guess (an all-zero one is no guess: ``r = b`` without a
    product).  ``restart``: default 20, clipped to ``n``.  ``maxiter``: default ``10 n``, counted in restart cycles (with
    ``callback_type='legacy'`` in inner steps, and the cycle ends where the count runs out, as in SciPy).  The first test is
    ``|r| < atol_eff``; every later one is on the true residual formed at the end of a cycle.  The inner tolerance follows SciPy's rule
    (module docstring); the inner loop also ends on the breakdown indicator ``h1 <= eps h0``, and after a breakdown the solve ends.
    ``callback_type``: ``'x'`` (``callback(x)`` behind every cycle), ``'pr_norm'`` or ``'legacy'`` (``callback(presid / |b|)`` for every
    inner step); a callback without a type raises SciPy's ``DeprecationWarning`` and means ``'legacy'``; an unknown type is a
    ``ValueError``.

    Deliberate deviations from SciPy.  The orthogonalisation is the basis layer's classical Gram-Schmidt with the DGKS second pass, not
    modified Gram-Schmidt: results agree to rounding, not bit for bit.  ``restart`` above 128 (after the clip to ``n``) raises
    ``ValueError``: the basis holds at most 128 + 1 rows.  ``'pr_norm'`` and ``'legacy'`` callbacks are delivered in order with the
    device's ``presid / |b|`` values, but a chunk at a time, after the chunk's synchronisation.  ``'x'`` runs one cycle per
    synchronisation and downloads ``x`` behind each: the slow path.  Past the inner exit the rest of a chunk's products still run.

    ``M`` (preconditioning), complex ``A`` / ``b`` / ``x0`` and a ``LinearOperator`` raise ``NotImplementedError``; shape and value
    errors raise ``ValueError``; all of them before any device is asked for.  ``n == 1`` is answered on the host.
    ``check_every`` (default ``min(restart, 4)``, the fastest of 4 / 8 / ``restart`` measured, profiles/r30/gmres_probe.json): inner steps
    enqueued between two host synchronisations, cycle ends and restarts included; past the inner exit the rest of a chunk - up to
    ``check_every - 1`` products and Gram-Schmidt steps - still runs and changes nothing.  ``x`` does not depend on it.
    ``handle``: an open ``_capi.Handle`` to run on (its square matrix is replaced; its thick-restart basis is left alone); ``info``: a
    dict that receives ``iterations`` (inner), ``cycles``, ``code``, ``exit`` (``"converged"``, ``"breakdown"`` or ``"maxiter"``),
    ``residual_norm`` (the device's true ``|b - A x|``), ``atol_effective``, ``products``, ``chunks``, ``launches_per_step``, ``history``
    (``presid`` of every inner step) and ``cycle_history`` (``rnorm``, ``cols`` and ``ptol`` of every cycle)."""
    n, b, x0, restart, maxiter, check_every, callback_type = check_gmres_args(A, b, x0, M, restart, maxiter, check_every, rtol, atol,
                                                                              callback, callback_type)
    bnorm = float(np.linalg.norm(b))
    atol_eff = max(float(atol), float(rtol) * bnorm)
    if x0 is not None and not np.any(x0):
        x0 = None
    run = {"iterations": 0, "cycles": 0, "code": 0, "exit": "converged", "residual_norm": 0.0, "atol_effective": atol_eff, "products": 0,
           "chunks": 0, "launches_per_step": None, "history": np.zeros(0), "cycle_history": []}
    if bnorm == 0.0:
        x, code = np.zeros(n), 0
    elif n == 1:
        x, code = b / float(_entry00(A)), 0
        if callback_type == "x":
            callback(x.copy())
    elif _backend is not None:  # the host tests' way in: a NumpyGmresBackend
        x, code = solve(_backend, b, x0, atol_eff, restart, maxiter, check_every, callback, callback_type, bnorm, run)
    else:
        from . import _capi

        h = handle if handle is not None else _capi.Handle(device_id)
        try:
            upload_matrix(h, A)
            x, code = solve(DeviceGmresBackend(h, n), b, x0, atol_eff, restart, maxiter, check_every, callback, callback_type, bnorm, run)
        finally:
            if handle is None:
                h.close()
    if info is not None:
        info.update(run)
    return np.asarray(x, dtype=np.float64).reshape(n), code
