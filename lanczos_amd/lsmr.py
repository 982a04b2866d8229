"""``lsmr``: least-squares solves ``min |A x - b|`` or ``min |A x - b|^2 + damp^2 |x|^2`` for a rectangular or non-symmetric ``A`` on the GPU.

LSMR (Fong & Saunders 2011) is Golub-Kahan bidiagonalisation with no basis kept and MINRES on the normal equations done implicitly:
``A^T A`` is never formed and the condition number is not squared.  The loop is ``scipy.sparse.linalg.lsmr``'s, scalar for scalar -
the same ``_sym_ortho``, the same estimates of ``|r|``, ``|A^T r|``, ``|A|`` and ``cond(A)``, the same ``istop`` codes.  From
``u_1 = (b - A x0) / beta_1``, ``v_1 = A^T u_1 / alpha_1``, ``h = v_1``, ``hbar = 0`` step ``k = 1, 2, ...`` is

    beta_{k+1} u_{k+1} = A v_k - alpha_k u_k              alpha_{k+1} v_{k+1} = A^T u_{k+1} - beta_{k+1} v_k
    the rotations (Qhat for damp, Q, Qbar) -> rho, rhobar, thetanew, thetabar, zeta, zetabar
    hbar = h - (thetabar rho / (rho_old rhobar_old)) hbar;   x += (zeta / (rho rhobar)) hbar;   h = v_{k+1} - (thetanew / rho) h
    normr, normar = |zetabar|, normA, condA and the tests on them

On the device (``lz_lsmr_*`` in include/lanczos_hip.h) the scalars never leave it inside a chunk of
``check_every`` steps: two one-block kernels form ``beta``, ``alpha``, the rotations and the tests and set a flag that gates the rest
of the chunk.  ``u`` and ``v`` are kept un-normalised with the numbers to divide by, and every kernel divides where it reads.  The
update of ``hbar``, ``x`` and ``h`` rides one step behind in the streaming pass that forms ``v``, because its scalars depend on
``alpha_{k+1}``; the pending update is applied when a chunk ends.

The one deviation from SciPy.  SciPy forms ``|x_k|`` by a pass over ``x`` at every step and uses it in tests 1 and 4
(``rtol = btol + atol |A| |x| / |b|`` and ``t1``).  On the device ``x_k`` does not exist until the next pass, so the tests of step
``k`` use ``|x_{k-1}|``, which falls out of the lagged pass.  Without ``x0`` ``|x_k|`` is non-decreasing for LSMR, so in exact
arithmetic this rule never stops earlier than SciPy's.  The returned ``normx`` is the true norm of the returned ``x``.

``solve`` below is the host loop over chunks; it runs on ``DeviceLsmrBackend`` and on ``NumpyLsmrBackend``, a host restatement of
the same calls with the same lag and the same rule, which the host tests drive.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse

from .svds import _pack


def _sign(a):
    return 1.0 if a > 0.0 else -1.0 if a < 0.0 else a


def _sym_ortho(a, b):
    """SciPy's stable Givens rotation: ``(c, s, r)`` with ``c a + s b = r``"""
    if b == 0.0:
        return _sign(a), 0.0, abs(a)
    if a == 0.0:
        return 0.0, _sign(b), abs(b)
    if abs(b) > abs(a):
        tau = a / b
        s = _sign(b) / math.sqrt(1.0 + tau * tau)
        return s * tau, s, b / s
    tau = b / a
    c = _sign(a) / math.sqrt(1.0 + tau * tau)
    return c, c * tau, a / c


def _div(a, b):
    """float division as the device does it: no exception, inf or NaN instead"""
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else math.nan


SCALARS = ("alpha", "beta", "alphabar", "rho", "rhobar", "cbar", "sbar", "zeta", "zetabar", "betadd", "betad", "rhodold", "tautildeold",
           "thetatilde", "d", "normA2", "maxrbar", "minrbar", "damp", "normb", "c1", "c2", "c3")


def initial_scalars(alpha, beta, damp, normb):
    """the scalars step 1 starts from; the pending update is the empty one"""
    s = dict.fromkeys(SCALARS, 0.0)
    s.update({"alpha": alpha, "beta": beta, "alphabar": alpha, "rho": 1.0, "rhobar": 1.0, "cbar": 1.0, "zetabar": alpha * beta,
              "betadd": beta, "rhodold": 1.0, "normA2": alpha * alpha, "minrbar": 1e100, "damp": damp, "normb": normb,
              "normr": beta, "normar": alpha * beta, "normA": math.sqrt(alpha * alpha), "condA": 1.0, "normx_lagged": 0.0})
    return s


def scalar_step(s, alpha, beta, normx, itn, atol, btol, ctol):
    """the body of SciPy's loop behind its two products, on the dict ``s`` (``k_lsmr_scalars``): ``alpha``, ``beta`` are those of step
    ``itn + 1``, ``normx`` the norm the tests use.  Returns ``istop`` (0: go on)."""
    damp, normb = s["damp"], s["normb"]
    chat, shat, alphahat = _sym_ortho(s["alphabar"], damp)
    rhoold = s["rho"]
    c, sn, rho = _sym_ortho(alphahat, beta)
    thetanew = sn * alpha
    alphabar = c * alpha
    rhobarold, zetaold = s["rhobar"], s["zeta"]
    thetabar = s["sbar"] * rho
    rhotemp = s["cbar"] * rho
    cbar, sbar, rhobar = _sym_ortho(s["cbar"] * rho, thetanew)
    zeta = cbar * s["zetabar"]
    zetabar = -sbar * s["zetabar"]
    s["c1"] = _div(thetabar * rho, rhoold * rhobarold)
    s["c2"] = _div(zeta, rho * rhobar)
    s["c3"] = _div(thetanew, rho)
    betaacute = chat * s["betadd"]
    betacheck = -shat * s["betadd"]
    betahat = c * betaacute
    betadd = -sn * betaacute
    thetatildeold = s["thetatilde"]
    ctildeold, stildeold, rhotildeold = _sym_ortho(s["rhodold"], thetabar)
    thetatilde = stildeold * rhobar
    rhodold = ctildeold * rhobar
    betad = -stildeold * s["betad"] + ctildeold * betahat
    tautildeold = _div(zetaold - thetatildeold * s["tautildeold"], rhotildeold)
    taud = _div(zeta - thetatilde * tautildeold, rhodold)
    d = s["d"] + betacheck * betacheck
    normr = _sqrt(d + (betad - taud) * (betad - taud) + betadd * betadd)
    normA2 = s["normA2"] + beta * beta
    normA = _sqrt(normA2)
    normA2 = normA2 + alpha * alpha
    maxrbar = max(s["maxrbar"], rhobarold)
    minrbar = s["minrbar"]
    if itn > 1:
        minrbar = min(minrbar, rhobarold)
    condA = _div(max(maxrbar, rhotemp), min(minrbar, rhotemp))
    normar = abs(zetabar)
    test1 = _div(normr, normb)
    test2 = _div(normar, normA * normr) if normA * normr != 0.0 else math.inf
    test3 = _div(1.0, condA)
    t1 = _div(test1, 1.0 + _div(normA * normx, normb))
    rtol = btol + _div(atol * normA * normx, normb)
    istop = 0
    if 1.0 + test3 <= 1.0:
        istop = 6
    if 1.0 + test2 <= 1.0:
        istop = 5
    if 1.0 + t1 <= 1.0:
        istop = 4
    if test3 <= ctol:
        istop = 3
    if test2 <= atol:
        istop = 2
    if test1 <= rtol:
        istop = 1
    s.update({"alpha": alpha, "beta": beta, "alphabar": alphabar, "rho": rho, "rhobar": rhobar, "cbar": cbar, "sbar": sbar, "zeta": zeta,
              "zetabar": zetabar, "betadd": betadd, "betad": betad, "rhodold": rhodold, "tautildeold": tautildeold,
              "thetatilde": thetatilde, "d": d, "normA2": normA2, "maxrbar": maxrbar, "minrbar": minrbar, "normr": normr,
              "normar": normar, "normA": normA, "condA": condA, "normx_lagged": normx})
    return istop


class NumpyLsmrBackend:
    """The calls of ``DeviceLsmrBackend`` in NumPy - the un-normalised ``u`` and ``v`` with their divisors, the lag of the update, the
    flush and the rule of ``|x_{k-1}|`` included: what the host tests drive ``solve`` with.  ``A`` is ``M x N`` as the caller holds it."""

    own_launches_per_iteration = None
    plan = None
    transposed = False

    def __init__(self, A):
        self.A = A if scipy.sparse.issparse(A) else np.asarray(A, dtype=np.float64)
        self.AT = self.A.T.tocsr() if scipy.sparse.issparse(A) else self.A.T
        self.m, self.n = self.A.shape

    def begin(self, b, x0, damp):
        b = np.asarray(b, dtype=np.float64)
        with np.errstate(all="ignore"):
            self.x = np.zeros(self.n) if x0 is None else np.array(x0, dtype=np.float64)
            self.uh = b.copy() if x0 is None else b - self.A @ self.x
            normb = float(np.sqrt(b @ b))
            beta = float(np.sqrt(self.uh @ self.uh))
            self.nu_u = beta if beta > 0.0 else 1.0
            self.vh, self.nu_v, alpha = np.zeros(self.n), 1.0, 0.0
            if beta > 0.0 and np.isfinite(beta):
                self.vh = (self.AT @ self.uh) / self.nu_u
                alpha = float(np.sqrt(self.vh @ self.vh))
                self.nu_v = alpha if alpha > 0.0 else 1.0
        self.h, self.hbar = np.zeros(self.n), np.zeros(self.n)
        self.s = initial_scalars(alpha, beta, float(damp), normb)
        finite = bool(np.isfinite(beta) and np.isfinite(alpha) and np.isfinite(normb))
        self.done = not finite or alpha * beta == 0.0 or normb == 0.0
        self.istop = 0 if finite else 7
        self.fresh = True  # the empty pending update: it makes h_1 = v_1
        self.normx2 = float(self.x @ self.x)
        self.steps = 0
        self.hist = []

    def _update(self):
        """the end of the step before: ``hbar``, ``x``, ``h`` from ``v_k = vh / nu_v``; returns ``|x|^2``"""
        vk = self.vh / self.nu_v
        self.hbar = self.h - self.s["c1"] * self.hbar
        self.x = self.x + self.s["c2"] * self.hbar
        self.h = vk - self.s["c3"] * self.h
        self.fresh = False
        self.normx2 = float(self.x @ self.x)

    def run(self, iters, atol, btol, conlim):
        ctol = 1.0 / conlim if conlim > 0 else 0.0
        s = self.s
        with np.errstate(all="ignore"):  # (a breakdown divides by a vanished number, as the device does)
            for _ in range(int(iters) if not self.done else 0):
                y = self.A @ self.vh
                self.uh = y / self.nu_v - s["alpha"] * (self.uh / self.nu_u)  # k_lsmr_u
                beta = float(np.sqrt(self.uh @ self.uh))  # k_lsmr_beta
                if not np.isfinite(beta):
                    self.done, self.istop = True, 7
                    break
                nu_u = beta if beta > 0.0 else 1.0
                alpha = s["alpha"]
                vh, nu_v = self.vh, self.nu_v
                if beta > 0.0:  # k_lsmr_v, the three-term
                    z = self.AT @ self.uh
                    vh = z / nu_u - beta * (self.vh / self.nu_v)
                if self.fresh:  # ... and the end of the step before, from the same load of vh
                    self._update()
                self.nu_u = nu_u
                if beta > 0.0:  # k_lsmr_scalars
                    alpha = float(np.sqrt(vh @ vh))
                    if not np.isfinite(alpha):
                        self.done, self.istop = True, 7
                        break
                    self.vh, self.nu_v = vh, (alpha if alpha > 0.0 else 1.0)
                self.steps += 1
                istop = scalar_step(s, alpha, beta, math.sqrt(self.normx2), self.steps, atol, btol, ctol)
                self.hist.append((s["normr"], s["normar"]))
                self.fresh = True
                if istop:
                    self.done, self.istop = True, istop
                    break
            if self.fresh and int(iters) > 0:
                self._update()  # the flush
        return self._state()

    def _state(self):
        s = self.s
        return {"iterations": self.steps, "done": bool(self.done), "istop": int(self.istop), "normr": s["normr"], "normar": s["normar"],
                "normA": s["normA"], "condA": s["condA"], "normx": math.sqrt(self.normx2), "alpha": s["alpha"], "beta": s["beta"],
                "rho": s["rho"], "rhobar": s["rhobar"], "zeta": s["zeta"], "zetabar": s["zetabar"], "normx_lagged": s["normx_lagged"],
                "normb": s["normb"]}

    def history(self, count):
        return np.array(self.hist[:count], dtype=np.float64).reshape(-1, 2)

    def solution(self):
        return self.x.copy()


class DeviceLsmrBackend:
    """The ``lz_lsmr_*`` calls on one ``_capi.Handle`` that already holds the rectangular matrix (``gk_set_csr`` or ``gk_set_dense``)."""

    def __init__(self, handle, transposed, plan=None):
        self.h = handle
        self.transposed = bool(transposed)
        self.plan = plan
        self.own_launches_per_iteration = handle.lsmr_info()["own_launches_per_iteration"]

    def begin(self, b, x0, damp):
        self.h.lsmr_begin(b, x0, damp, transposed=self.transposed)

    def run(self, iters, atol, btol, conlim):
        return self.h.lsmr_run(iters, atol, btol, conlim)

    def history(self, count):
        return self.h.lsmr_history(count)

    def solution(self):
        return self.h.lsmr_get("x")


def solve(backend, b, x0, damp, atol, btol, conlim, maxiter, check_every, show=False, info=None):
    """The loop over chunks on a backend (``NumpyLsmrBackend`` or ``DeviceLsmrBackend``) -> SciPy's 8-tuple"""
    backend.begin(b, x0, damp)
    st = backend.run(0, atol, btol, conlim)
    chunks = 0
    while not st["done"] and st["iterations"] < maxiter:
        st = backend.run(min(int(check_every), maxiter - st["iterations"]), atol, btol, conlim)
        chunks += 1
        if show:
            print(f"lsmr: chunk {chunks:5d}  iterations {st['iterations']:7d}  normr {st['normr']:.3e}  normar {st['normar']:.3e}  "
                  f"normA {st['normA']:.2e}  condA {st['condA']:.2e}")
    x = backend.solution()
    itn = st["iterations"]
    istop = st["istop"] if st["done"] or itn == 0 else 7  # 7 is the host's: the steps ran out and the flag is clear
    if show:
        print(f"lsmr: istop {istop}  itn {itn}  normr {st['normr']:.3e}  normar {st['normar']:.3e}")
    if info is not None:
        info.update({"iterations": itn, "chunks": chunks, "plan": backend.plan, "transposed": backend.transposed,
                     "own_launches_per_iteration": backend.own_launches_per_iteration, "history": backend.history(itn)})
    return x, int(istop), int(itn), st["normr"], st["normar"], st["normA"], st["condA"], st["normx"]


def _is_complex(a):
    return np.iscomplexobj(a) if not scipy.sparse.issparse(a) else a.dtype.kind == "c"


def check_lsmr_args(A, b, damp, atol, btol, maxiter, x0, check_every):
    """``(A, M, N, b as (M,) float64, x0 as (N,) float64 or None, maxiter)`` or the error of a bad call - before any device is asked for"""
    if not scipy.sparse.issparse(A):
        if hasattr(A, "matvec") and not isinstance(A, np.ndarray):
            raise NotImplementedError("lsmr: LinearOperator input is not implemented (a SciPy sparse matrix or a dense array)")
        A = np.asarray(A)
    if len(A.shape) != 2:
        raise ValueError(f"expected a matrix (shape={A.shape})")
    if _is_complex(A):
        raise NotImplementedError("lsmr: complex A is not implemented (real matrices only)")
    M, N = (int(v) for v in A.shape)
    if M < 1 or N < 1:
        raise ValueError(f"expected a matrix with at least one row and one column (shape={A.shape})")
    b = np.asarray(b)
    if np.iscomplexobj(b):
        raise NotImplementedError("lsmr: complex b is not implemented")
    if not (b.shape == (M,) or b.shape == (M, 1)):
        raise ValueError(f"shapes of A {A.shape} and b {b.shape} are incompatible")
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(M)
    if x0 is not None:
        x0 = np.asarray(x0)
        if np.iscomplexobj(x0):
            raise NotImplementedError("lsmr: complex x0 is not implemented")
        if not (x0.shape == (N,) or x0.shape == (N, 1)):
            raise ValueError(f"shapes of A {A.shape} and x0 {x0.shape} are incompatible")
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(N)
    for name, val in (("damp", damp), ("atol", atol), ("btol", btol)):
        if not float(val) >= 0.0:
            raise ValueError(f"{name} must be non-negative")
    if maxiter is not None and int(maxiter) < 0:
        raise ValueError("maxiter must be non-negative")
    maxiter = min(M, N) if maxiter is None else int(maxiter)
    if int(check_every) < 1:
        raise ValueError("check_every must be at least 1")
    return A, M, N, b, x0, maxiter


def _closed_form(A, b, x0, damp, atol, btol):
    """``min(M, N) == 1`` on the host: the rectangular operator on the device needs both sides of length 2 at least"""
    a = np.asarray(A.toarray() if scipy.sparse.issparse(A) else A, dtype=np.float64)
    x = np.zeros(a.shape[1]) if x0 is None else x0.copy()
    r0 = b - a @ x
    if a.shape[1] == 1:  # one unknown: a^T r0 / (a^T a + damp^2)
        col = a[:, 0]
        den = float(col @ col) + damp * damp
        dx = np.array([float(col @ r0) / den]) if den > 0.0 else np.zeros(1)
    else:  # one equation: the minimum-norm a^T r0 / (a a^T + damp^2)
        row = a[0]
        den = float(row @ row) + damp * damp
        dx = row * (r0[0] / den) if den > 0.0 else np.zeros(a.shape[1])
    normA = float(np.linalg.norm(a))
    if not np.any(a.T @ r0):
        return x, 0, 0, float(np.linalg.norm(r0)), 0.0, normA, 1.0, float(np.linalg.norm(x))
    x = x + dx
    r = b - a @ x
    normr = float(np.sqrt(r @ r + damp * damp * (dx @ dx)))
    normar = float(np.linalg.norm(a.T @ r - damp * damp * dx))
    normx = float(np.linalg.norm(x))
    istop = 1 if normr <= btol * np.linalg.norm(b) + atol * normA * normx else 2
    return x, istop, 1, normr, normar, normA, 1.0, normx


def lsmr(A, b, damp=0.0, atol=1e-6, btol=1e-6, conlim=1e8, maxiter=None, show=False, x0=None, *, check_every=8, device_id=0, handle=None,
         info=None, _backend=None):
    """Solve ``min |A x - b|^2 + damp^2 |x|^2`` for a real ``M x N`` matrix ``A`` - ``scipy.sparse.linalg.lsmr``'s positional signature,
    defaults and 8-tuple - by LSMR on the GPU.  Returns ``(x, istop, itn, normr, normar, normA, condA, normx)``: ``x`` is ``(N,)``
    float64; ``istop`` has SciPy's meaning (0: ``x0`` or zero is the solution, 1: ``|r| <= btol |b| + atol |A| |x|``, 2:
    ``|A^T r| <= atol |A| |r|``, 3: ``cond(A) >= conlim``, 4 / 5 / 6: the same three at machine precision, 7: ``maxiter`` steps ran);
    ``normr`` estimates ``|[b - A x; -damp x]|``, ``normar`` the norm of the normal equations' residual, ``normA`` the Frobenius norm
    of ``[A; damp I]`` and ``condA`` its condition; ``normx`` is ``|x|`` of the returned ``x``.

    ``A``: what ``svds`` takes - any SciPy sparse format or a dense ndarray; float32 is converted to float64 with a notice.  A dense
    array stays dense on the device unless ``12 count_nonzero(A) < 8 A.size`` (then its CSR is the smaller stream); a C- or
    F-contiguous float64 array is uploaded as it lies in memory.  ``b``: ``(M,)`` or ``(M, 1)``; ``x0``: ``(N,)`` or ``(N, 1)`` - the
    iteration then runs on ``b - A x0`` and, with ``damp``, regularises the correction, as SciPy's does.  Complex ``A``, ``b`` or
    ``x0`` and a ``LinearOperator`` raise ``NotImplementedError``; a shape mismatch, a negative ``damp`` / ``atol`` / ``btol`` /
    ``maxiter`` or ``check_every < 1`` raise ``ValueError``; all of them before any device is asked for.  ``maxiter`` defaults to
    ``min(M, N)``.  ``b = 0`` returns zeros with ``istop = 0``; ``A^T (b - A x0) = 0`` returns ``x0`` (or zeros) with ``istop = 0``;
    ``min(M, N) == 1`` is answered on the host in closed form.

    The stopping tests deviate from SciPy's in one point: those of step ``k`` use ``|x_{k-1}|`` where SciPy uses ``|x_k|`` (module
    docstring).  Without ``x0`` ``|x_k|`` is non-decreasing for LSMR, so in exact arithmetic this never stops earlier than SciPy's
    rule.  A ``beta`` or ``alpha`` that is not finite stops at once and reports 7.

    ``check_every`` (default 8): steps enqueued between two host synchronisations; past the stopping step the rest of a chunk is
    gated off on the device, but its products still run.  ``x`` does not depend on it.  ``show``: one line per chunk.  ``handle``: an
    open ``_capi.Handle`` to run on - its rectangular (``svds``) matrix is replaced; its square matrix, thick-restart basis and MINRES
    state are left alone.  ``info``: a dict that receives ``iterations``, ``chunks``, ``plan`` (``"dense"`` or ``"csr"``),
    ``transposed`` (the device holds ``A^T``, the tall orientation), ``own_launches_per_iteration`` (beside the two products) and
    ``history`` (``(itn, 2)``: ``normr``, ``normar`` per step).
    Several right-hand sides, preconditioning and more than one GPU are out of scope."""
    A, M, N, b, x0, maxiter = check_lsmr_args(A, b, damp, atol, btol, maxiter, x0, check_every)
    damp, atol, btol, conlim = float(damp), float(atol), float(btol), float(conlim)
    run = {"iterations": 0, "chunks": 0, "plan": None, "transposed": False, "own_launches_per_iteration": None, "history": np.zeros((0, 2))}
    if not np.any(b):
        out = (np.zeros(N), 0, 0, 0.0, 0.0, 0.0, 1.0, 0.0)
    elif min(M, N) == 1:
        out = _closed_form(A, b, x0, damp, atol, btol)
        run["iterations"] = out[2]
    elif _backend is not None:  # the host tests' way in: a NumpyLsmrBackend
        out = solve(_backend, b, x0, damp, atol, btol, conlim, maxiter, check_every, show, run)
    else:
        Aop, AopT, transposed = _pack(A)
        from . import _capi

        h = handle if handle is not None else _capi.Handle(device_id)
        try:
            if isinstance(Aop, np.ndarray):  # one dense copy: whichever of the two views is C-contiguous, as it lies in memory
                wide = not Aop.flags.c_contiguous
                h.gk_set_dense(AopT if wide else Aop, stored_transposed=wide)
            else:
                h.gk_set_csr(Aop, AopT)
            backend = DeviceLsmrBackend(h, transposed, "dense" if isinstance(Aop, np.ndarray) else "csr")
            out = solve(backend, b, x0, damp, atol, btol, conlim, maxiter, check_every, show, run)
        finally:
            if handle is None:
                h.close()
    if info is not None:
        info.update(run)
    return (np.asarray(out[0], dtype=np.float64).reshape(N),) + tuple(out[1:])
