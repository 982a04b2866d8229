"""References for the ``gmres`` tests: SciPy's restarted GMRES loop (lanczos_amd/gmres.py's docstring; modified Gram-Schmidt, as SciPy
runs it) in ``np.longdouble`` and in float64 with three summation orders, every tested number recorded; SciPy's own ``gmres`` as a
further run; the admission rule that keeps every test off its threshold; and the forward-error bounds of the new kernels - the rotated
column and ``S``, the triangular solve, ``x += y . V`` and the residual norm - derived from ``gamma(L)``.  Nothing here imports the
package."""
import warnings

import numpy as np
import scipy.sparse.linalg as sla

from bicgstab_reference import EPS, LD, ORDERS, Operator, _dots, dot_bound, gamma, norm_bound  # noqa: F401


def lartg_any(f, g, dt):
    """``(c, s, r)`` with LAPACK lartg's signs, in ``dt`` (no scaling: the references' numbers are of order one)"""
    f, g = dt(f), dt(g)
    if g == 0:
        return dt(1.0), dt(0.0), f
    if f == 0:
        return dt(0.0), dt(np.sign(g)), abs(g)
    d = np.sqrt(f * f + g * g)
    r = d if f > 0 else -d
    return abs(f) / d, g / r, r


def pseudo_solve(R, S, cols):
    """SciPy's pseudo-solve; ``R[j, :j + 1]`` is column ``j`` of the triangle"""
    col = cols - 1
    if R[col, col] == 0:
        S[col] = 0
    y = S[:cols].copy()
    for k in range(col, 0, -1):
        if y[k] != 0:
            y[k] = y[k] / R[k, k]
            y[:k] = y[:k] - y[k] * R[k, :k]
    if y[0] != 0:
        y[0] = y[0] / R[0, 0]
    return y


def loop(A, b, atol_eff, restart, maxiter, order="longdouble", x0=None, op=None):
    """SciPy's loop (``maxiter`` in cycles; no callback); float64 with the inner products summed in ``order``, or everything in
    longdouble.  Returns ``code``, ``iterations`` (inner), ``cycles``, ``x``, ``cols`` (per cycle), ``breakdown``, ``branches`` (per cycle
    that went on: ``"tighten"`` where the inner test passed but the outer one did not, else ``"relax"``) and ``tests``: every tested
    number as ``("p", cycle, col, presid, ptol)`` or ``("r", cycle, rnorm, atol_eff)`` (cycle -1: the first test)."""
    ld = order == "longdouble"
    dt = LD if ld else np.float64
    dot = _dots(order)
    if ld:
        op = op if op is not None else Operator(A)
        mv = op.matvec
    else:
        mv = lambda v: np.asarray(A @ v)  # noqa: E731
    n = len(b)
    m = min(int(restart), n)
    b = np.asarray(b, dtype=dt)
    x = np.zeros(n, dtype=dt) if x0 is None else np.array(x0, dtype=dt)
    bnorm = np.sqrt(dot(b, b))
    tests, cols_log, branches = [], [], []
    out = {"iterations": 0, "cycles": 0, "breakdown": False}

    def end(code):
        out.update({"code": code, "x": x, "tests": tests, "cols": cols_log, "branches": branches})
        return out

    factor = dt(1.0)
    ptol = bnorm * min(dt(1.0), atol_eff / bnorm)
    presid = dt(0.0)
    v = np.zeros((m + 1, n), dtype=dt)
    h = np.zeros((m, m + 1), dtype=dt)
    giv = np.zeros((m, 2), dtype=dt)
    rnorm = None
    with np.errstate(all="ignore"):
        for it in range(maxiter):
            if it == 0:
                r = b - mv(x) if np.any(x) else b.copy()
                rn = np.sqrt(dot(r, r))
                tests.append(("r", -1, float(rn), float(atol_eff)))
                if rn < atol_eff:
                    return end(0)
            tmp = np.sqrt(dot(r, r))
            v[0] = r * (1 / tmp)
            S = np.zeros(m + 1, dtype=dt)
            S[0] = tmp
            breakdown = False
            for col in range(m):
                w = np.asarray(mv(v[col]), dtype=dt).copy()
                h0 = np.sqrt(dot(w, w))
                for k in range(col + 1):
                    t = dot(v[k], w)
                    h[col, k] = t
                    w = w - t * v[k]
                h1 = np.sqrt(dot(w, w))
                h[col, col + 1] = h1
                v[col + 1] = w
                if h1 <= EPS * h0:
                    h[col, col + 1] = 0
                    breakdown = True
                else:
                    v[col + 1] = w * (1 / h1)
                for k in range(col):
                    c, s = giv[k]
                    n0, n1 = h[col, k], h[col, k + 1]
                    h[col, k], h[col, k + 1] = c * n0 + s * n1, -s * n0 + c * n1
                c, s, mag = lartg_any(h[col, col], h[col, col + 1], dt)
                giv[col] = c, s
                h[col, col], h[col, col + 1] = mag, 0
                t = -s * S[col]
                S[col], S[col + 1] = c * S[col], t
                presid = abs(t)
                out["iterations"] += 1
                tests.append(("p", it, col, float(presid), float(ptol)))
                if presid <= ptol or breakdown:
                    break
            y = pseudo_solve(h, S, col + 1)
            x = x + y @ v[: col + 1]
            r = b - mv(x)
            rnorm = np.sqrt(dot(r, r))
            out["cycles"] += 1
            cols_log.append(col + 1)
            tests.append(("r", it, float(rnorm), float(atol_eff)))
            if rnorm <= atol_eff:
                break
            if breakdown:
                out["breakdown"] = True
                break
            if presid <= ptol:
                factor = max(dt(EPS), dt(0.25) * factor)
                branches.append("tighten")
            else:
                factor = min(dt(1.0), dt(1.5) * factor)
                branches.append("relax")
            ptol = presid * min(factor, atol_eff / rnorm)
    return end(0 if rnorm is not None and rnorm <= atol_eff else maxiter)


def scipy_run(A, b, rtol, restart, maxiter=None, x0=None, atol=0.0):
    """SciPy's own ``gmres`` (modified Gram-Schmidt): ``x``, ``code``, inner ``iterations``, ``cycles`` and the ``pr_norm`` values"""
    pr, xs = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, code = sla.gmres(A, b, x0=x0, rtol=rtol, atol=atol, restart=restart, maxiter=maxiter, callback=pr.append, callback_type="pr_norm")
        sla.gmres(A, b, x0=x0, rtol=rtol, atol=atol, restart=restart, maxiter=maxiter, callback=lambda xk: xs.append(1), callback_type="x")
    return {"x": x, "code": code, "iterations": len(pr), "cycles": len(xs), "pr_norm": np.array(pr)}


def admission(A, b, rtol, restart, maxiter=None, x0=None):
    """The four reference runs of a case, SciPy's own run, and whether the case is admitted: all runs take the same inner exits in the
    same cycles and the same number of cycles (SciPy's run, whose cycles cannot be seen from outside one at a time: the same totals of
    inner steps and cycles and the same code), and every tested ``presid`` against its ``ptol`` and every ``rnorm`` against
    ``atol_eff`` keeps a relative margin of at least ``max(0.05, 1000 x the runs' spread at that test)``.  Margin and spread are both
    measured in units of the threshold (the tested number over its threshold, against 1): where a test is anywhere near its threshold
    that is bicgstab_reference's spread relative to the tested numbers' mean, and where the tested number is rounding noise far below
    the threshold (``presid`` of the step that solves ``skew64`` exactly) it still says how far the runs are from flipping the test,
    which a spread relative to a mean of nearly zero does not.  ``x_spread``: the largest distance (2-norm) between two of the five
    solutions."""
    n = len(b)
    atol_eff = rtol * float(np.linalg.norm(b))
    maxiter = 10 * n if maxiter is None else maxiter
    op = Operator(A)
    runs = [loop(A, b, atol_eff, restart, maxiter, order, x0=x0, op=op) for order in ORDERS]
    sc = scipy_run(A, b, rtol, restart, maxiter, x0=x0)
    r0 = runs[0]
    same = all((r["code"], r["iterations"], r["cycles"], r["cols"], r["breakdown"], len(r["tests"])) ==
               (r0["code"], r0["iterations"], r0["cycles"], r0["cols"], r0["breakdown"], len(r0["tests"])) for r in runs)
    same = same and (sc["code"], sc["iterations"], sc["cycles"]) == (r0["code"], r0["iterations"], r0["cycles"])
    worst_margin, worst_spread = np.inf, 0.0
    ok = same
    if same:
        for i in range(len(r0["tests"])):
            ratios = np.array([r["tests"][i][-2] / r["tests"][i][-1] for r in runs])  # the tested number over its threshold
            spread = float(ratios.max() - ratios.min())  # (relative to the threshold, as the margin is)
            margin = float(np.min(np.abs(ratios - 1.0)))
            if not margin >= max(0.05, 1000.0 * spread):
                ok = False
            worst_margin, worst_spread = min(worst_margin, margin), max(worst_spread, spread)
    xs = [np.asarray(r["x"], dtype=LD) for r in runs] + [np.asarray(sc["x"], dtype=LD)]
    x_spread = max(float(np.linalg.norm(np.asarray(xs[i] - xs[j], dtype=np.float64))) for i in range(5) for j in range(i))
    return {"admitted": ok, "same_stop": same, "margin": worst_margin, "spread": worst_spread, "x_spread": x_spread, "atol_eff": atol_eff,
            "runs": dict(zip(ORDERS, runs)), "scipy": sc}


# ---------------------------------------------------------------- forward bounds of the new kernels
def column_reference(proj, h1, gc, gs, Sj):
    """One step of k_gmres_column on float64 inputs, in longdouble, with entry-wise bounds of what float64 arithmetic may leave.
    ``proj``: the ``j + 1`` coefficients, ``h1``: the norm behind them (0 at a breakdown), ``gc`` / ``gs``: the ``j`` stored rotations,
    ``Sj``: ``S[j]``.  Each stored rotation forms ``c n0 + s n1`` and ``-s n0 + c n1``: two products and a sum, ``gamma(2)`` of the sum
    of magnitudes, plus what the carried entry brings in (``e``).  The new rotation is lartg's ``d = sqrt(f^2 + g^2)`` (``gamma(3) d``),
    ``c = |f| / d`` and ``s = g / r`` (``gamma(4)`` each); the error ``e`` of ``f`` moves ``d`` by at most ``e`` and ``c``, ``s`` by at
    most ``e / (d - e)`` (``|dc/df|, |ds/df| <= 1 / d``).  ``S[j] = c S_j`` and ``S[j + 1] = -s S_j`` are one product each.
    Returns ``(col, c, s, S_j', S_j+1')`` and their bounds in the same order."""
    j = len(proj) - 1
    col = np.append(np.asarray(proj, dtype=LD), LD(h1))
    ecol = np.zeros(j + 2)
    g2 = float(gamma(2))
    for k in range(j):
        c, s, n0, n1 = LD(gc[k]), LD(gs[k]), col[k], col[k + 1]
        e0, e1 = ecol[k], ecol[k + 1]
        mag = float(abs(c) * abs(n0) + abs(s) * abs(n1))
        mag2 = float(abs(s) * abs(n0) + abs(c) * abs(n1))
        carried = float(abs(c)) * e0 + float(abs(s)) * e1
        carried2 = float(abs(s)) * e0 + float(abs(c)) * e1
        col[k], col[k + 1] = c * n0 + s * n1, -s * n0 + c * n1
        ecol[k] = g2 * (mag + carried) + carried
        ecol[k + 1] = g2 * (mag2 + carried2) + carried2
    f, e = col[j], ecol[j]
    c, s, r = lartg_any(f, LD(h1), LD)
    d = float(abs(r))
    ec = float(gamma(4)) * float(abs(c)) + (e / (d - e) if d > e else np.inf) * (1 + float(gamma(4)))
    es = float(gamma(4)) * float(abs(s)) + (e / (d - e) if d > e else np.inf) * (1 + float(gamma(4)))
    if h1 == 0:  # lartg's exact branch: c = 1, s = 0, r = f
        ec = es = 0.0
        col[j], ecol[j] = f, e
    else:
        col[j], ecol[j] = r, float(gamma(3)) * d + e * (1 + float(gamma(3)))
    Sj = LD(Sj)
    out = (col[: j + 1], c, s, c * Sj, -s * Sj)
    a = float(abs(Sj))
    bounds = (ecol[: j + 1], ec, es, a * ec + EPS * (float(abs(c)) + ec) * a, a * es + EPS * (float(abs(s)) + es) * a)
    return out, bounds


def solve_reference(R, S, cols, y_dev):
    """The pseudo-solve in longdouble and the bound of a float64 back substitution (Higham, Accuracy and Stability, Theorem 8.5: the
    computed ``y`` solves ``(R + dR) y = S`` with ``|dR| <= gamma(cols) |R|``, so ``|y^ - y| <= gamma(cols) |R^-1| |R| |y^|``).  A zero
    last pivot leaves ``y[cols - 1] = 0`` exactly and the bound is that of the leading triangle."""
    Rl, Sl = np.asarray(R, dtype=LD).copy(), np.asarray(S, dtype=LD).copy()
    y = pseudo_solve(Rl, Sl, cols)
    k = cols - 1 if Rl[cols - 1, cols - 1] == 0 else cols
    T = np.triu(Rl[:k, :k].T)  # T[i, j] = entry (i, j) of the triangle
    bound = np.zeros(cols)
    if k > 0:
        Tinv = np.abs(np.asarray(np.linalg.inv(T.astype(np.float64)), dtype=LD))
        yk = np.abs(np.asarray(y_dev[:k], dtype=LD))
        rhs = np.abs(T) @ yk
        if k < cols:
            pass  # (the zeroed unknown contributes nothing: y[cols - 1] = 0)
        bound[:k] = np.asarray(float(gamma(k)) * (Tinv @ rhs), dtype=np.float64) * (1.0 + 1e-6)  # (the inverse itself is float64-accurate)
    return np.asarray(y, dtype=LD), bound


def update_reference(x, y, V):
    """``x + sum_i y_i V[i]`` in longdouble and its entry-wise bound ``gamma(cols + 1) (|x| + sum |y_i| |V_i|)``"""
    xl, yl, Vl = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD), np.asarray(V, dtype=LD)
    ref = xl + yl @ Vl
    bound = float(gamma(len(y) + 1)) * np.asarray(np.abs(xl) + np.abs(yl) @ np.abs(Vl), dtype=np.float64)
    return ref, bound


def rnorm_reference(w):
    """``|w|`` in longdouble and the bound of a float64 ``sqrt(sum w_i^2)`` in any summation order"""
    wl = np.asarray(w, dtype=LD)
    ref = np.sqrt(np.sum(wl * wl))
    return ref, norm_bound(dot_bound(w, w), ref)


# ---------------------------------------------------------------- the cases of the host and the device tests
def _matrices():
    import bicgstab_reference as br

    return {"convdiff24x20": lambda: br.convdiff(24, 20), "convdiff33x31": lambda: br.convdiff(33, 31), "random401": br.random401,
            "dense130": br.dense130, "skew64": br.skew64}


MATRICES = _matrices()
RTOLS = (1e-6, 1e-10)
RESTARTS = (5, 20, 40)
# Two seeds from 0 .. 11 per (matrix, rtol, restart), in RTOLS x RESTARTS order: the first two that the reference runs alone admit
# (b = default_rng(seed).standard_normal(n)).  No combination had to be dropped.
SEEDS = {
    "convdiff24x20": ((0, 1), (2, 4), (1, 2), (0, 1), (0, 1), (1, 2)),
    "convdiff33x31": ((0, 1), (3, 8), (0, 1), (1, 3), (0, 1), (0, 2)),
    "random401": ((0, 1), (0, 1), (0, 2), (0, 1), (0, 1), (1, 3)),
    "dense130": ((0, 2), (0, 2), (1, 2), (3, 4), (0, 2), (0, 1)),
    "skew64": ((0, 1),) * 6,
}
CASES = [(name, rtol, restart, seed) for name in SEEDS for i, (rtol, restart) in enumerate((t, r) for t in RTOLS for r in RESTARTS)
         for seed in SEEDS[name][i]]
_cache = {}


def matrix(name):
    if ("A", name) not in _cache:
        _cache[("A", name)] = MATRICES[name]()
    return _cache[("A", name)]


def case(name, rtol, restart, seed):
    """``(A, b, admission)`` of a case; computed once and shared, never modified"""
    key = (name, rtol, restart, seed)
    if key not in _cache:
        A = matrix(name)
        b = np.random.default_rng(seed).standard_normal(A.shape[0])
        _cache[key] = (A, b, admission(A, b, rtol, restart))
    return _cache[key]


def breakdown_case():
    """``b`` inside a 3-dimensional invariant subspace of a 100 x 100 matrix: the third step's ``h1`` vanishes"""
    n = 100
    rng = np.random.default_rng(3)
    A = np.diag(np.arange(1.0, n + 1))
    A[:3, :3] = rng.standard_normal((3, 3)) + 3 * np.eye(3)
    b = np.zeros(n)
    b[:3] = [1.0, 2.0, -1.0]
    return np.ascontiguousarray(A), b


def tighten_case():
    """An ill-conditioned normal matrix with six eigenvalue clusters (1 .. 1e-6), ``rtol = 1e-11``, ``restart = 12``, 8 cycles: the
    inner test passes after 7 to 9 steps of cycles 2 to 4 while the true residual stalls near ``eps cond |x|`` above ``atol_eff`` -
    the branch ``ptol_max_factor = max(eps, 0.25 f)``.  (In exact arithmetic the branch cannot be taken - ``presid`` is the true
    residual norm - so the longdouble run is no reference here: the three float64 runs and SciPy's own are.)"""
    n, k = 64, 6
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.repeat(np.logspace(0, -6, k), n // k + 1)[:n]
    A = np.ascontiguousarray(Q @ np.diag(d) @ Q.T)
    return A, rng.standard_normal(n), 1e-11, 12, 8
