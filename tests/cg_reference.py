"""References for the ``cg`` tests: SciPy's conjugate-gradient loop (lanczos_amd/cg.py's docstring) with an optional diagonal
preconditioner, in ``np.longdouble`` and in float64 with three summation orders, every tested norm recorded; the admission rule that
keeps a stopping test off its threshold; and one iteration in longdouble from a random state with the forward-error bounds of
``alpha``, ``beta``, ``|r|``, ``r``, ``p`` and ``x``.  Nothing here imports the package."""
import numpy as np
import scipy.sparse as sp
from bicgstab_reference import EPS, LD, ORDERS, Operator, _dots, dot_bound, gamma, norm_bound, product_bound, worst  # noqa: F401


# ---------------------------------------------------------------- matrices
def lap(nx, ny, diag=4.5):
    """the periodic 5-point Laplacian of the ``nx x ny`` grid: ``diag`` on the diagonal, -1 to the four neighbours"""
    n = nx * ny
    idx = np.arange(n).reshape(nx, ny)
    rows = np.tile(idx.ravel(), 5)
    cols = np.concatenate([idx.ravel(), np.roll(idx, 1, 0).ravel(), np.roll(idx, -1, 0).ravel(), np.roll(idx, 1, 1).ravel(),
                           np.roll(idx, -1, 1).ravel()])
    vals = np.concatenate([np.full(n, float(diag)), np.full(4 * n, -1.0)])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def sym401():
    """``S + S^T + diag(rowabs + 1)``: symmetric, strictly diagonally dominant, rows of 2 to 16 entries"""
    rng = np.random.default_rng(401)
    S = sp.random(401, 401, 0.01, random_state=rng, data_rvs=rng.standard_normal).tocsr()
    T = (S + S.T).tocsr()
    A = (T + sp.diags(np.asarray(abs(T).sum(axis=1)).ravel() + 1.0)).tocsr()
    A.sort_indices()
    return A


def dense130():
    G = np.random.default_rng(130).standard_normal((130, 130))
    return np.ascontiguousarray(G @ G.T / 130.0 + np.eye(130))


def well33x31():
    """``lap33x31`` with diagonal 4.05 plus a log-uniform potential over four decades: the diagonal is the whole difficulty"""
    n = 33 * 31
    A = (lap(33, 31, 4.05) + sp.diags(10.0 ** np.random.default_rng(7).uniform(-1.0, 3.0, n))).tocsr()
    A.sort_indices()
    return A


MATRICES = {"lap24x20": lambda: lap(24, 20), "lap33x31": lambda: lap(33, 31), "sym401": sym401, "dense130": dense130,
            "well33x31": well33x31}


def diagonal_of(A):
    return np.asarray(A.diagonal() if sp.issparse(A) else np.diagonal(A), dtype=np.float64).copy()


# ---------------------------------------------------------------- the loop
def loop(A, b, atol_eff, maxiter, order="longdouble", x0=None, d=None, op=None):
    """SciPy's loop with ``z = d o r`` (``d`` None: ``z = r``); float64 with the inner products summed in ``order``, or everything in
    longdouble.  Returns ``code`` (SciPy's: a run that meets ``|r| < atol_eff`` at the end of the last permitted iteration reports
    ``maxiter``), ``exit`` (``"converged"`` or ``"maxiter"``), ``iterations``, ``x``, ``r``, ``callbacks``, ``indefinite_at`` and
    ``tests``: ``|r|`` at every head test."""
    ld = order == "longdouble"
    dt = LD if ld else np.float64
    dot = _dots(order)
    if ld:
        op = op if op is not None else Operator(A)
        mv = op.matvec
    else:
        mv = lambda v: np.asarray(A @ v)  # noqa: E731
    b = np.asarray(b, dtype=dt)
    dd = None if d is None else np.asarray(d, dtype=dt)
    x = np.zeros(len(b), dtype=dt) if x0 is None else np.array(x0, dtype=dt)
    r = b.copy() if x0 is None or not np.any(x0) else b - mv(x)
    tests = []
    out = {"callbacks": 0, "indefinite_at": None}
    rho_prev = p = None
    it = 0

    def end(code, kind):
        out.update({"code": code, "exit": kind, "iterations": it, "x": x, "r": r, "tests": tests})
        return out

    with np.errstate(all="ignore"):
        for k in range(maxiter):
            rnorm = np.sqrt(dot(r, r))
            tests.append(float(rnorm))
            if rnorm < atol_eff:
                return end(0, "converged")
            z = r if dd is None else dd * r
            rho = dot(r, z)
            p = z.copy() if k == 0 else z + (rho / rho_prev) * p
            q = mv(p)
            pq = dot(p, q)
            if pq <= 0 and out["indefinite_at"] is None:
                out["indefinite_at"] = k
            alpha = rho / pq
            x = x + alpha * p
            r = r - alpha * q
            rho_prev = rho
            it = k + 1
            out["callbacks"] += 1
    return end(maxiter, "maxiter")


# ---------------------------------------------------------------- admission
def admission(A, b, rtol, d=None, maxiter=None):
    """The four reference runs of a case and whether it is admitted: they stop at the same test, and at every tested norm
    ``|norm - atol_eff| / atol_eff >= max(0.05, 1000 x the runs' relative spread at that test)``.  ``x_spread``: the largest distance
    (2-norm) between two of the four solutions."""
    n = len(b)
    atol_eff = rtol * float(np.linalg.norm(b))
    maxiter = 10 * n if maxiter is None else maxiter
    op = Operator(A)
    runs = [loop(A, b, atol_eff, maxiter, order, d=d, op=op) for order in ORDERS]
    same = all((r["exit"], r["iterations"], len(r["tests"])) == (runs[0]["exit"], runs[0]["iterations"], len(runs[0]["tests"])) for r in runs)
    worst_margin, worst_spread = np.inf, 0.0
    ok = same
    if same:
        for i in range(len(runs[0]["tests"])):
            norms = np.array([r["tests"][i] for r in runs])
            spread = float((norms.max() - norms.min()) / np.abs(norms).mean())
            margin = float(np.min(np.abs(norms - atol_eff)) / atol_eff)
            if not margin >= max(0.05, 1000.0 * spread):
                ok = False
            worst_margin, worst_spread = min(worst_margin, margin), max(worst_spread, spread)
    xs = [np.asarray(r["x"], dtype=LD) for r in runs]
    x_spread = max(float(np.linalg.norm(np.asarray(xs[i] - xs[j], dtype=np.float64))) for i in range(4) for j in range(i))
    return {"admitted": ok, "same_stop": same, "margin": worst_margin, "spread": worst_spread, "x_spread": x_spread, "atol_eff": atol_eff,
            "runs": dict(zip(ORDERS, runs))}


# ---------------------------------------------------------------- one iteration and its bounds
def random_state(n, seed, preconditioned):
    """a state that an iteration starts from: normal ``x``, ``r``, ``p``, a ``d`` uniform in (0.5, 2) or None, ``rho = r . (d o r)``"""
    rng = np.random.default_rng(seed)
    s = {name: rng.standard_normal(n) for name in ("x", "r", "p")}
    s["d"] = rng.uniform(0.5, 2.0, n) if preconditioned else None
    s["rho"] = float(np.dot(s["r"], s["r"] if s["d"] is None else s["d"] * s["r"]))
    return s


_F = 1.0 + 16.0 * EPS  # the second-order terms of the bounds below


def _rounded(exact_abs, carried):
    """the bound of a float64 result whose exact value has magnitude ``exact_abs`` and whose operands carry ``carried``: the carried
    error and the rounding of the result itself"""
    return _F * (carried + EPS * (exact_abs + carried))


def one_iteration(A, s, op=None):
    """One iteration of the loop in longdouble from the state ``s`` (``x``, ``r``, ``p`` = the direction this iteration multiplies,
    ``d`` or None, ``rho``) -> ``(ref, bound)``: ``q``, ``pq``, ``alpha``, ``r``, ``rnorm``, ``rho``, ``beta``, ``p``, ``x`` and for each
    the a-priori forward-error bound of the float64 computation ``q = A p; alpha = rho / (p . q); r -= alpha q; rho' = r . (d o r);
    beta = rho' / rho; x += alpha p; p = d o r + beta p`` with every product, sum and inner product rounded in any order."""
    op = op if op is not None else Operator(A)
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    x, r, p = (np.asarray(s[k], dtype=LD) for k in ("x", "r", "p"))
    pa = f(np.abs(p))
    rho = LD(s["rho"])
    ref, bound = {}, {}
    q = op.matvec(s["p"])
    dq = product_bound(op, s["p"])
    qmag = f(np.abs(q)) + dq
    pq = np.dot(p, q)
    dpq = dot_bound(s["p"], qmag, db=dq)
    alpha = rho / pq
    slack = float(abs(pq)) - dpq
    dalpha = _rounded(float(abs(alpha)), float(abs(rho)) * dpq / (float(abs(pq)) * slack)) if slack > 0.0 else np.inf
    ahi = float(abs(alpha)) + dalpha
    r1 = r - alpha * q
    dr = _rounded(f(np.abs(r1)), dalpha * f(np.abs(q)) + ahi * dq + EPS * ahi * qmag)
    rmag = f(np.abs(r1)) + dr
    rr = np.dot(r1, r1)
    drr = dot_bound(rmag, rmag, da=dr, db=dr)
    rnorm = np.sqrt(rr)
    if s["d"] is None:
        z1, dz, rho1, drho = r1, dr, rr, drr
    else:
        dd = np.asarray(s["d"], dtype=LD)
        z1 = dd * r1
        dz = _rounded(f(np.abs(z1)), s["d"] * dr)
        rho1 = np.dot(r1, z1)
        drho = dot_bound(rmag, f(np.abs(z1)) + dz, da=dr, db=dz)
    beta = rho1 / rho
    dbeta = _rounded(float(abs(beta)), drho / float(abs(rho)))
    bhi = float(abs(beta)) + dbeta
    p1 = z1 + beta * p
    dp = _rounded(f(np.abs(p1)), dz + dbeta * pa + EPS * bhi * pa)
    x1 = x + alpha * p
    dx = _rounded(f(np.abs(x1)), dalpha * pa + EPS * ahi * pa)
    ref.update({"q": q, "pq": pq, "alpha": alpha, "r": r1, "rnorm": rnorm, "rho": rho1, "beta": beta, "p": p1, "x": x1})
    bound.update({"q": dq, "pq": dpq, "alpha": dalpha, "r": dr, "rnorm": norm_bound(drr, rnorm), "rho": drho, "beta": dbeta, "p": dp,
                  "x": dx})
    return ref, bound
