"""References for the ``bicgstab`` tests: SciPy's BiCGSTAB loop (lanczos_amd/bicgstab.py's docstring) in ``np.longdouble`` and in float64
with three summation orders, every tested norm recorded; the admission rule that keeps a stopping test off its threshold; and one
iteration in longdouble with the forward-error bounds of its products, inner products and norms.  Nothing here imports the package."""
import math

import numpy as np
import scipy.sparse as sp

EPS = float(np.finfo(np.float64).eps)
TINY = EPS * EPS
LD = np.longdouble


# ---------------------------------------------------------------- matrices
def convdiff(nx, ny, cx=0.6, cy=-0.3, shift=0.5):
    """the periodic 5-point convection-diffusion stencil: diagonal 4 + shift, west -1 - cx, east -1 + cx, south -1 - cy, north -1 + cy"""
    n = nx * ny
    idx = np.arange(n).reshape(nx, ny)
    rows = np.tile(idx.ravel(), 5)
    cols = np.concatenate([idx.ravel(), np.roll(idx, 1, 0).ravel(), np.roll(idx, -1, 0).ravel(), np.roll(idx, 1, 1).ravel(),
                           np.roll(idx, -1, 1).ravel()])
    vals = np.concatenate([np.full(n, 4.0 + shift), np.full(n, -1.0 - cx), np.full(n, -1.0 + cx), np.full(n, -1.0 - cy), np.full(n, -1.0 + cy)])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def random_csr(n, per_row=3, seed=None):
    """``per_row`` normal entries in random columns of every row, plus ``diag(row abs-sum + 1)``: non-symmetric, no empty row"""
    rng = np.random.default_rng(n if seed is None else seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, size=n * per_row)
    S = sp.csr_matrix((rng.standard_normal(n * per_row), (rows, cols)), shape=(n, n))
    A = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr()
    A.sort_indices()
    return A


def random401():
    rng = np.random.default_rng(401)
    S = sp.random(401, 401, 0.02, random_state=rng, data_rvs=rng.standard_normal).tocsr()
    A = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr()
    A.sort_indices()
    return A


def dense130():
    return np.ascontiguousarray(np.random.default_rng(130).standard_normal((130, 130)) + 14.0 * np.eye(130))


def skew64():
    """block diagonal of [[0, 1], [-1, 0]]: ``r . A r`` is exactly 0 for every ``r``, so the first iteration breaks down (-11)"""
    return np.ascontiguousarray(np.kron(np.eye(32), np.array([[0.0, 1.0], [-1.0, 0.0]])))


MATRICES = {"convdiff24x20": lambda: convdiff(24, 20, 0.6, -0.3, 0.5), "convdiff33x31": lambda: convdiff(33, 31, 0.6, -0.3, 0.05),
            "random401": random401, "dense130": dense130}


class Operator:
    """``A x`` and ``|A| |x|`` in longdouble, and the rows' lengths: a dense array or a CSR matrix with no empty row (any size)"""

    def __init__(self, A):
        self.A = A
        self.n = A.shape[0]
        if sp.issparse(A):
            A = A.tocsr()
            self.ptr, self.idx, self.val = A.indptr[:-1].astype(np.int64), A.indices, A.data.astype(LD)
            self.rowlen = np.diff(A.indptr).astype(np.float64)
            assert self.rowlen.min() >= 1
            self.dense = None
        else:
            self.dense = np.asarray(A).astype(LD)
            self.rowlen = np.full(self.n, float(self.n))

    def matvec(self, x):
        x = np.asarray(x, dtype=LD)
        if self.dense is not None:
            return self.dense @ x
        return np.add.reduceat(self.val * x[self.idx], self.ptr)

    def absmatvec(self, x):
        x = np.abs(np.asarray(x, dtype=LD))
        if self.dense is not None:
            return np.abs(self.dense) @ x
        return np.add.reduceat(np.abs(self.val) * x[self.idx], self.ptr)


# ---------------------------------------------------------------- the loop
def _dots(order):
    if order == "dot":
        return lambda a, b: float(np.dot(a, b))
    if order == "reversed":
        return lambda a, b: float(np.dot(a[::-1].copy(), b[::-1].copy()))
    if order == "fsum":
        return lambda a, b: math.fsum((a * b).tolist())
    assert order == "longdouble"
    return lambda a, b: np.dot(a, b)


ORDERS = ("dot", "reversed", "fsum", "longdouble")


def loop(A, b, atol_eff, maxiter, order="longdouble", x0=None, op=None):
    """SciPy's loop; float64 with the inner products summed in ``order``, or everything in longdouble.  Returns ``code`` (SciPy's: a
    run that meets ``|r| < atol_eff`` at the end of the last permitted iteration reports ``maxiter``), ``exit`` (``"half"``, ``"full"``,
    ``"breakdown"``, ``"maxiter"``), ``iterations`` (those that updated ``x``), ``x``, ``r``, ``callbacks`` and ``tests``: every tested
    norm as ``(kind, iteration, norm)`` with kind ``"r"`` (a head test) or ``"s"`` (the half step)."""
    ld = order == "longdouble"
    dt = LD if ld else np.float64
    dot = _dots(order)
    if ld:
        op = op if op is not None else Operator(A)
        mv = op.matvec
    else:
        mv = lambda v: np.asarray(A @ v)  # noqa: E731
    b = np.asarray(b, dtype=dt)
    x = np.zeros(len(b), dtype=dt) if x0 is None else np.array(x0, dtype=dt)
    r = b.copy() if x0 is None or not np.any(x0) else b - mv(x)
    rtilde = r.copy()
    tests = []
    out = {"callbacks": 0}
    rho_prev = omega = alpha = dt(1.0)
    p = v = None
    it = 0

    def end(code, kind):
        out.update({"code": code, "exit": kind, "iterations": it, "x": x, "r": r, "tests": tests})
        return out

    with np.errstate(all="ignore"):
        for k in range(maxiter):
            rnorm = np.sqrt(dot(r, r))
            tests.append(("r", k, float(rnorm)))
            if rnorm < atol_eff:
                return end(0, "full")
            rho = dot(rtilde, r)
            if abs(rho) < TINY:
                return end(-10, "breakdown")
            if k > 0:
                if abs(omega) < TINY:
                    return end(-11, "breakdown")
                beta = (rho / rho_prev) * (alpha / omega)
                p = (p - omega * v) * beta + r
            else:
                p = r.copy()
            v = mv(p)
            rv = dot(rtilde, v)
            if rv == 0:
                return end(-11, "breakdown")
            alpha = rho / rv
            s = r - alpha * v
            snorm = np.sqrt(dot(s, s))
            tests.append(("s", k, float(snorm)))
            if snorm < atol_eff:
                x = x + alpha * p
                r = s
                it = k + 1
                return end(0, "half")
            t = mv(s)
            omega = dot(t, s) / dot(t, t)
            x = (x + alpha * p) + omega * s
            r = s - omega * t
            rho_prev = rho
            it = k + 1
            out["callbacks"] += 1
    return end(maxiter, "maxiter")


# ---------------------------------------------------------------- admission
def admission(A, b, rtol, maxiter=None):
    """The four reference runs of a case and whether it is admitted: they stop at the same test, and at every tested norm
    ``|norm - atol_eff| / atol_eff >= max(0.05, 1000 x the runs' relative spread at that test)``.  ``x_spread``: the largest distance
    (2-norm) between two of the four solutions."""
    n = len(b)
    atol_eff = rtol * float(np.linalg.norm(b))
    maxiter = 10 * n if maxiter is None else maxiter
    op = Operator(A)
    runs = [loop(A, b, atol_eff, maxiter, order, op=op) for order in ORDERS]
    same = all((r["exit"], r["iterations"], len(r["tests"])) == (runs[0]["exit"], runs[0]["iterations"], len(runs[0]["tests"])) for r in runs)
    worst_margin, worst_spread = np.inf, 0.0
    ok = same
    if same:
        for i in range(len(runs[0]["tests"])):
            norms = np.array([r["tests"][i][2] for r in runs])
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
def gamma(L):
    """the standard forward bound's factor ``L eps / (1 - L eps)`` of a sum of ``L`` terms"""
    L = np.asarray(L, dtype=np.float64)
    return L * EPS / (1.0 - L * EPS)


def dot_bound(a, b, da=None, db=None):
    """``(sum a_i b_i in longdouble, bound)`` for a float64 inner product of the float64 vectors ``a`` and ``b``: ``gamma(n) sum |a_i b_i|``;
    where an operand is itself a computed product row off its exact value by at most ``da`` (``db``) entry-wise, the reference is formed
    with the exact operand and the same bound is added for the perturbation the operand carries into the sum"""
    n = len(a)
    al, bl = np.abs(np.asarray(a, dtype=LD)), np.abs(np.asarray(b, dtype=LD))
    g = gamma(n)
    bound = g * float(np.sum(al * bl))
    carried = LD(0.0)
    if da is not None:
        carried = carried + np.sum(np.asarray(da, dtype=LD) * bl)
    if db is not None:
        carried = carried + np.sum(np.asarray(db, dtype=LD) * al)
    if da is not None and db is not None:
        carried = carried + np.sum(np.asarray(da, dtype=LD) * np.asarray(db, dtype=LD))
    return bound + (1.0 + g) * float(carried)


def norm_bound(ss_bound, norm_ref):
    """the bound of ``sqrt(ss)`` from the bound of ``ss``: ``|sqrt a - sqrt b| <= |a - b| / sqrt b``, and the square root's own rounding"""
    return ss_bound / float(norm_ref) + EPS * float(norm_ref)


def product_bound(op, x):
    """entry-wise bound of a float64 product ``A x``: ``gamma(row length) (|A| |x|)_i``"""
    return np.asarray(gamma(op.rowlen) * np.asarray(op.absmatvec(x), dtype=np.float64), dtype=np.float64)


def random_state(n, k, seed):
    """a state that iteration ``k`` starts from: normal vectors and scalars of order one"""
    rng = np.random.default_rng(seed)
    s = {name: rng.standard_normal(n) for name in ("x", "r", "rtilde", "p", "v")}
    s["k"] = k
    s["scalars"] = np.array([1.3, 0.7, -0.45]) if k > 0 else np.array([1.0, 1.0, 1.0])  # rho_prev, alpha, omega
    return s


def worst(err, bound):
    """the largest error / bound over the entries (a zero bound admits a zero error only)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), np.where(err == 0.0, 0.0, np.inf))
    return float(ratio.max()) if ratio.size else 0.0
