"""LSMR in ``np.longdouble`` - one step and the whole loop - with first-order error bounds for a float64 device, and the matrices
of tests/test_lsmr_host.py and tests/test_gpu_lsmr.py.

A state is what the device holds behind ``lz_lsmr_set_state``: unit ``u_k`` and ``v_k``, the scalars of SciPy's loop after step
``k - 1``, and ``x_{k-2}``, ``h_{k-1}``, ``hbar_{k-2}`` with the update of step ``k - 1`` pending (``c1, c2, c3``).  ``step`` applies
that update and then takes one whole step of SciPy's loop, NOT lagged: it returns the next state (lagged again, so that ``loop`` can
chain it) and beside it what a call of ``lz_lsmr_run`` for one step leaves: ``x_out = x_k``, ``h_out = h_{k+1}``, ``hbar_out``.

``step_bounds`` carries an absolute bound on the error of each result through the same operations, for inputs that are float64
numbers.  ``EPS`` is float64's machine epsilon, twice the unit roundoff, so that ``m EPS sum|terms|`` for an expression of ``m``
rounded operations has a factor two in hand over ``gamma_m sum|terms|``:

- a product row errs by ``hermitian_reference.product_bound``, and by ``|A| e`` for an operand that carries the error ``e``;
- a dot product of ``n`` terms, summed in ANY order (so also in the order of the partial-sum tree of the device), by
  ``n EPS sum|a_i b_i|`` plus what its operands carry;
- ``y / nu - alpha (u / nu)`` is four rounded operations, ``a - c b`` and ``a + c b`` two;
- the scalars run through the SAME code as the reference (``scalar_step``) on numbers that carry a bound (``Bnd``): every sum, product,
  quotient and square root adds ``EPS |result|`` to the first-order propagation of its operands' bounds.

A plain module: no fixtures, nothing collected from it.
"""
import numpy as np
import scipy.sparse as sp
from arnoldi_reference import EPS, padded, worst  # noqa: F401  (worst, padded: re-exported for the tests)
from arnoldi_reference import matvec as ld_matvec
from hermitian_reference import product_bound

LD = np.longdouble

SCALARS = ("alpha", "beta", "alphabar", "rho", "rhobar", "cbar", "sbar", "zeta", "zetabar", "betadd", "betad", "rhodold", "tautildeold",
           "thetatilde", "d", "normA2", "maxrbar", "minrbar", "damp", "normb", "c1", "c2", "c3")  # lz_lsmr_set_state's order
CHECKED = ("alpha", "beta", "rho", "rhobar", "zeta", "zetabar", "normr", "normar")


# ---------------------------------------------------------------- matrices
def family(m, n):
    """``F(m, n)``: about six random entries a row plus 4 on the main diagonal, sorted CSR"""
    rng = np.random.default_rng(m + n)
    A = (sp.random(m, n, density=6.0 / n, random_state=rng, data_rvs=rng.standard_normal) + 4.0 * sp.eye(m, n)).tocsr()
    A.sort_indices()
    return A


def rhs(A, consistent, seed=7):
    rng = np.random.default_rng(seed)
    return A @ rng.standard_normal(A.shape[1]) if consistent else rng.standard_normal(A.shape[0])


# ---------------------------------------------------------------- numbers that carry a bound
class Bnd:
    """a longdouble value and an absolute bound on the error of its float64 twin"""

    def __init__(self, val, err=0.0):
        self.val, self.err = LD(val), LD(err)

    @staticmethod
    def of(x):
        return x if isinstance(x, Bnd) else Bnd(x)

    def _new(self, val, err):
        return Bnd(val, err + EPS * abs(val))

    def __add__(self, o):
        o = Bnd.of(o)
        return self._new(self.val + o.val, self.err + o.err)

    __radd__ = __add__

    def __sub__(self, o):
        o = Bnd.of(o)
        return self._new(self.val - o.val, self.err + o.err)

    def __rsub__(self, o):
        return Bnd.of(o) - self

    def __mul__(self, o):
        o = Bnd.of(o)
        return self._new(self.val * o.val, abs(self.val) * o.err + abs(o.val) * self.err)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Bnd.of(o)
        with np.errstate(all="ignore"):
            q = self.val / o.val
            return self._new(q, self.err / abs(o.val) + abs(q) * o.err / abs(o.val))

    def __rtruediv__(self, o):
        return Bnd.of(o) / self

    def __neg__(self):
        return Bnd(-self.val, self.err)

    def __abs__(self):
        return Bnd(abs(self.val), self.err)


def _val(x):
    return x.val if isinstance(x, Bnd) else x


def _sqrt(x):
    if isinstance(x, Bnd):
        r = np.sqrt(x.val)
        return Bnd(r, (x.err / (2 * r) if r > 0 else np.sqrt(x.err)) + EPS * r)
    return np.sqrt(x)


def _pick(a, b, first):
    """``max`` / ``min``: the operand the values choose, with the larger bound of the two"""
    out = a if first else b
    if isinstance(a, Bnd) or isinstance(b, Bnd):
        return Bnd(_val(out), max(Bnd.of(a).err, Bnd.of(b).err))
    return out


def _max(a, b):
    return _pick(a, b, _val(a) >= _val(b))


def _min(a, b):
    return _pick(a, b, _val(a) <= _val(b))


def sym_ortho(a, b):
    """SciPy's ``_sym_ortho`` on longdouble numbers or on ``Bnd``"""
    va, vb = _val(a), _val(b)
    sign = lambda v: LD(np.sign(v))  # noqa: E731
    if vb == 0:
        return sign(va), LD(0), abs(a)
    if va == 0:
        return LD(0), sign(vb), abs(b)
    if abs(vb) > abs(va):
        tau = a / b
        s = sign(vb) / _sqrt(1 + tau * tau)
        return s * tau, s, b / s
    tau = b / a
    c = sign(va) / _sqrt(1 + tau * tau)
    return c, c * tau, a / c


def scalar_step(s, alpha, beta, itn):
    """the body of SciPy's loop behind its two products -> a dict of every scalar it leaves (``c1, c2, c3``: the update it makes
    pending); ``s`` holds the scalars before it, ``alpha`` and ``beta`` are the new ones.  Longdouble numbers or ``Bnd``."""
    chat, shat, alphahat = sym_ortho(s["alphabar"], s["damp"])
    rhoold = s["rho"]
    c, sn, rho = sym_ortho(alphahat, beta)
    thetanew = sn * alpha
    alphabar = c * alpha
    rhobarold, zetaold = s["rhobar"], s["zeta"]
    thetabar = s["sbar"] * rho
    rhotemp = s["cbar"] * rho
    cbar, sbar, rhobar = sym_ortho(s["cbar"] * rho, thetanew)
    zeta = cbar * s["zetabar"]
    zetabar = -sbar * s["zetabar"]
    c1 = thetabar * rho / (rhoold * rhobarold)
    c2 = zeta / (rho * rhobar)
    c3 = thetanew / rho
    betaacute = chat * s["betadd"]
    betacheck = -shat * s["betadd"]
    betahat = c * betaacute
    betadd = -sn * betaacute
    thetatildeold = s["thetatilde"]
    ctildeold, stildeold, rhotildeold = sym_ortho(s["rhodold"], thetabar)
    thetatilde = stildeold * rhobar
    rhodold = ctildeold * rhobar
    betad = -stildeold * s["betad"] + ctildeold * betahat
    tautildeold = (zetaold - thetatildeold * s["tautildeold"]) / rhotildeold
    taud = (zeta - thetatilde * tautildeold) / rhodold
    d = s["d"] + betacheck * betacheck
    normr = _sqrt(d + (betad - taud) * (betad - taud) + betadd * betadd)
    normA2 = s["normA2"] + beta * beta
    normA = _sqrt(normA2)
    normA2 = normA2 + alpha * alpha
    maxrbar = _max(s["maxrbar"], rhobarold)
    minrbar = _min(s["minrbar"], rhobarold) if itn > 1 else s["minrbar"]
    condA = _max(maxrbar, rhotemp) / _min(minrbar, rhotemp)
    return {"alpha": alpha, "beta": beta, "alphabar": alphabar, "rho": rho, "rhobar": rhobar, "cbar": cbar, "sbar": sbar, "zeta": zeta,
            "zetabar": zetabar, "betadd": betadd, "betad": betad, "rhodold": rhodold, "tautildeold": tautildeold, "thetatilde": thetatilde,
            "d": d, "normA2": normA2, "maxrbar": maxrbar, "minrbar": minrbar, "damp": s["damp"], "normb": s["normb"], "c1": c1, "c2": c2,
            "c3": c3, "normr": normr, "normar": abs(zetabar), "normA": normA, "condA": condA}


# ---------------------------------------------------------------- the recurrence
class LdOperator:
    """``A`` and ``A^T`` multiplied in longdouble: dense arrays up to 2048 rows and columns, else the sparse product"""

    def __init__(self, A):
        self.shape = A.shape
        self.A = A
        big = sp.issparse(A) and max(A.shape) > 2048
        self.AT = A.T.tocsr() if sp.issparse(A) else np.ascontiguousarray(np.asarray(A).T)
        self.dense = None if big else np.asarray(A.toarray() if sp.issparse(A) else A, dtype=LD)

    def matvec(self, x):
        return ld_matvec(self.A, x) if self.dense is None else self.dense @ np.asarray(x, dtype=LD)

    def rmatvec(self, x):
        return ld_matvec(self.AT, x) if self.dense is None else self.dense.T @ np.asarray(x, dtype=LD)


def ld_operator(A):
    return A if isinstance(A, LdOperator) else LdOperator(A)


def start(A, b, damp=0.0, x0=None):
    """the state step 1 starts from: the pending update is the empty one on ``h = hbar = 0``, which makes ``h_1 = v_1``"""
    Ad = ld_operator(A)
    n = Ad.shape[1]
    b = np.asarray(b, dtype=LD)
    x = np.zeros(n, dtype=LD) if x0 is None else np.asarray(x0, dtype=LD)
    u = b - Ad.matvec(x) if x0 is not None else b.copy()
    beta = np.sqrt(u @ u)
    u = u / beta
    v = Ad.rmatvec(u)
    alpha = np.sqrt(v @ v)
    v = v / alpha
    z = np.zeros(n, dtype=LD)
    s = dict.fromkeys(SCALARS, LD(0))
    s.update({"alpha": alpha, "beta": beta, "alphabar": alpha, "rho": LD(1), "rhobar": LD(1), "cbar": LD(1), "zetabar": alpha * beta,
              "betadd": beta, "rhodold": LD(1), "normA2": alpha * alpha, "minrbar": LD(1e100), "damp": LD(damp), "normb": np.sqrt(b @ b)})
    s.update({"k": 1, "u": u, "v": v, "x": x, "h": z, "hbar": z.copy()})
    return s


def step(A, s):
    """the pending update, then one step -> the next state with ``x_out``, ``h_out``, ``hbar_out``, ``uh``, ``vh`` (the un-normalised
    ``u`` and ``v``), ``y``, ``z``, ``normx_lagged`` and ``normx`` beside it"""
    Ad = ld_operator(A)
    u, v = s["u"], s["v"]
    hbar1 = s["h"] - s["c1"] * s["hbar"]
    x1 = s["x"] + s["c2"] * hbar1
    h1 = v - s["c3"] * s["h"]
    y = Ad.matvec(v)
    uh = y - s["alpha"] * u
    beta = np.sqrt(uh @ uh)
    un = uh / beta
    z = Ad.rmatvec(uh)
    vh = z / beta - beta * v
    alpha = np.sqrt(vh @ vh)
    vn = vh / alpha
    out = scalar_step(s, alpha, beta, s["k"])
    hbar2 = h1 - out["c1"] * hbar1
    x2 = x1 + out["c2"] * hbar2
    h2 = vn - out["c3"] * h1
    out.update({"k": s["k"] + 1, "u": un, "v": vn, "x": x1, "h": h1, "hbar": hbar1, "uh": uh, "vh": vh, "y": y, "z": z,
                "x_out": x2, "h_out": h2, "hbar_out": hbar2, "normx_lagged": np.sqrt(x1 @ x1), "normx": np.sqrt(x2 @ x2)})
    return out


def loop(A, b, damp, steps, x0=None):
    """``steps`` steps in longdouble -> the final state (``["x_out"]`` is the iterate)"""
    Ad = ld_operator(A)
    s = start(Ad, b, damp, x0)
    s["x_out"] = s["x"]
    for _ in range(steps):
        s = step(Ad, s)
    return s


def step_bounds(A, s, out):
    """bounds on a float64 device's errors in one call of ``lz_lsmr_run`` for one step from the float64 state ``s`` to
    ``out = step(A, s)``: per element for ``uh``, ``vh``, ``u``, ``v``, ``x`` (``x_out``), ``h``, ``hbar``, scalars for ``CHECKED``,
    ``normx_lagged`` and ``normx``"""
    f = lambda a: np.abs(np.asarray(a, dtype=LD))  # noqa: E731
    AT = A.T.tocsr() if sp.issparse(A) else np.ascontiguousarray(np.asarray(A).T)
    absAT = abs(AT) if sp.issparse(AT) else np.abs(AT)
    u, v, x, h, hbar = f(s["u"]), f(s["v"]), f(s["x"]), f(s["h"]), f(s["hbar"])
    c1, c2, c3 = abs(s["c1"]), abs(s["c2"]), abs(s["c3"])
    mp, np_ = padded(len(u)), padded(len(v))
    # the pending update
    hbar1, x1, h1 = f(out["hbar"]), f(out["x"]), f(out["h"])
    e_hb1 = 2 * EPS * (h + c1 * hbar)
    e_x1 = c2 * e_hb1 + 2 * EPS * (x + c2 * hbar1)
    e_h1 = 3 * EPS * (v + c3 * h)

    def norm_bound(vec, e_vec, n_pad):
        n2 = vec @ vec
        nrm = np.sqrt(n2)
        e2 = 2 * (vec @ e_vec) + n_pad * EPS * n2
        return Bnd(n2, e2), (e2 / (2 * nrm) + EPS * nrm if nrm > 0 else np.sqrt(e2))

    _, e_normx_lag = norm_bound(x1, e_x1, np_)
    # u = A v - alpha u
    alpha0 = abs(s["alpha"])
    y = f(out["y"])
    e_y = np.asarray(product_bound(A, np.asarray(s["v"], dtype=np.float64)), dtype=LD)
    uh = f(out["uh"])
    e_uh = e_y + 4 * EPS * (y + alpha0 * u)
    beta = abs(out["beta"])
    _, e_beta = norm_bound(uh, e_uh, mp)
    # v = A^T u / beta - beta v
    z = f(out["z"])
    e_z = np.asarray(absAT @ np.asarray(e_uh, dtype=np.float64), dtype=LD) + np.asarray(
        product_bound(AT, np.asarray(out["uh"], dtype=np.float64)), dtype=LD)
    vh = f(out["vh"])
    e_vh = e_z / beta + z * e_beta / (beta * beta) + e_beta * v + 4 * EPS * (z / beta + beta * v)
    alpha = abs(out["alpha"])
    _, e_alpha = norm_bound(vh, e_vh, np_)
    un, vn = f(out["u"]), f(out["v"])
    e_un = (e_uh + uh * (e_beta / beta + EPS)) / beta
    e_vn = (e_vh + vh * (e_alpha / alpha + EPS)) / alpha
    # the scalars, through the reference's own code
    sb = {key: Bnd(s[key]) for key in SCALARS}
    ob = scalar_step(sb, Bnd(out["alpha"], e_alpha), Bnd(out["beta"], e_beta), s["k"])
    e = {key: ob[key].err for key in ob if isinstance(ob[key], Bnd)}
    n1, n2_, n3 = abs(out["c1"]), abs(out["c2"]), abs(out["c3"])
    # the flush
    hbar2, x2 = f(out["hbar_out"]), f(out["x_out"])
    e_hb2 = e_h1 + e["c1"] * hbar1 + n1 * e_hb1 + 2 * EPS * (h1 + n1 * hbar1)
    e_x2 = e_x1 + e["c2"] * hbar2 + n2_ * e_hb2 + 2 * EPS * (x1 + n2_ * hbar2)
    e_h2 = e_vn + e["c3"] * h1 + n3 * e_h1 + 2 * EPS * (vn + n3 * h1)
    _, e_normx = norm_bound(x2, e_x2, np_)
    g = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    res = {"uh": g(e_uh), "vh": g(e_vh), "u": g(e_un), "v": g(e_vn), "x": g(e_x2), "h": g(e_h2), "hbar": g(e_hb2),
           "normx_lagged": float(e_normx_lag), "normx": float(e_normx)}
    res.update({key: float(e[key]) for key in CHECKED})
    return res


def random_state(A, k, seed, damp=0.3):
    """a float64 state for step ``k`` with a pending update: scalars from a longdouble run of ``k - 1`` steps on ``A``, random unit
    ``u_k`` and ``v_k``, random ``x``, ``h`` and ``hbar``.  Every entry is a float64 number held in longdouble."""
    m, n = A.shape
    rng = np.random.default_rng(seed)
    s = loop(A, rng.standard_normal(m), damp, k - 1)
    u = rng.standard_normal(m)
    u /= np.linalg.norm(u)
    v = rng.standard_normal(n)
    v /= np.linalg.norm(v)
    vec = {"u": u, "v": v, "x": rng.standard_normal(n), "h": rng.standard_normal(n), "hbar": rng.standard_normal(n)}
    st = {key: LD(np.float64(s[key])) for key in SCALARS}
    st.update({key: np.asarray(val, dtype=np.float64).astype(LD) for key, val in vec.items()})
    st["k"] = k
    return st
