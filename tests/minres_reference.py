"""MINRES in ``np.longdouble`` - one step and the whole loop, the matrix a dense longdouble array (a longdouble sparse product past
2048 rows) - with first-order error bounds for a float64 device, and the matrices of tests/test_minres_host.py and
tests/test_gpu_minres.py.

``step`` is one step of lanczos_amd/minres.py's recurrence from a given state, NOT lagged: it returns ``r``, ``w_k``, ``x_k``, ``v_{k+1}`` and
the scalars.  ``step_bounds`` carries an absolute bound on the error of each through the same operations, for inputs that are float64
numbers.  ``eps`` is float64's machine epsilon, twice the unit roundoff, so that ``m eps sum|terms|`` for an expression of ``m`` rounded
operations has a factor two in hand over ``gamma_m sum|terms|``:

- a product row errs by ``hermitian_reference.product_bound``;
- a dot product of ``n`` terms, summed in ANY order (so also in the order of the partial-sum tree of the device), by
  ``n eps sum|a_i b_i|`` plus what its operands carry;
- ``r_i = (y_i - a v_i) - b m_i`` is four rounded operations, ``w_i = ((v_i - oldeps w2_i) - delta w1_i) / gamma`` five,
  ``x_i + phi w_i`` two, a scalar product or quotient one, ``hypot`` and ``sqrt`` one.

A plain module: no fixtures, nothing collected from it.
"""
import functools

import numpy as np
import scipy.sparse as sp
from arnoldi_reference import EPS, padded, worst  # noqa: F401  (worst, padded: re-exported for the tests)
from arnoldi_reference import matvec as ld_matvec
from hermitian_reference import product_bound

LD = np.longdouble


# ---------------------------------------------------------------- matrices
def lap2d(nx, ny):
    """the Dirichlet 5-point Laplacian on an nx x ny grid (CSR, positive definite)"""
    def t(n):
        return sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])

    A = (sp.kron(sp.eye(ny), t(nx)) + sp.kron(t(ny), sp.eye(nx))).tocsr()
    A.sort_indices()
    return A


def lap1d_periodic(n):
    """the periodic 1-D Laplacian (singular: the constant vector)"""
    A = sp.diags([2.0 * np.ones(n), -np.ones(n - 1), -np.ones(n - 1), [-1.0], [-1.0]], [0, 1, -1, n - 1, -(n - 1)]).tocsr()
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def named(name):
    """``ragged1000`` (empty rows and a row of 300 entries) and ``band70001`` (many partial blocks and a tail): the real parts of
    test_gpu_eigsh_complex.product_matrix's"""
    from test_gpu_eigsh_complex import product_matrix

    A = sp.csr_matrix(product_matrix(name).real)
    A.sort_indices()
    return A


class LdOperator:
    """``A`` for the recurrence below: a dense longdouble array, or - past 2048 rows, where that array would not fit - the sparse matrix
    multiplied in longdouble (arnoldi_reference.matvec)"""

    def __init__(self, A):
        self.shape = A.shape
        self.sparse = A if sp.issparse(A) and A.shape[0] > 2048 else None
        self.dense = None if self.sparse is not None else np.asarray(A.toarray() if sp.issparse(A) else A, dtype=LD)

    def __matmul__(self, x):
        return ld_matvec(self.sparse, x) if self.sparse is not None else self.dense @ np.asarray(x, dtype=LD)


def dense_ld(A):
    return A if isinstance(A, LdOperator) else LdOperator(A)


# ---------------------------------------------------------------- the recurrence
def start(Ad, b, shift=0.0, x0=None):
    """the state step 1 starts from (``Ad``: dense longdouble)"""
    n = Ad.shape[0]
    b = np.asarray(b, dtype=LD)
    x = np.zeros(n, dtype=LD) if x0 is None else np.asarray(x0, dtype=LD)
    r0 = b - (Ad @ x - LD(shift) * x)
    beta1 = np.sqrt(r0 @ r0)
    z = np.zeros(n, dtype=LD)
    return {"k": 1, "x": x, "v": r0 / beta1, "v_prev": z, "w1": z, "w2": z, "beta": beta1, "cs": LD(-1), "sn": LD(0), "dbar": LD(0),
            "epsln": LD(0), "phibar": beta1, "tnorm2": LD(0), "beta1": beta1, "shift": LD(shift)}


def step(Ad, s):
    """one step from state ``s`` -> the next state, with ``r``, ``alpha``, ``phi``, ``gamma``, ``delta``, ``oldeps`` of the step beside it"""
    v, vm, shift = s["v"], s["v_prev"], s["shift"]
    y = Ad @ v
    alpha = v @ y - shift
    r = (y - (alpha + shift) * v) - s["beta"] * vm
    beta = np.sqrt(r @ r)
    tnorm2 = s["tnorm2"] + alpha * alpha + s["beta"] * s["beta"] + beta * beta
    oldeps = s["epsln"]
    delta = s["cs"] * s["dbar"] + s["sn"] * alpha
    gbar = s["sn"] * s["dbar"] - s["cs"] * alpha
    epsln = s["sn"] * beta
    dbar = -s["cs"] * beta
    gamma = max(np.hypot(gbar, beta), LD(EPS))
    cs, sn = gbar / gamma, beta / gamma
    phi = cs * s["phibar"]
    phibar = sn * s["phibar"]
    w = ((v - oldeps * s["w2"]) - delta * s["w1"]) / gamma
    x = s["x"] + phi * w
    with np.errstate(divide="ignore", invalid="ignore"):
        vn = r / beta
    return {"k": s["k"] + 1, "x": x, "v": vn, "v_prev": v, "w1": w, "w2": s["w1"], "beta": beta, "cs": cs, "sn": sn, "dbar": dbar,
            "epsln": epsln, "phibar": phibar, "tnorm2": tnorm2, "beta1": s["beta1"], "shift": shift,
            "r": r, "y": y, "alpha": alpha, "phi": phi, "gamma": gamma, "delta": delta, "gbar": gbar, "oldeps": oldeps}


def loop(A, b, shift, steps, x0=None):
    """``steps`` steps in longdouble -> the final state (``["x"]`` is the iterate)"""
    Ad = dense_ld(A)
    s = start(Ad, b, shift, x0)
    for _ in range(steps):
        s = step(Ad, s)
    return s


SCALARS = ("beta", "cs", "sn", "dbar", "epsln", "phibar", "tnorm2", "beta1", "shift")


def step_bounds(A, s, out):
    """bounds on a float64 device's errors in one step from the float64 state ``s`` to ``out = step(dense_ld(A), s)``: per element for
    ``r``, ``w``, ``x``, ``v`` (the next Lanczos vector), scalars for ``alpha``, ``beta``, ``phi``, ``phibar``"""
    f = lambda a: np.abs(np.asarray(a, dtype=LD))  # noqa: E731
    v, vm = f(s["v"]), f(s["v_prev"])
    n_pad = padded(len(v))
    e_y = np.asarray(product_bound(A, np.asarray(s["v"], dtype=np.float64)), dtype=LD)
    y = f(out["y"])
    e_dot = n_pad * EPS * (v @ y) + v @ e_y
    e_alpha = e_dot + EPS * (abs(out["alpha"]) + abs(s["shift"]))
    a = abs(out["alpha"] + s["shift"])
    e_a = e_alpha + EPS * a
    b = abs(s["beta"])
    e_r = e_y + e_a * v + 4 * EPS * (y + a * v + b * vm)
    r = f(out["r"])
    beta = abs(out["beta"])
    e_nrm2 = 2 * (r @ e_r) + n_pad * EPS * (r @ r)
    e_beta = e_nrm2 / (2 * beta) + EPS * beta
    cs0, sn0, dbar0, phibar0 = abs(s["cs"]), abs(s["sn"]), abs(s["dbar"]), abs(s["phibar"])
    al = abs(out["alpha"])
    e_delta = sn0 * e_alpha + 3 * EPS * (cs0 * dbar0 + sn0 * al)
    e_gbar = cs0 * e_alpha + 3 * EPS * (sn0 * dbar0 + cs0 * al)
    gamma, gbar = abs(out["gamma"]), abs(out["gbar"])
    e_gamma = (gbar * e_gbar + beta * e_beta) / gamma + 2 * EPS * gamma
    cs, sn = abs(out["cs"]), abs(out["sn"])
    e_cs = e_gbar / gamma + cs * e_gamma / gamma + EPS * cs
    e_sn = e_beta / gamma + sn * e_gamma / gamma + EPS * sn
    phi, phibar = abs(out["phi"]), abs(out["phibar"])
    e_phi = e_cs * phibar0 + EPS * phi
    e_phibar = e_sn * phibar0 + EPS * phibar
    w1, w2, w = f(s["w1"]), f(s["w2"]), f(out["w1"])
    e_w = (e_delta * w1 + 5 * EPS * (v + abs(out["oldeps"]) * w2 + abs(out["delta"]) * w1)) / gamma + w * e_gamma / gamma
    e_x = phi * e_w + e_phi * w + 2 * EPS * (f(s["x"]) + phi * w)
    e_v = (e_r + r * (e_beta / beta + EPS)) / beta
    g = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    return {"r": g(e_r), "w": g(e_w), "x": g(e_x), "v": g(e_v), "alpha": float(e_alpha), "beta": float(e_beta), "phi": float(e_phi),
            "phibar": float(e_phibar)}


def random_state(A, k, seed):
    """a float64 state for step ``k``: scalars from a longdouble run of ``k - 1`` steps on ``A``, random unit ``v_k`` orthogonal to a
    random unit ``v_{k-1}``, random ``w`` and ``x``.  Every entry is a float64 number held in longdouble."""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    s = loop(A, rng.standard_normal(n), 0.3, k - 1)
    vm = rng.standard_normal(n)
    vm /= np.linalg.norm(vm)
    v = rng.standard_normal(n)
    v -= (v @ vm) * vm
    v /= np.linalg.norm(v)
    vec = {"x": rng.standard_normal(n), "v": v, "v_prev": vm, "w1": rng.standard_normal(n), "w2": rng.standard_normal(n)}
    st = {key: LD(np.float64(s[key])) for key in SCALARS}
    st.update({key: np.asarray(val, dtype=np.float64).astype(LD) for key, val in vec.items()})
    st["k"] = k
    return st
