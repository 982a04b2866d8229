"""One loop body of the one-sweep loop - the single fused step, a pair, a group of four - in ``np.longdouble`` with first-order error
bounds for a float64 device, and host-made states on which every term of those bodies is large.

The kernels under test (``k_os_pair_*`` / ``k_os_quad_*`` / ``k_os_sweep`` / ``k_os_post`` / ``k_os_sum_predict``, lz_reorth.hip) keep
``G = V V^T``, the applied coefficients ``H`` (``A V_i = sum_l H[l, i] V_l``) and their predictions on the device.  On a Lanczos basis
every off-diagonal of ``G`` and every prediction is O(eps), so a dropped term changes nothing a whole-run test can see.  ``skew_state``
builds a basis by a recurrence whose coefficients are perturbed by ``amp``: ``G`` and ``H`` stay exact descriptions of the rows (to
rounding), and every term is O(amp).  The predictions and the new columns of ``G`` and ``H`` are algebraic identities in ``G``, ``H`` and
the rows, so they hold on such a basis as they do on an orthonormal one.

Values and bounds travel together in ``B`` (value ``v``, absolute bound ``e``, both longdouble).  Every operation adds its own rounding
- ``eps |result|``, for a sum ``eps (|a| + |b|)`` so that another grouping of three terms is covered too, with ``eps`` float64's machine
  epsilon, twice the unit roundoff, so a fused and an unfused evaluation are both covered -
and carries the operands' bounds to first order (sums of magnitudes, never of values):

- a sum or difference: ``e_a + e_b``; a product: ``|a| e_b + |b| e_a``; a quotient: ``(e_a + |q| e_b) / |b|``, two roundings (the device
  may multiply by a reciprocal); a root: ``e_a / (2 root)``;
- a dot product of ``terms`` products, in any order and grouping: ``terms eps sum |a||b|`` plus ``sum (|a| e_b + |b| e_a)``; a dot over
  a basis row counts the padded length, which the device streams too;
- a product row of the matrix: ``nnz_row eps (|A||x|)_row + (|A| e_x)_row`` (``arnoldi_reference``'s).

The bounds run forward from the float64 inputs the device is given (rows, ``y = A V[j-1]`` with the SpMV's own bound, ``G``, ``H``,
``chat``, two scalars) through the whole body, so they grow along the chain of a group; tests/test_one_sweep_step_host.py shows that they
still bind (a dropped term is at least a hundred bounds away) and that they are not too tight (the float64 prototypes lie inside).

``mut`` names one deliberately wrong term (tests/test_one_sweep_step_host.py, "every bound binds"); ``None`` is the reference.

A plain module: no fixtures, nothing collected from it.
"""
import functools

import numpy as np
import scipy.sparse as sp
from arnoldi_reference import EPS, LD, _abs_matvec, matvec, padded, worst  # noqa: F401  (worst: re-exported for the tests)

from lanczos_invariants import perturbed

from lanczos_amd import synthetic

TAU = 1e-14            # kOneSweepTau
FINAL_THREADS = 1024   # kFinalThreads: the one-block kernels' width, which sets the mu chunks of the post kernels


# ---------------------------------------------------------------------------------------------------------------- values with bounds
class B:
    """a longdouble array (or scalar) and an absolute bound on what a float64 device may have in its place"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, dtype=LD), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, B) else B(x)

    def _r(self, v, e):  # one rounding on top of the carried bound
        return B(v, e + EPS * np.abs(v))

    def __add__(self, o):  # (rounded at the operands' magnitudes: the device may add three terms in another grouping)
        o = B.of(o)
        return B(self.v + o.v, self.e + o.e + EPS * (np.abs(self.v) + np.abs(o.v)))

    __radd__ = __add__

    def __sub__(self, o):
        o = B.of(o)
        return B(self.v - o.v, self.e + o.e + EPS * (np.abs(self.v) + np.abs(o.v)))

    def __rsub__(self, o):
        return B.of(o) - self

    def __neg__(self):
        return B(-self.v, self.e)

    def __mul__(self, o):
        o = B.of(o)
        return self._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = B.of(o)
        q = self.v / o.v
        return B(q, (self.e + np.abs(q) * o.e) / np.abs(o.v) + 2 * EPS * np.abs(q))

    def sqrt(self):
        r = np.sqrt(self.v)
        return self._r(r, self.e / (2 * r))

    def __getitem__(self, k):
        return B(np.array(self.v[k]), self.e[k])  # (a copy, never a view: assigning into the parent later must not change it)

    def __setitem__(self, k, o):
        o = B.of(o)
        self.v[k], self.e[k] = o.v, o.e

    def __len__(self):
        return len(self.v)

    @property
    def f(self):
        return self.v.astype(np.float64)

    @property
    def bound(self):
        return self.e.astype(np.float64)


def zeros(*shape):
    return B(np.zeros(shape, dtype=LD))


def dot(a, b, terms=None):
    """``sum a b`` over the last axis of ``a`` (``a``: vector or a matrix of rows, ``b``: vector); ``terms``: the products the device adds"""
    a, b = B.of(a), B.of(b)
    terms = a.v.shape[-1] if terms is None else terms
    mag = np.abs(a.v) @ np.abs(b.v)
    return B(a.v @ b.v, terms * EPS * mag + np.abs(a.v) @ b.e + a.e @ np.abs(b.v))


def comb(c, rows):
    """``sum_i c_i rows_i``: a running sum of ``len(c)`` products per element"""
    c, rows = B.of(c), B.of(rows)
    mag = np.abs(c.v) @ np.abs(rows.v)
    return B(c.v @ rows.v, (len(c) + 1) * EPS * mag + np.abs(c.v) @ rows.e + c.e @ np.abs(rows.v))


def spmv(A, x):
    x = B.of(x)
    ax, terms = _abs_matvec(A, x.f)
    aA = abs(sp.csr_matrix(A)) if sp.issparse(A) else np.abs(A)
    return B(matvec(A, x.v), terms * EPS * ax + matvec(aA, x.e))


def cat(items):
    items = [B.of(x) for x in items]
    return B(np.concatenate([np.atleast_1d(x.v) for x in items]), np.concatenate([np.atleast_1d(x.e) for x in items]))


# ------------------------------------------------------------------------------------------------------------------------- the states
def two_pass_rows(A, j, seed):
    """``j`` rows of a float64 Lanczos run with two Gram-Schmidt passes per step, and the coefficients as ``H``'s columns"""
    A = sp.csr_matrix(A)
    M = A.shape[0]
    V = np.zeros((j, M))
    H = np.zeros((j, j))
    v = np.random.default_rng(seed).standard_normal(M)
    V[0] = v / np.linalg.norm(v)
    for i in range(j - 1):
        w = A @ V[i]
        c = V[: i + 1] @ w
        w = w - c @ V[: i + 1]
        c2 = V[: i + 1] @ w
        w = w - c2 @ V[: i + 1]
        h = np.linalg.norm(w)
        V[i + 1] = w / h
        H[i, i] = (c + c2)[i]  # the three-term part: what the loops record for a step whose walk applied O(eps) coefficients
        if i:
            H[i - 1, i] = H[i, i - 1]
        H[i + 1, i] = h
    return V, H


def skew_rows(A, j, seed, amp):
    """``V_{i+1} = (A V_i - sum_l c_l V_l) / h`` in float64 with ``c`` and ``h`` moved by ``amp``: ``A V_i = sum_l H[l, i] V_l`` to rounding
    whatever the perturbation, ``G``'s off-diagonal entries are O(amp)"""
    A = sp.csr_matrix(A)
    M = A.shape[0]
    rng = np.random.default_rng(seed)
    V = np.zeros((j, M))
    H = np.zeros((j, j))
    v = rng.standard_normal(M)
    V[0] = v / np.linalg.norm(v)
    for i in range(j - 1):
        y = A @ V[i]
        c = V[: i + 1] @ y
        c = c + V[: i + 1] @ (y - c @ V[: i + 1])  # (a second pass: on a skew basis one pass leaves O(amp) of the old rows behind, and the
        c = c + amp * rng.standard_normal(i + 1)   # skewness would grow with j instead of staying O(amp))
        w = y - c @ V[: i + 1]
        h = np.linalg.norm(w) * (1.0 + amp * rng.standard_normal())
        V[i + 1] = w / h
        H[: i + 1, i] = c
        H[i + 1, i] = h
    return V, H, rng


def _gram(V):
    """``V V^T`` in longdouble, by blocks of rows, one triangle (the product of two float64 numbers is exact in longdouble)"""
    Vl = V.astype(LD)
    G = np.zeros((len(V), len(V)), dtype=LD)
    for k in range(0, len(V), 64):
        G[k : k + 64, k:] = Vl[k : k + 64] @ Vl[k:].T
    return np.triu(G) + np.triu(G, 1).T


def basis(A, jmax, kind, seed, amp=1e-3):
    """``jmax`` rows of the ``orth`` or the ``skew`` recurrence with their ``H`` and their Gram matrix (longdouble products of the float64
    rows, rounded once).  A shorter basis of the same seed is a prefix: ``skew_state`` takes its ``j`` rows from any basis that has them."""
    if kind == "orth":
        V, H = two_pass_rows(A, jmax, seed)
    else:
        V, H, _ = skew_rows(A, jmax, seed, amp)
    return V, H, _gram(V).astype(np.float64)


def skew_state(A, j, n, kind, seed, amp=1e-3, rows=None):
    """What the device is handed before step ``j`` of an ``n``-step run.  ``kind``: ``orth`` (a two-pass Lanczos basis: everything O(eps)),
    ``skew`` (the perturbed recurrence), ``miss`` (``skew`` with ``chat`` moved by 1e-6: every leftover far above the gate), ``nan``
    (``orth`` with one NaN in ``chat``).  ``rows``: a ``basis`` of the matching recurrence with at least ``j`` rows (made here if None).
    Returns a dict of float64 arrays: ``V`` (j rows), ``G``, ``H`` (n x n, ``[row, column]``), ``chat`` (j), ``alpha_prev``, ``beta_prev``
    (the two scalars of ``w_j = (A V[j-1] - alpha_prev V[j-1]) - beta_prev V[j-2]``), ``beta_prev2``."""
    assert kind in ("orth", "skew", "miss", "nan") and 2 <= j < n
    plain = kind in ("orth", "nan")
    Vb, Hb, Gb = basis(A, j, "orth" if plain else "skew", seed, amp) if rows is None else rows
    V = np.ascontiguousarray(Vb[:j])
    rng = np.random.default_rng([seed, j])
    amp_ab = 0.0 if plain else amp
    Vl = V.astype(LD)
    y = matvec(A, Vl[j - 1])
    al = float(Vl[j - 1] @ y) + amp_ab * rng.standard_normal()
    be = float(Vl[j - 2] @ y) + amp_ab * rng.standard_normal()
    w = (y - LD(al) * Vl[j - 1]) - LD(be) * Vl[j - 2]
    chat = (Vl @ w).astype(np.float64)
    if kind == "miss":
        chat = chat + 1e-6 * rng.standard_normal(j)
    if kind == "nan":
        chat[j // 2] = np.nan
    G = np.zeros((n, n))
    G[:j, :j] = Gb[:j, :j]
    H = np.zeros((n, n))
    H[:j, : j - 1] = Hb[:j, : j - 1]
    H[j - 1, j - 1] = al  # column j - 1 holds its three-term part only, as the loops leave it
    H[j - 2, j - 1] = be
    return {"V": V, "G": G, "H": H, "chat": chat, "alpha_prev": al, "beta_prev": be, "beta_prev2": float(H[j - 2, j - 3]) if j >= 3 else 0.0,
            "j": j, "n": n, "kind": kind}


# ---- the inputs both test files share, built once per process
@functools.lru_cache(maxsize=None)
def matrix(name):
    """perturbed five-point and seven-point grids (``lanczos_invariants.perturbed``); the name carries the shape"""
    kind, dims = name.split("_")
    dims = tuple(int(d) for d in dims.split("x"))
    L = synthetic.laplacian_2d_5pt(*dims) if kind == "values" else synthetic.laplacian_3d_7pt(*dims)
    return perturbed(L.to_scipy(), "values", 1e-3)


@functools.lru_cache(maxsize=None)
def shared_basis(name, jmax, kind, seed, amp):
    return basis(matrix(name), jmax, kind, seed, amp)


@functools.lru_cache(maxsize=None)
def state(name, j, n, kind, seed=1, amp=1e-3):
    """``skew_state`` on ``matrix(name)``; one basis per input and length class, shared by every case that fits into it"""
    jmax = next(b for b in (16, 72, 520, 1021) if b >= j)
    rows = shared_basis(name, jmax, "orth" if kind in ("orth", "nan") else "skew", seed, amp)
    return skew_state(matrix(name), j, n, kind, seed, amp, rows)


# ------------------------------------------------------------------------------------------------------------------- shared pieces
def _inputs(A, st):
    """the device's inputs as ``B``: exact but for ``y``, which the device's own SpMV formed"""
    V = B(st["V"])
    y = spmv(A, V[st["j"] - 1])
    return V, y, B(st["G"]), B(st["H"]), B(st["chat"])


def _leftover(d, c):
    """``max |d - c|`` as the post kernels form it: a NaN leftover is infinity.  The bound is the largest bound of a difference."""
    e = abs_b(d - c)
    if len(e) == 0:
        return B(0.0)
    if np.isnan(e.v).any():
        return B(np.inf)
    return B(e.v.max(), e.e.max())


def abs_b(x):
    return B(np.abs(x.v), x.e)


def closing(A, G, H, v, J, bJ, n, out, given=None):
    """the plain SpMV on the finished ``V[J]``, ``alpha_J`` and (``J + 1 < n``) the next ``chat`` and column ``J`` of ``H``
    (k_os_sum_predict, fused form: un-normalised predictions)"""
    n_pad = padded(len(v))
    y = spmv(A, v)
    a = dot(v, y, n_pad)
    out["y"], out["alpha_last"] = y, a
    if J + 1 >= n:
        return
    a = _given(given, "alpha_last", a)
    gj, gm = G[:, J], G[:, J - 1]
    chat = zeros(J + 1)
    for i in range(J):
        s = dot(H[: i + 2, i], gj[: i + 2])
        chat[i] = (s - a * gj[i]) - bJ * gm[i]
    chat[J] = (a - a * gj[J]) - bJ * gm[J]
    out["chat_next"] = chat
    H[:, J] = zeros(n)
    H[J, J] = a
    H[J - 1, J] = bJ


# ----------------------------------------------------------------------------------------------------------------- the group of four
def group_chain(A, V, y, al, be, j, m=4):
    n_pad = padded(V.v.shape[1])
    w = (y - al * V[j - 1]) - be * V[j - 2]
    nrm = [dot(w, w, n_pad)]
    b = [nrm[0].sqrt()]
    X = [w / b[0]]
    a = []
    for t in range(m - 1):
        yt = spmv(A, X[t])
        a.append(dot(X[t], yt, n_pad))
        z = (yt - a[t] * X[t]) - b[t] * (X[t - 1] if t else V[j - 1])
        nrm.append(dot(z, z, n_pad))
        b.append(nrm[-1].sqrt())
        X.append(z / b[-1])
    return X, a, b, nrm[-1]


def group_predict(G, H, chat, a, b, j, m=4, mut=None):
    """k_os_quad_predict: ``g[t]`` of length ``j + m`` (zero behind ``j + t``); tools/one_sweep_group_prototype.py's group_predict"""
    g = [zeros(j + m) for _ in range(m)]
    g[0][:j] = chat / b[0]
    for t in range(m - 1):
        gt, new = g[t], g[t + 1]
        prev = g[t - 1] if t else None
        for i in range(j):
            ln = min(i + 2, j)
            if mut == "pred_len_less" and t == 1:
                ln = max(ln - 1, 1)
            s = dot(H[:ln, i], gt[:ln])
            if i == j - 1 and not (mut == "pred_b0" and t == 1) and not (mut == "pred_b0_first" and t == 0):
                s = s + b[0] * (gt[j] if t else 1.0)
            pv = prev[i] if t else G[i, j - 1]
            if mut == "pred_bt_prev" and t == 1:
                pv = B(0.0)
            new[i] = ((s - a[t] * gt[i]) - b[t] * pv) / b[t + 1]
        for s_ in range(t):
            up = B(1.0) if s_ + 1 == t else gt[j + s_ + 1]
            lo = gt[j + s_ - 1] if s_ else gt[j - 1]
            pv = B(1.0) if s_ == t - 1 else prev[j + s_]
            if t == 2 and s_ == 0:  # (the first in-group row with all three neighbours)
                up = B(0.0) if mut == "pred_up" else up
                lo = B(0.0) if mut == "pred_lo" else lo
                pv = B(0.0) if mut == "pred_pv" else pv
            new[j + s_] = ((((b[s_ + 1] * up + a[s_] * gt[j + s_]) + b[s_] * lo) - a[t] * gt[j + s_]) - b[t] * pv) / b[t + 1]
        lo = gt[j + t - 1] if t else gt[j - 1]
        new[j + t] = -(b[t] * lo) / b[t + 1]
    return g


def group_walk(V, X, g, j, m=4, mut=None):
    """k_os_quad_sweep: the measured dots ``D[t]`` (run ``t`` of the walk: ``V_i . x_t``, ``v_{j+s} . x_t``, ``v_{j+t} . v_{j+t}``) and the
    finished rows"""
    n_pad = padded(V.v.shape[1])
    Vo = V[:j]
    D = [zeros(j + m) for _ in range(m)]
    Vn = []
    for t in range(m):
        D[t][:j] = dot(Vo, X[t], n_pad)
        v = X[t] - comb(g[t][:j], Vo)
        for s in range(t):
            gi = g[t][j + s]
            if mut == "walk_gi" and (t, s) == (2, 1):
                gi = B(0.0)
            v = v - gi * Vn[s]
        Vn.append(v)
        for s in range(t):
            D[t][j + s] = dot(Vn[s], X[t], n_pad)
        D[t][j + t] = dot(v, v, n_pad)
    return D, Vn


def mu_chunks(j):
    """the column chunks of the post kernels' sums along the rows of H: ``nchunk`` interleaved chunks of the columns below ``j - 1``"""
    Lp = (j + 63) & ~63
    return max(FINAL_THREADS // Lp, 1)


def group_post(G, H, g, D, a, b, j, n, m=4, mut=None):
    """k_os_quad_post: the leftovers, columns ``j .. j+m-1`` of ``G`` and ``j-1 .. j+m-2`` of ``H`` (in place)"""
    e_old = _leftover(cat([D[t][:j] for t in range(m)]), cat([g[t][:j] for t in range(m)]))
    ins = [(D[t][j + s], g[t][j + s]) for t in range(m) for s in range(t)]
    e_in = _leftover(cat([x for x, _ in ins]), cat([c for _, c in ins]))
    L = j + m + 2
    C = [zeros(L) for _ in range(m)]
    for t in range(m):
        C[t][: j + t] = g[t][: j + t]
        C[t][j + t] = B(1.0)
    col = [zeros(L) for _ in range(m)]
    Gold = G[:j, :j]
    for t in range(m):
        ct = D[t][:j] - dot(Gold, C[t][:j])
        for s in range(t):
            if not (mut == "post_g_ingroup" and (t, s) == (2, 1)):
                ct = ct - col[s][:j] * C[t][j + s]
        col[t][:j] = ct
        for s in range(t):
            v = D[t][j + s] - dot(col[s][:j], C[t][:j])
            for q in range(t):
                hi, lo = (min(s, q), max(s, q)) if mut == "post_g_triangle" else (max(s, q), min(s, q))
                v = v - col[hi][j + lo] * C[t][j + q]
            col[t][j + s] = v
        col[t][j + t] = D[t][j + t]
    # H
    nchunk = mu_chunks(j)
    mu = []
    for t in range(m - 1):
        mt = zeros(L)
        for l in range(j):
            lo = max(l - 1, 0) + (1 if mut == "post_h_start" and t == 1 else 0)
            cols = [i for i in range(lo, j - 1) if not (mut == "post_h_chunk" and t == 1 and i % nchunk == 1)]
            if cols:
                mt[l] = dot(H[l, cols], C[t][cols], len(cols) + nchunk)
        mu.append(mt)
    hn = [zeros(L) for _ in range(m)]
    if mut == "post_h_b0c0":
        hn[0][:j] = H[:j, j - 1]
    else:
        hn[0][:j] = H[:j, j - 1] + b[0] * C[0][:j]
    hn[0][j] = b[0]
    for t in range(m - 1):
        rows = j + t + 2
        sub = mu[t][:rows]
        if not (mut == "post_h_cjm1" and t == 1):
            sub = sub + C[t][j - 1] * hn[0][:rows]
        for s in range(t):
            sub = sub + C[t][j + s] * hn[1 + s][:rows]
        if t:
            last = b[t] * C[t - 1][:rows]
        else:
            last = zeros(rows)
            last[j - 1] = b[0]
        hn[1 + t][:rows] = ((b[t + 1] * C[t + 1][:rows] + a[t] * C[t][:rows]) + last) - sub
    for t in range(m):
        G[: j + t + 1, j + t] = col[t][: j + t + 1]
        G[j + t, : j + t + 1] = col[t][: j + t + 1]
    H[: j + 1, j - 1] = hn[0][: j + 1]
    for t in range(m - 1):
        H[:, j + t] = zeros(n)
        H[: j + t + 2, j + t] = hn[1 + t][: j + t + 2]
    return e_old, e_in


def _given(given, key, default):
    """the device's own value of an intermediate, exact as an input of the next stage, where a test supplies it"""
    if given is None or key not in given:
        return default
    x = given[key]
    return [B(r) for r in x] if isinstance(default, list) else B(x)


def group_step(A, st, mut=None, given=None):
    """One group at step ``j`` on the state ``st``: every quantity the device leaves, as ``B``.  Each stage - chain, predict, walk, post,
    closing - is evaluated on the inputs of that stage: the forward values, or the device's own where ``given`` has them (``a``, ``b``: the
    chain's scalars; ``g``: the predictions; ``D``: the measured sums; ``v_last``: the finished row ``j + 3``; ``alpha_last``), so the
    bounds of one stage do not compound into the next.  The rows ``x_t`` of the chain are overwritten by the walk and cannot be given:
    ``a``, ``b``, ``D`` and the rows carry the chain's bounds."""
    j, n, m = st["j"], st["n"], 4
    V, y, G, H, chat = _inputs(A, st)
    X, a, b, nrm2 = group_chain(A, V, y, B(st["alpha_prev"]), B(st["beta_prev"]), j)
    out = {"a": a, "b": b, "nrm2": nrm2, "y0": y}
    a_in, b_in = _given(given, "a", a), _given(given, "b", b)
    out["g"] = group_predict(G, H, chat, a_in, b_in, j, mut=mut)
    g_in = _given(given, "g", out["g"])
    out["D"], out["rows"] = group_walk(V, X, g_in, j, mut=mut)
    D_in = _given(given, "D", out["D"])
    e_old, e_in = group_post(G, H, g_in, D_in, a_in, b_in, j, n, mut=mut)
    out.update(e_old=e_old, e_in=e_in, G=G, H=H, elog=B(np.maximum(e_old.v, e_in.v), np.maximum(e_old.e, e_in.e)))
    out["flag"] = int(not (e_old.v <= TAU and e_in.v <= TAU))  # (a NaN or infinite leftover trips)
    closing(A, G, H, _given(given, "v_last", out["rows"][m - 1]), j + m - 1, b_in[m - 1], n, out, given)
    return out


# ------------------------------------------------------------------------------------------------------------- the single fused step
def _hess_mu(H, c, rows, ncols, nchunk, mut=None):
    """``mu[l] = sum_{i < ncols} H[l, i] c[i]`` for ``l < rows`` along the rows of the Hessenberg ``H``: the columns from ``l - 1`` on, in
    ``nchunk`` interleaved chunks (k_os_pair_predict's and k_os_quad_post's sums)"""
    mu = zeros(rows)
    for l in range(rows):
        lo = max(l - 1, 0) + (1 if mut == "mu_start" else 0)
        cols = [i for i in range(lo, ncols) if not (mut == "mu_chunk" and i % nchunk == 1)]
        if cols:
            mu[l] = dot(H[l, cols], c[cols], len(cols) + nchunk)
    return mu


def single_step(A, st, mut=None, given=None):
    """The single fused step at ``j >= 2`` (one_sweep_fused_iter): k_os_sweep in the units of ``w``, k_os_post, the gated correcting sweep,
    the scaling SpMV and k_os_sum_predict.  ``given``: ``d`` (the second-stage sums), ``gcorr`` (the correction's coefficients, where the
    gate opened), ``v_last`` (row ``j``), ``alpha_last``."""
    j, n = st["j"], st["n"]
    V, y, G, H, chat = _inputs(A, st)
    n_pad = padded(V.v.shape[1])
    w = (y - V[j - 1] * st["alpha_prev"]) - V[j - 2] * st["beta_prev"]
    t = comb(chat, V) + w
    ut = 2.0 * w - t
    d = cat([dot(V, w, n_pad), dot(ut, ut, n_pad), dot(w, w, n_pad)])
    out = {"y0": y, "d": d}
    d_in = _given(given, "d", d)
    s2 = d_in[j + 1]
    b = s2.sqrt()
    dn, cn = d_in[:j] / b, chat / b
    e = _leftover(dn, cn)
    col = zeros(j + 1)
    col[:j] = dn - dot(G[:j, :j], cn)
    col[j] = d_in[j] / s2
    trip = int(not (e.v <= TAU))
    capp = cn
    if trip:
        g = col[:j]
        out["gcorr"] = g
        g = _given(given, "gcorr", g)
        tg = dot(G[:j, :j], g)
        vv = col[j]
        if mut != "single_vv":
            for i in range(j):  # (the device adds the rows' shares one after the other)
                vv = vv + g[i] * (tg[i] - 2.0 * g[i])
        col[:j] = g - tg
        col[j] = vv
        gb = b * g
        out["gcorr_u"] = gb
        ut = ut - comb(gb, V)
        if mut != "single_capp":
            capp = cn + g
    G[:j, j] = col[:j]
    G[j, : j + 1] = col
    H[:j, j - 1] = H[:j, j - 1] + b * capp
    H[j, j - 1] = b
    v = ut / b
    out.update(u=ut, rows=[v], b=b, nrm2=s2, elog=e, trip=trip, G=G, H=H)
    closing(A, G, H, _given(given, "v_last", v), j, b, n, out, given)
    return out


# -------------------------------------------------------------------------------------------------------------------------- the pair
def pair_predict(G, H, chat, a0, b, j, n, mut=None):
    """k_os_pair_predict: column ``j - 1`` of ``H`` gets the step's applied coefficients (in place), then ``kap`` and ``p`` (``j + 1`` each)"""
    cn = zeros(j + 1)
    cn[:j] = chat / b
    H[:j, j - 1] = H[:j, j - 1] + b * cn[:j]
    H[j, j - 1] = b
    gp = zeros(j + 1)
    gp[:j] = cn[:j] if mut == "pair_gp" else cn[:j] - dot(G[:j, :j], cn[:j])
    gp[j] = B(1.0)
    q = zeros(j)
    for i in range(j):
        ln = min(i + 2, j)
        q[i] = dot(H[:ln, i], cn[:ln])
    if mut != "pair_q_b":
        q[j - 1] = q[j - 1] + b
    Lp = (j + 1 + 63) & ~63
    nchunk = max(FINAL_THREADS // Lp, 1)
    Hm = H
    if mut == "pair_mu_b":  # the row of b_0 that the walk has not yet made
        Hm = B(H.v.copy(), H.e.copy())
        Hm[j, j - 1] = B(0.0)
    mu = _hess_mu(Hm, cn, j + 1, j, nchunk, mut)
    vAv = a0 - 2.0 * dot(cn[:j], q)
    p, kap = zeros(j + 1), zeros(j + 1)
    for i in range(j):
        s = dot(H[: i + 2, i], gp[: i + 2])
        bg = B(0.0) if mut == "pair_p_bg" else b * G[i, j - 1]
        p[i] = (s - a0 * gp[i]) - bg
        kap[i] = (mu[i] - (B(0.0) if mut == "pair_kap_a0" else a0 * cn[i])) + p[i]
    p[j] = (vAv - a0 * gp[j]) - b * gp[j - 1]
    kap[j] = mu[j] + p[j]
    return kap, p


def pair_post(G, H, d1, d2, chat, kap, p, a0, b_w, j, n, mut=None):
    """k_os_pair_post: the leftovers, columns ``j`` and ``j + 1`` of ``G``, column ``j`` of ``H`` (in place); ``d1`` = [V_i . w, u~ . u~],
    ``d2`` = [V_i . z, v_j . z, u~_{j+1} . u~_{j+1}]"""
    uu, vz, uu2 = d1[j], d2[j], d2[j + 1]
    b2 = uu2.sqrt()
    dn, cn = d1[:j] / b_w["b"], chat / b_w["b"]
    e1 = _leftover(dn, cn)
    colj = zeros(j + 1)
    colj[:j] = dn - dot(G[:j, :j], cn)
    colj[j] = uu / b_w["s2"]
    col2 = zeros(j + 1)
    cross = B(0.0) if mut == "pair_post_colj" else colj[:j] * kap[j]
    col2[:j] = (d2[:j] - (dot(G[:j, :j], kap[:j]) + cross)) / b2
    acc = B(0.0) if mut == "pair_post_acc" else dot(colj[:j], kap[:j])
    col2[j] = (vz - (acc + colj[j] * kap[j])) / b2
    e2 = _leftover(col2, zeros(j + 1))
    G[: j + 1, j] = colj
    G[j, : j + 1] = colj
    G[: j + 1, j + 1] = col2
    G[j + 1, : j + 1] = col2
    G[j + 1, j + 1] = B(1.0)
    hc = zeros(n)
    hc[: j + 1] = p
    if mut != "pair_post_hb":
        hc[j - 1] = b_w["b"] + hc[j - 1]
    hc[j] = a0 + hc[j]
    hc[j + 1] = b2
    H[:, j] = hc
    return e1, e2, b2


def pair_step(A, st, mut=None, given=None):
    """One pair at step ``j`` (one_sweep_pair_iter).  ``given``: ``a0`` (alpha_j), ``b`` (the norm of ``w_j``), ``kap``, ``p``, ``d1``, ``d2``
    (the two runs of the second-stage sums), ``u2`` (u~_{j+1}), ``v_last`` (row ``j + 1``), ``alpha_last``.  ``w_j`` and ``y°`` are
    overwritten on the device and carry their forward bounds."""
    j, n = st["j"], st["n"]
    V, y, G, H, chat = _inputs(A, st)
    n_pad = padded(V.v.shape[1])
    w = (y - st["alpha_prev"] * V[j - 1]) - st["beta_prev"] * V[j - 2]
    s2 = dot(w, w, n_pad)
    b = s2.sqrt()
    vo = w / b
    yo = spmv(A, vo)
    a0 = dot(vo, yo, n_pad)
    out = {"y0": y, "a0": a0, "b": b}
    a0_in, b_in = _given(given, "a0", a0), _given(given, "b", b)
    kap, p = pair_predict(G, H, chat, a0_in, b_in, j, n, mut)
    out["kap"], out["p"] = kap, p
    kap_in, p_in = _given(given, "kap", kap), _given(given, "p", p)
    # the walk
    z = (yo - a0_in * (w / b_in)) - b_in * V[j - 1]
    ut = w - comb(chat, V)
    v = ut / b_in
    u2 = (z - comb(kap_in[:j], V)) - kap_in[j] * v
    d1 = cat([dot(V, w, n_pad), dot(ut, ut, n_pad)])
    d2 = cat([dot(V, z, n_pad), dot(v, z, n_pad), dot(u2, u2, n_pad)])
    out.update(d1=d1, d2=d2, u2=u2)
    d1_in, d2_in = _given(given, "d1", d1), _given(given, "d2", d2)
    bw = {"b": b_in, "s2": s2 if given is None or "b" not in given else b_in * b_in}
    e1, e2, b2 = pair_post(G, H, d1_in, d2_in, chat, kap_in, p_in, a0_in, bw, j, n, mut)
    v2 = _given(given, "u2", u2) / b2
    out.update(rows=[v, v2], b2=b2, nrm2=d2_in[j + 1], e1=e1, e2=e2, G=G, H=H, flag=int(not (e1.v <= TAU and e2.v <= TAU)))
    closing(A, G, H, _given(given, "v_last", v2), j + 1, b2, n, out, given)
    return out
