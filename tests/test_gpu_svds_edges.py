"""lanczos_amd.svds on the device at the places tests/test_gpu_svds.py leaves alone: the work-item plan of the rectangular product at
its edges, lz_gk_probe and the resumed extension against their NumPy statement, dead (NaN) rows, svds at the size limits and without
convergence, and one handle that serves several problems.  The builders and their properties: tests/test_svds_edges_host.py.

Bars: exact integers and Higham's gamma_n for the product (derived in test_plan_edges_of_the_product); everything else the
project's own (tests/test_gpu_svds.py): step coefficients 1e-12 |A|, basis rows 1e-10, orthogonality 1e-12, restart 1e-13 relative,
values 1e-10 sigma_max, residuals 1e-9 sigma_max (check_triplets)."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg
from scipy.sparse.linalg import ArpackNoConvergence
from test_svds_edges_host import (DEFAULT_CAP, KINDS, NOCONV, NOCONV_TOL, TINY, edge_matrix, shared_handle_calls, step_matrix,
                                  tiny_matrix)
from test_svds_host import check_triplets, host_svds, random_sparse

import lanczos_amd
from lanczos_amd import _capi
from lanczos_amd.svds import NumpyGKBackend

pytestmark = pytest.mark.gpu
U_ROUND = np.finfo(np.float64).eps / 2
P, Q = 4099, 1000  # the shape of the probe, resume and dead-row tests


# ------------------------------------------------------------------ C1: the plan of the product


def long_sums(B, x):
    """per row sum_j B_ij x_j and sum_j |B_ij| |x_j| accumulated in np.longdouble (rows of more than 256 entries only, NaN elsewhere)"""
    ref = np.full(B.shape[0], np.nan, dtype=np.longdouble)
    mag = np.full(B.shape[0], np.nan, dtype=np.longdouble)
    prod = B.data.astype(np.longdouble) * x.astype(np.longdouble)[B.indices]
    for r in np.flatnonzero(np.diff(B.indptr) > 256):
        a, b = B.indptr[r], B.indptr[r + 1]
        ref[r] = prod[a:b].sum()
        mag[r] = np.abs(prod[a:b]).sum()
    return ref, mag


def check_product(h, B, transpose, cap, integer, tag):
    rows, cols = B.shape
    rng = np.random.default_rng(rows + cols)
    x = rng.integers(-4, 5, cols).astype(np.float64) if integer else rng.standard_normal(cols)
    y = h.gk_spmv(x, transpose=transpose)
    n = np.diff(B.indptr)
    split = n > cap
    assert y.shape == (h.padded_rows(rows),)
    assert np.array_equal(y[rows:], np.zeros(len(y) - rows)), tag  # the padding is written (lz_gk_spmv pre-fills y with NaN)
    assert np.isfinite(y).all(), tag                                # ... and so is every row
    if integer:
        exact = scipy.sparse.csr_matrix((B.data.astype(np.int64), B.indices, B.indptr), shape=B.shape) @ x.astype(np.int64)
        assert exact.dtype == np.int64 and np.abs(exact).max() < 2**20
        bad = np.flatnonzero(y[:rows] != exact.astype(np.float64))
        assert len(bad) == 0, f"{tag}: rows {bad[:8]} (lengths {n[bad[:8]]}) got {y[bad[:8]]}, exact {exact[bad[:8]]}"
    else:
        ref = B @ x
        bad = np.flatnonzero((y[:rows] != ref) & ~split)
        assert len(bad) == 0, f"{tag}: unsplit rows {bad[:8]} (lengths {n[bad[:8]]}) differ from csr_matvec by {(y[:rows] - ref)[bad[:8]]}"
        lref, lmag = long_sums(B, x)
        nu = n[split] * U_ROUND
        bound = 1.01 * nu / (1.0 - nu) * lmag[split]
        err = np.abs(y[:rows][split].astype(np.longdouble) - lref[split])
        print(f"\n{tag}: split rows {np.flatnonzero(split)} err / bound {np.asarray(err / bound, dtype=np.float64)}")
        assert np.all(err <= bound), tag
    assert np.array_equal(h.gk_spmv(x, transpose=transpose), y), tag  # same input, same bits
    return int(split.sum())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cap", [256, None, 8190])
def test_plan_edges_of_the_product(cap, kind):
    """Guards lz_gk.hip: rect_plan's `e - r < 512 && rowptr[e + 1] - k0 <= nnz_cap` and its segment loop; k_spmv_rect's
    `kk = k0 & ~1`, `npair = (k1 - kk + 1) >> 1` and the `cap + 2` LDS products, its `blk == 0` padding store and its segment branch;
    k_spmv_rect_fold; launch_spmv_rect's LDS request (65 536 B dynamic + 32 B static at cap 8190); gk_fill_meta's clamp of knob 4
    (lz_gk_api.hip).

    Integer matrix and integer x: |entry| <= 8, |x| <= 4, rows of at most 3 cap + 7 entries - every product and partial sum is an
    integer below 2^20, so any correct summation order gives the exact result bit for bit, split row or not.
    Gaussian: a row inside one tile is added in csr_matvec's order (bit-identical to B @ x); a split row is a sum of n = nnz_row
    products in another order, for which Higham (Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2) gives
    |fl - exact| <= gamma_{n-1} sum |a_i x_i| plus one rounding per product, together <= gamma_n sum |a_i x_i|, gamma_n = n u /
    (1 - n u), u = eps / 2.  The reference and sum |a_i x_i| are np.longdouble sums (relative error about n 2^-64, 2^-11 of
    gamma_n): the factor 1.01."""
    tile = DEFAULT_CAP if cap is None else cap
    nsplit = 0
    for flags in (0, _capi.FLAG_SPMV_STREAM):  # segments, and every long row in one workgroup: the same bounds
        for integer in (True, False):
            E = edge_matrix(tile, kind, integer=integer)
            ET = E.T.tocsr()
            ET.sort_indices()
            tall = E.shape[0] >= E.shape[1]
            h = _capi.Handle(0)
            try:
                if flags:
                    h.set_options(flags)
                if cap is not None:
                    h.set_tuning(_capi.TUNE_STREAM_ENTRIES, cap)
                h.gk_set_csr(*((E, ET) if tall else (ET, E)))
                for B, transpose in ((E, not tall), (ET, tall)):
                    tag = f"cap {cap} {kind} flags {flags} {'integer' if integer else 'gaussian'} {'E^T' if B is ET else 'E'}"
                    nsplit += check_product(h, B, transpose, tile, integer, tag)
            finally:
                h.close()
    assert nsplit == 4 * 4  # E's four long rows each time (no column of E is that long)


# ------------------------------------------------------------------ C2 / C3: probe, resume, dead rows

M17 = 17


class Pair:
    """the device and NumpyGKBackend holding the same P x Q matrix and the same basis rows"""

    def __init__(self, m, flags=0):
        self.A, self.AT = step_matrix(P, Q)
        self.m = m
        self.h = _capi.Handle(0)
        if flags:
            self.h.set_options(flags)
        self.h.gk_set_csr(self.A, self.AT)
        self.be = NumpyGKBackend(self.A)
        self.pp, self.qp = self.h.padded_rows(P), self.h.padded_rows(Q)
        self.v0 = np.random.default_rng(m).uniform(-1.0, 1.0, Q)

    def begin(self):
        """a fresh basis on both (clears the resume state)"""
        self.h.gk_begin(self.m, self.v0)
        self.be.begin(self.m, self.v0)

    def rows(self):
        return self.h.gk_get_rows(0, 0, self.m + 1), self.h.gk_get_rows(1, 0, self.m + 1)

    def set_rows(self, U, V):
        """padded (m + 1)-row images on the device, their finite meaning on the NumPy side"""
        self.h.gk_set_rows(0, 0, U)
        self.h.gk_set_rows(1, 0, V)
        self.be.U[:], self.be.V[:] = U[:, :P], V[:, :Q]

    def close(self):
        self.h.close()


@pytest.fixture(scope="module")
def anorm():
    A, _ = step_matrix(P, Q)
    return scipy.sparse.linalg.svds(A, k=1, return_singular_vectors=False)[0]


@pytest.fixture(scope="module")
def factored():
    """(pair, U, V, colproj, alpha, beta): a partial factorisation extend(0, m) at m = 17 on both backends, the device's rows"""
    pr = Pair(M17)
    pr.begin()
    c, a, b = pr.h.gk_extend(0, M17)
    pr.be.extend(0, M17)
    U, V = pr.rows()
    assert np.linalg.norm(U[:M17, :P] - pr.be.U[:M17], axis=1).max() <= 1e-10
    assert np.linalg.norm(V[:, :Q] - pr.be.V, axis=1).max() <= 1e-10
    yield pr, U, V, c, a, b
    pr.close()


def restore(pr, U, V):
    pr.begin()
    pr.set_rows(U, V)


def check_probe(pr, side, k, x, U, V, tag):
    """one probe on both backends from the state (U, V); NaN rows of that state at or behind k must not matter"""
    pr.h.gk_probe(side, k, x)
    pr.be.probe("uv"[side], k, x)
    Un, Vn = pr.rows()
    new, old, ref, n = ((Un, U, pr.be.U, P), (Vn, V, pr.be.V, Q))[side]
    other_new, other_old = ((Vn, V), (Un, U))[side]
    assert np.isfinite(new[k]).all(), tag
    assert np.linalg.norm(new[k, :n] - ref[k]) <= 1e-10, tag
    assert abs(np.linalg.norm(new[k, :n]) - 1.0) <= 1e-12, tag
    if k:
        assert np.abs(new[:k, :n] @ new[k, :n]).max() <= 1e-12, tag
    assert not new[k, n:].any(), tag  # zero padding
    keep = np.arange(pr.m + 1) != k
    assert np.array_equal(new[keep], old[keep], equal_nan=True), tag  # the other rows: bit-unchanged
    assert np.array_equal(other_new, other_old, equal_nan=True), tag


PROBES = [(1, 0), (1, 5), (1, M17), (0, 0), (0, 5), (0, M17 - 1)]


def test_probe_matches_numpy(factored):
    """Guards lz_gk_api.hip: lz_gk_probe's bound `k > h->gk.m - (side == 0 ? 1 : 0)`; lz_orth.hip: orth_upload_x's memset of the work
    vector's padding, orth_store's two CGS passes over rows [0, k) (orth_dots' `launch_qtw(b.B, b.ld, b.pad, n + 1, n, ...)`: row k is
    the self slot and is not read), its `k == 0` norm-only branch and launch_scale_store's write of row k alone."""
    pr, U, V, *_ = factored
    rng = np.random.default_rng(3)
    for side, k in PROBES:
        restore(pr, U, V)
        check_probe(pr, side, k, rng.standard_normal((P, Q)[side]), U, V, f"side {side} k {k}")
    restore(pr, U, V)
    for side, k in ((0, M17), (1, M17 + 1), (0, -1)):
        with pytest.raises(_capi.LanczosHipError):
            pr.h.gk_probe(side, k, np.ones((P, Q)[side]))
    with pytest.raises(_capi.LanczosHipError):
        pr.h.check(pr.h.lib.lz_gk_probe(pr.h._h, 2, 0, _capi.dptr(np.ones(P))))
    Un, Vn = pr.rows()
    assert np.array_equal(Un, U) and np.array_equal(Vn, V)  # a refused call changes nothing


def compare_extension(pr, dev, ref, j0, anorm, first_half_from):
    """the device's (colproj, alpha, beta) and rows of steps j0 .. m-1 against NumpyGKBackend's (ref, its rows); first_half_from: the
    first step whose first half (alpha, colproj, U row) was computed by this extension"""
    m = pr.m
    c, a, b = dev
    rc, ra, rb = ref
    f = first_half_from
    assert np.isfinite(c[f:]).all() and np.isfinite(a[f:]).all() and np.isfinite(b[j0:]).all()
    assert np.abs(c[f:] - rc[f:]).max() <= 1e-12 * anorm
    assert np.abs(a[f:] - ra[f:]).max() <= 1e-12 * anorm
    assert np.abs(b[j0:] - rb[j0:]).max() <= 1e-12 * anorm
    Un, Vn = pr.rows()
    assert np.isfinite(Un).all() and np.isfinite(Vn).all()
    assert np.linalg.norm(Un[f:m, :P] - pr.be.U[f:m], axis=1).max() <= 1e-10
    assert np.linalg.norm(Vn[j0 + 1:, :Q] - pr.be.V[j0 + 1:], axis=1).max() <= 1e-10
    assert not Un[:, P:].any() and not Vn[:, Q:].any() and not Un[m].any()  # zero padding, zero row U[m]
    return Un, Vn


def test_resume_at_the_second_half_step(factored, anorm):
    """Guards lz_gk_api.hip, lz_gk_extend: `const int u_ready = g.u_ready == k ? k : -1;` and `if (j != u_ready)` - after a probed
    U[5] the extension from 5 starts at A^T U[5] and leaves U[5], alpha[5] and row 5 of the coefficients as they were."""
    pr, U, V, c0, a0, _ = factored
    m = M17
    x = np.random.default_rng(4).standard_normal(P)
    restore(pr, U, V)
    pr.h.gk_extend(0, m)  # (the small arrays of a fresh basis are zero: leave the earlier extension's there)
    restore_rows = pr.rows()
    assert np.array_equal(restore_rows[0], U) and np.array_equal(restore_rows[1], V)  # same input, same bits
    pr.be.U[:], pr.be.V[:] = U[:, :P], V[:, :Q]
    pr.h.gk_probe(0, 5, x)
    pr.be.probe("u", 5, x)
    U5 = pr.h.gk_get_rows(0, 5, 1)[0]
    dev = pr.h.gk_extend(5, m)
    ref = pr.be.extend(5, m)
    Un, Vn = compare_extension(pr, dev, ref, 5, anorm, first_half_from=6)
    assert np.array_equal(Un[5], U5)  # the probed row: bit-unchanged
    assert np.array_equal(Un[:5], U[:5]) and np.array_equal(Vn[:6], V[:6])
    assert dev[1][5] == a0[5] and np.array_equal(dev[0][5], c0[5])  # not rewritten
    assert a0[5] > 0 and np.abs(c0[5, :5]).max() > 0  # (and they were there to be rewritten)


def test_restart_and_extend_clear_the_resume(factored, anorm):
    """Guards lz_gk_api.hip: `g.u_ready = -1;` in lz_gk_restart and at the top of lz_gk_extend.  A probed U[5] followed by a restart
    to kk = 5 (U[5] becomes the zero row U[m]) or by an extension from 6 must not make the next extension from 5 skip A V[5]."""
    pr, U, V, *_ = factored
    m, kk = M17, 5
    rng = np.random.default_rng(5)
    x = rng.standard_normal(P)
    # probe, restart, extend(kk)
    restore(pr, U, V)
    pr.h.gk_probe(0, kk, x)
    pr.be.probe("u", kk, x)
    Pm = np.linalg.qr(rng.standard_normal((m, kk)))[0]
    Qm = np.linalg.qr(rng.standard_normal((m, kk)))[0]
    pr.h.gk_restart(m, kk, Pm, Qm)
    pr.be.restart(m, kk, Pm, Qm)
    assert not pr.h.gk_get_rows(0, kk, 1).any()  # U[kk] = U[m], the zero row: a skipped first half would normalise A^T 0
    dev = pr.h.gk_extend(kk, m)
    ref = pr.be.extend(kk, m)
    compare_extension(pr, dev, ref, kk, anorm, first_half_from=kk)
    # probe, extend(6), extend(5)
    restore(pr, U, V)
    pr.h.gk_probe(0, 5, x)
    pr.be.probe("u", 5, x)
    probed = pr.h.gk_get_rows(0, 5, 1)[0]
    pr.h.gk_extend(6, m)
    pr.be.extend(6, m)
    dev = pr.h.gk_extend(5, m)
    ref = pr.be.extend(5, m)
    Un, _ = compare_extension(pr, dev, ref, 5, anorm, first_half_from=5)
    assert np.linalg.norm(Un[5] - probed) > 0.5  # recomputed from A V[5], not the probed direction


def orthonormal_rows(count, n, rng):
    return np.linalg.qr(rng.standard_normal((n, count)))[0].T.copy()


@pytest.mark.parametrize("k,m", [(0, 17), (5, 17), (0, 23), (5, 23)])
def test_extension_never_reads_dead_rows(k, m, anorm):
    """Guards lz_orth.hip, orth_cgs_step: orth_dots' `launch_qtw(b.B, b.ld, b.pad, n + 1, n, ...)` and `launch_trl_cgs(.., nb, ..)` read rows
    [0, nb) only - lz_reorth.hip's tile_rows clamps the rows of a ragged last tile to `nrows - 1` and steps off row j (`i == jskip`)
    instead of multiplying whatever lies there by zero - and launch_spmv_rect reads x at column indices only, never its padding.
    Rows at and behind the first one an extension writes are NaN, padding included, as a vanished alpha or beta leaves them."""
    pr = Pair(m)
    try:
        pr.begin()
        rng = np.random.default_rng(P + k)
        U = np.zeros((m + 1, pr.pp))
        V = np.zeros((m + 1, pr.qp))
        V[: k + 1, :Q] = orthonormal_rows(k + 1, Q, rng)
        if k:
            U[:k, :P] = orthonormal_rows(k, P, rng)
        pr.set_rows(U, V)
        U[k:m] = np.nan
        V[k + 1:] = np.nan
        pr.h.gk_set_rows(0, 0, U)
        pr.h.gk_set_rows(1, 0, V)
        dev = pr.h.gk_extend(k, m)
        ref = pr.be.extend(k, m)
        Un, Vn = compare_extension(pr, dev, ref, k, anorm, first_half_from=k)
        assert np.array_equal(Un[:k], U[:k]) and np.array_equal(Vn[: k + 1], V[: k + 1])
    finally:
        pr.close()


def test_probe_never_reads_dead_rows(factored):
    """Guards lz_orth.hip, orth_store (see test_probe_matches_numpy): with U[5 ..] or V[6 ..] NaN, padding included, a probe of a
    row in front of them, or of the first dead row itself, still gives NumpyGKBackend's row."""
    pr, U, V, *_ = factored
    Ud, Vd = U.copy(), V.copy()
    Ud[5:M17] = np.nan
    Vd[6:] = np.nan
    rng = np.random.default_rng(6)
    for side, k in ((0, 0), (0, 5), (1, 0), (1, 5), (1, 6)):
        pr.begin()
        pr.set_rows(U, V)  # (the NumPy side keeps the finite rows: it reads none of the dead ones either)
        pr.h.gk_set_rows(0, 0, Ud)
        pr.h.gk_set_rows(1, 0, Vd)
        check_probe(pr, side, k, rng.standard_normal((P, Q)[side]), Ud, Vd, f"side {side} k {k}")


@pytest.mark.parametrize("m,kk", [(23, 21), (20, 10)])
def test_restart_with_a_dead_last_row(m, kk):
    """Guards lz_trl.hip, k_trl_restart: `i = i < m ? i : m - 1;  // rows past m: any valid row, its S entries are 0` (m = 23 is no
    multiple of the 4 rows of a k-step: the clamp must land on row m - 1, never on V[m]) and the `lk == 0` copy V[kk] = V[m].  After
    an exhausted short space V[m] is NaN: rows [0, kk) stay finite and V[kk] receives the NaN row."""
    pr = Pair(m)
    try:
        pr.begin()
        rng = np.random.default_rng(m)
        U = np.zeros((m + 1, pr.pp))
        V = np.zeros((m + 1, pr.qp))
        U[:m, :P] = rng.standard_normal((m, P))
        V[:m, :Q] = rng.standard_normal((m, Q))
        V[m] = np.nan
        pr.h.gk_set_rows(0, 0, U)
        pr.h.gk_set_rows(1, 0, V)
        Pm = np.linalg.qr(rng.standard_normal((m, kk)))[0]
        Qm = np.linalg.qr(rng.standard_normal((m, kk)))[0]
        pr.h.gk_restart(m, kk, Pm, Qm)
        Uo, Vo = pr.rows()
    finally:
        pr.close()
    for out, B, S, n in ((Uo, U, Pm, P), (Vo, V, Qm, Q)):
        ref = S.T @ B[:m, :n]
        assert np.isfinite(out[:kk]).all()
        assert np.abs(out[:kk, :n] - ref).max() <= 1e-13 * np.abs(ref).max()
        assert not out[:kk, n:].any()
        assert np.array_equal(out[kk, :n], B[m, :n], equal_nan=True)  # V: all NaN, U: the zero row
        assert np.array_equal(out[kk, n:], B[kk, n:])                 # (the copy stops at the row length)
        assert np.array_equal(out[kk + 1:], B[kk + 1:], equal_nan=True)
    assert np.isnan(Vo[kk, :Q]).all()


# ------------------------------------------------------------------ C4 - C6: svds


@pytest.mark.parametrize("M,N,k,ncv", TINY)
def test_svds_at_the_size_limits(M, N, k, ncv):
    """Guards lz_gk_api.hip: lz_gk_set_csr's `q < 2 || p < q` and its padded lengths (`round_up(q, kPadDoubles)` with q below one
    padded row), lz_gk_begin's `m > g.V.len`; and, since every case has ncv = min(M, N), the device's exhausted short space: the
    unsynchronised `w / 0` of the last half step (orth_cgs_step's launch_scale_store) leaves V[m] NaN, which lz_gk_restart copies to
    V[k] and lz_gk_residuals / lz_gk_get_vectors (rows [0, k)) never read."""
    A = tiny_matrix(M, N)
    info = {}
    u, s, vh = lanczos_amd.svds(A, k=k, ncv=ncv, info=info)
    check_triplets(A, u, s, vh, "LM", k, info)
    assert info["cycles"] == 1


@pytest.mark.parametrize("shape", sorted(NOCONV))
def test_no_convergence_on_the_device(shape):
    """Guards svds.py, _svds: `err.eigenvectors = backend.get_vectors("u", nconv)` for a wide input, on lz_gk_get_vectors
    (lz_gk_api.hip: `xfer_d2h` of k rows of the long side) after gkl's restart to the nconv converged triplets."""
    A = random_sparse(*shape)
    nconv = NOCONV[shape]
    with pytest.raises(ArpackNoConvergence) as ei:
        lanczos_amd.svds(A, k=6, tol=NOCONV_TOL, maxiter=1)
    err = ei.value
    with pytest.raises(ArpackNoConvergence) as eh:
        host_svds(A, k=6, tol=NOCONV_TOL, maxiter=1)
    smax = np.linalg.svd(A.toarray(), compute_uv=False)[0]
    assert err.nconv == nconv and eh.value.nconv == nconv
    assert err.eigenvalues.shape == (nconv,) and np.all(np.diff(err.eigenvalues) > 0)
    assert np.abs(err.eigenvalues - eh.value.eigenvalues).max() <= 1e-10 * smax
    assert err.eigenvectors.shape == (shape[1], nconv)
    assert np.abs(err.eigenvectors.T @ err.eigenvectors - np.eye(nconv)).max() <= 1e-12
    assert np.abs(np.linalg.norm(A @ err.eigenvectors, axis=0) - err.eigenvalues).max() <= NOCONV_TOL * smax
    assert err.info["cycles"] == 1


def run_calls(calls, handle):
    out = []
    for _, A, kw in calls:
        info = {}
        u, s, vh = lanczos_amd.svds(A, k=6, info=info, handle=handle, **kw)
        out.append((u, s, vh, info["residuals"]))
    return out


@pytest.mark.parametrize("reverse", [False, True])
def test_one_handle_several_problems(reverse):
    """Guards lz_gk_api.hip: lz_gk_set_csr's `gk_free_basis` and re-upload (a second matrix of another shape on the same handle:
    plans, `ldp` / `ldq`, work vectors), lz_gk_begin's `if (!g.d_U || g.m != m)` reallocation with its `gk_small_layout(m)` and
    `if (need > g.part_cap)`: what a call leaves behind must not reach the next one.  Every result is bit-identical to the same call
    on a fresh handle."""
    calls = shared_handle_calls()
    if reverse:
        calls = [calls[1], calls[0]] + calls[2:]
    fresh = []
    for c in calls:
        h = _capi.Handle(0)
        fresh += run_calls([c], h)
        h.close()
    h = _capi.Handle(0)
    shared = run_calls(calls, h)
    h.close()
    for (name, A, _), a, b in zip(calls, shared, fresh):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
    check_triplets(calls[0][1], *shared[0][:3], "LM", 6)
    check_triplets(calls[1][1], *shared[1][:3], "LM", 6)
