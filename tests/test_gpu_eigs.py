"""lanczos_amd.eigs on the device: the Krylov-Schur loop over lz_trl_* under the host tests' bars, lz_trl_residuals_cplx against NumPy in
longdouble, the non-symmetric products, handle reuse between eigsh and eigs, the restart kernel with a non-orthonormal S."""
import numpy as np
import pytest
import scipy.sparse as sp
from test_eigs_host import CASES, EPS, check_result, matrix

import lanczos_amd
from lanczos_amd import _capi
from lanczos_amd.eigs import DeviceCplxBackend, krylov_schur
from lanczos_amd.eigsh import upload_matrix

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _id(c):
    return f"{c[0]}-{c[1]}-k{c[2]}" + (f"-ncv{c[3]}" if c[3] else "")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_eigs_on_the_device(case):
    name, which, k, ncv = case
    A = matrix(name)
    info = {}
    w, X = lanczos_amd.eigs(A, k=k, which=which, ncv=ncv, info=info)
    print(case, "cycles", info["cycles"], "breakdowns", info["breakdowns"])
    check_result(case, A, w, X, info["residuals"])
    assert info["breakdowns"] >= 3 if name == "d" else info["breakdowns"] == 0


@pytest.mark.parametrize("case", [("c", "LM", 4, None), ("c", "LI", 1, None), ("e", "LM", 4, 12), ("e", "LR", 4, 8), ("e", "LI", 3, 12)], ids=_id)
def test_eigs_dense_input(case):
    name, which, k, ncv = case
    A = matrix(name)
    h = _capi.Handle(0)
    info = {}
    w, X = lanczos_amd.eigs(A.toarray(), k=k, which=which, ncv=ncv, handle=h, info=info)
    assert h.spmv_plan() == "dense"
    check_result(case, A, w, X, info["residuals"])
    w2, X2 = lanczos_amd.eigs(A.toarray(), k=k, which=which, ncv=ncv, handle=h)
    assert np.array_equal(w, w2) and np.array_equal(X, X2)  # same call, same bits
    assert np.array_equal(lanczos_amd.eigs(A.toarray(), k=k, which=which, ncv=ncv, return_eigenvectors=False), w)
    h.close()


# ---------------------------------------------------------------- lz_trl_residuals_cplx: the kernel's arithmetic, without the loop
M_TRL = 8
# (k, [positions of the first row of a pair]): a pair in rows 0-1, a pair in the last two of k, k = 1 real, real and pair mixed, k = m
PATTERNS = [(2, [0]), (5, [3]), (1, []), (6, [1, 4]), (M_TRL, [0, 6]), (M_TRL, [])]


def _random_csr(rows, seed):
    """about 6 entries per row at random columns, every seventh row empty, one row with 40 entries"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 12, rows)
    counts[::7] = 0
    counts[rows // 2] = min(40, rows)
    r = np.repeat(np.arange(rows), counts)
    c = np.concatenate([rng.choice(rows, n, replace=False) for n in counts])
    A = sp.csr_matrix((rng.standard_normal(len(r)), (r, c)), shape=(rows, rows))
    A.sort_indices()
    return A


def _load(h, A, kind):
    if kind == "dense":
        h.set_dense(A.toarray())
    else:
        h.set_csr(A.shape[0], 0, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data)


def _spectrum(k, pairs, rng):
    re, im = rng.uniform(-2.0, 2.0, k), np.zeros(k)
    for i in pairs:
        re[i + 1] = re[i]
        im[i] = rng.uniform(0.1, 2.0)
        im[i + 1] = -im[i]
    return re, im


def _reference(A, V, re, im):
    """(residual norms in longdouble, the bound 4 nnz_row eps | |A||x| + |lambda||x| |)"""
    k, rows = len(re), A.shape[0]
    Al = sp.csr_matrix(A)
    # |A| entry by entry as stored (SciPy's abs() first sums a matrix's duplicate entries, in place, in arrays that Al and A share;
    # for a canonical matrix these are the same numbers)
    absA = sp.csr_matrix((np.abs(Al.data), Al.indices, Al.indptr), shape=Al.shape)
    coo = Al.tocoo()

    def mul(x):  # A x in longdouble
        y = np.zeros(rows, dtype=LD)
        np.add.at(y, coo.row, coo.data.astype(LD) * x[coo.col])
        return y

    nnz_row = max(int(np.diff(Al.indptr).max()), 1)
    out, bound = np.zeros(k), np.zeros(k)
    i = 0
    while i < k:
        xr = V[i, :rows].astype(LD)
        if im[i] == 0:
            t = mul(xr) - LD(re[i]) * xr
            out[i] = float(np.sqrt(np.sum(t * t)))
            bound[i] = 4 * nnz_row * EPS * np.linalg.norm(absA @ np.abs(V[i, :rows]) + abs(re[i]) * np.abs(V[i, :rows]))
            i += 1
            continue
        xi = V[i + 1, :rows].astype(LD)
        tr = mul(xr) - LD(re[i]) * xr + LD(im[i]) * xi
        ti = mul(xi) - LD(im[i]) * xr - LD(re[i]) * xi
        out[i] = out[i + 1] = float(np.sqrt(np.sum(tr * tr) + np.sum(ti * ti)))
        ax = np.abs(V[i, :rows]) + np.abs(V[i + 1, :rows])
        bound[i] = bound[i + 1] = 4 * nnz_row * EPS * np.linalg.norm(absA @ ax + abs(complex(re[i], im[i])) * ax)
        i += 2
    return out, bound


def _check_patterns(h, A, rows, seed):
    pad = h.padded_rows(rows)
    rng = np.random.default_rng(seed)
    for k, pairs in PATTERNS:
        V = np.full((M_TRL + 1, pad), np.nan)  # NaN in the padding and in the rows >= k
        V[:k, :rows] = rng.standard_normal((k, rows))
        h.trl_set_rows(0, V)
        re, im = _spectrum(k, pairs, rng)
        got = h.trl_residuals_cplx(k, re, im)
        ref, bound = _reference(A, V, re, im)
        print(rows, k, pairs, "error / bound =", (np.abs(got - ref) / bound).max())
        assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= bound)
        for i in pairs:
            assert got[i] == got[i + 1]
        assert np.array_equal(h.trl_residuals_cplx(k, re, im), got)  # same input, same bits
        if not pairs:  # all im == 0: lz_trl_residuals' bits
            assert np.array_equal(got, h.trl_residuals(k, re))
        else:  # ... and the real rows of a mixed call too
            real = [i for i in range(k) if im[i] == 0]
            plain = h.trl_residuals(k, re)
            assert np.array_equal(got[real], plain[real])


@pytest.mark.parametrize("kind", ["csr", "dense"])
@pytest.mark.parametrize("rows", [12, 255, 256, 257, 300, 1501])
def test_residuals_cplx_against_longdouble(rows, kind):
    A = _random_csr(rows, rows)
    h = _capi.Handle(0)
    _load(h, A, kind)
    assert (h.spmv_plan() == "dense") == (kind == "dense")
    h.trl_begin(M_TRL, np.ones(rows))
    _check_patterns(h, A, rows, rows + 1)
    h.close()


def test_residuals_cplx_on_an_assembled_stencil():
    dims = (4, 4, 4)
    h = _capi.Handle(0)
    h.build_stencil3d_block(dims, 7, 1.0, [-6.0, 1.0, 0.0, 0.0], 0, 64, (), negate_T=True)
    rowptr, colidx, vals = h.get_csr()
    A = sp.csr_matrix((vals, colidx, rowptr), shape=(64, 64))
    h.trl_begin(M_TRL, np.ones(64))
    _check_patterns(h, A, 64, 5)
    h.close()


def test_residuals_cplx_refuses_a_malformed_pair():
    rows = 300
    A = _random_csr(rows, 3)
    h = _capi.Handle(0)
    _load(h, A, "csr")
    h.trl_begin(M_TRL, np.ones(rows))
    rng = np.random.default_rng(4)
    V = np.zeros((M_TRL + 1, h.padded_rows(rows)))
    V[:, :rows] = rng.standard_normal((M_TRL + 1, rows))
    h.trl_set_rows(0, V)
    re, im = _spectrum(4, [1], rng)
    good = h.trl_residuals_cplx(4, re, im)
    bad = [(4, re, np.array([0.0, 0.0, 0.0, 0.7])),                      # a lone positive im at k - 1
           (4, np.array([re[0], re[1], re[1] + 1e-9, re[3]]), im),       # mismatched re
           (4, re, np.array([0.0, im[1], -0.5 * im[1], 0.0])),           # not the conjugate
           (4, re, np.array([-0.3, 0.0, 0.0, 0.0])),                     # a negative im without its partner in front
           (4, re, np.array([0.0, np.nan, 0.0, 0.0])),
           (2, re, im),                                                  # k cuts the pair
           (0, re, im), (M_TRL + 1, np.zeros(M_TRL + 1), np.zeros(M_TRL + 1))]
    for k, r, i in bad:
        with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_ARG"):
            h.trl_residuals_cplx(k, r, i)
    assert np.array_equal(h.trl_residuals_cplx(4, re, im), good)
    h.close()


# ---------------------------------------------------------------- the square product does not lean on symmetry
def _stencil_csr(nx, ny, nz):
    """a constant-coefficient non-symmetric 7-point stencil on a periodic nx x ny x nz grid"""
    def ring(n, lo, hi):
        S = sp.diags([np.full(n - 1, lo), np.full(n - 1, hi)], [-1, 1], format="lil")
        S[0, n - 1] += lo
        S[n - 1, 0] += hi
        return S.tocsr()
    Ix, Iy, Iz = sp.identity(nx), sp.identity(ny), sp.identity(nz)
    A = sp.kron(Iz, sp.kron(Iy, ring(nx, -1.3, -0.7))) + sp.kron(Iz, sp.kron(ring(ny, -1.1, -0.9), Ix)) + sp.kron(ring(nz, -1.2, -0.8), sp.kron(Iy, Ix))
    A = (A + 6.0 * sp.identity(nx * ny * nz)).tocsr()
    A.sort_indices()
    return A


@pytest.mark.parametrize("name", ["a", "c", "stencil", "c-dense"])
def test_products_of_non_symmetric_matrices(name):
    A = _stencil_csr(7, 9, 11) if name == "stencil" else matrix(name[0])
    assert abs(A - A.T).max() > 0.1
    n = A.shape[0]
    h = _capi.Handle(0)
    upload_matrix(h, A.toarray() if name.endswith("dense") else A)
    print(name, "plan", h.spmv_plan(), "coding", h.spmv_coding())
    rng = np.random.default_rng(7)
    absA = abs(A)
    nnz_row = int(np.diff(A.indptr).max())
    for _ in range(3):
        x = rng.standard_normal(n)
        y = h.spmv_host(x)
        bound = (n if name.endswith("dense") else nnz_row) * EPS * (absA @ np.abs(x))
        assert np.all(np.abs(y - A @ x) <= bound)
    h.close()


# ---------------------------------------------------------------- one handle, three solvers' worth of calls
def test_one_handle_serves_eigsh_eigs_eigsh():
    S = matrix("f")
    A = matrix("c")
    fresh = [lanczos_amd.eigsh(S, k=4, which="SA"), lanczos_amd.eigs(A, k=4, which="LM"), lanczos_amd.eigsh(S, k=3, which="LA", ncv=24)]
    h = _capi.Handle(0)
    got = [lanczos_amd.eigsh(S, k=4, which="SA", handle=h), lanczos_amd.eigs(A, k=4, which="LM", handle=h),
           lanczos_amd.eigsh(S, k=3, which="LA", ncv=24, handle=h)]
    h.close()
    for (w0, X0), (w1, X1) in zip(fresh, got):
        assert np.array_equal(w0, w1) and np.array_equal(X0, X1)


# ---------------------------------------------------------------- lz_trl_restart with a non-orthonormal S
class _Recording(DeviceCplxBackend):
    def restart(self, m, kk, S):
        self.before = self.h.trl_get_rows(0, m + 1)
        self.last = (m, kk, np.array(S))
        super().restart(m, kk, S)


def test_final_real_form_rotation_matches_numpy():
    A = matrix("b")
    n = A.shape[0]
    h = _capi.Handle(0)
    upload_matrix(h, A)
    be = _Recording(h, n)
    lam, _ = krylov_schur(be, n, 4, "LR")
    m, kq, S = be.last
    assert kq == len(lam) == 5 and np.abs(S.T @ S - np.eye(kq)).max() > 1e-3  # k splits a pair; S is not orthonormal
    out = h.trl_get_rows(0, kq + 1)
    V = be.before[:, :n]
    ref = S.T @ V[:m]
    scale = (np.abs(S).T @ np.abs(V[:m])).max()
    print("restart error / (m eps scale) =", np.abs(out[:kq, :n] - ref).max() / (m * EPS * scale))
    assert np.abs(out[:kq, :n] - ref).max() <= m * EPS * scale
    assert np.abs(out[:kq, :n] - V[:kq]).max() > 1e-3  # (the rows did change)
    assert np.array_equal(out[kq, :n], V[m])
    h.close()
