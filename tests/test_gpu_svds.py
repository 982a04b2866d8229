"""lanczos_amd.svds on the device: the rectangular product (lz_gk_spmv) against SciPy, extension steps (lz_gk_extend) against their
NumPy statement, the restart of both bases against NumPy, and svds end to end against numpy.linalg.svd.

Bars (tests/test_gpu_trl*.py): values 1e-10 sigma_max, residuals 1e-9 sigma_max, orthonormality 1e-12, step coefficients
1e-12 |A|, basis rows 1e-10 relative."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg
from test_svds_host import bidiagonal, check_triplets, random_sparse, rank5

import lanczos_amd
from lanczos_amd import _capi
from lanczos_amd.svds import NumpyGKBackend, _pack

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def two_per_row(M, N, seed):
    """M x N with exactly two entries in every row (M >> N: the transpose has rows of about 2 M / N entries)"""
    rng = np.random.default_rng(seed)
    c0 = rng.integers(0, N, M)
    c1 = (c0 + 1 + rng.integers(0, N - 1, M)) % N
    rows = np.repeat(np.arange(M), 2)
    return scipy.sparse.csr_matrix((rng.standard_normal(2 * M), (rows, np.stack([c0, c1], axis=1).ravel())), shape=(M, N))


def product_matrix(shape):
    M, N = shape
    if M >= 1_000_000:
        return two_per_row(M, N, 11)
    if M == 40:
        A = random_sparse(M, N, density=0.3, seed=12).tolil()
        A[7, :] = 0.0  # an empty row, and an empty row of the transpose
        A[:, 5] = 0.0
        return A.tocsr()
    return random_sparse(M, N, density=8.0 / min(M, N), seed=13)


_products = {}


def uploaded(shape):
    """(A tall, A^T, handle) per shape, shared by the product tests"""
    if shape not in _products:
        Aop, AopT, _ = _pack(product_matrix(shape))
        h = _capi.Handle(0)
        h.gk_set_csr(Aop, AopT)
        _products[shape] = (Aop, AopT, h)
    return _products[shape]


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("shape", [(40, 33), (1000, 4099), (4099, 1000), (1_000_003, 40)])
def test_rectangular_product(shape, transpose):
    Aop, AopT, h = uploaded(shape)
    B = AopT if transpose else Aop
    rows, cols = B.shape
    if shape == (1_000_003, 40) and transpose:
        assert np.diff(B.indptr).min() > 40000  # the segment path: rows far longer than the LDS tile
    if shape == (40, 33):
        assert np.diff(B.indptr).min() == 0  # an empty row
    x = np.random.default_rng(rows).standard_normal(cols)
    y = h.gk_spmv(x, transpose=transpose)
    assert y.shape == (h.padded_rows(rows),)
    assert np.array_equal(y[rows:], np.zeros(len(y) - rows))  # the padding is written as zeros
    ref = B @ x
    bound = 2.0 * np.diff(B.indptr) * EPS * (abs(B) @ np.abs(x))  # two sums of nnz_row rounded terms, each within nnz_row eps/2 |A||x|
    assert np.all(np.abs(y[:rows] - ref) <= bound)
    assert np.array_equal(h.gk_spmv(x, transpose=transpose), y)  # same input, same bits
    if np.diff(B.indptr).max() <= 4096:
        assert np.array_equal(y[:rows], ref)  # rows inside one tile are summed in csr_matvec's order


def test_long_rows_in_one_workgroup_agree():
    """LZ_FLAG_SPMV_STREAM at lz_gk_set_csr keeps a long row in one workgroup: another summation order, the same bound"""
    Aop, AopT, h = uploaded((1_000_003, 40))
    h2 = _capi.Handle(0)
    h2.set_options(_capi.FLAG_SPMV_STREAM)
    h2.gk_set_csr(Aop, AopT)
    x = np.random.default_rng(5).standard_normal(Aop.shape[0])
    y, y2 = h.gk_spmv(x, transpose=True)[:40], h2.gk_spmv(x, transpose=True)[:40]
    h2.close()
    bound = 2.0 * np.diff(AopT.indptr) * EPS * (abs(AopT) @ np.abs(x))
    assert np.all(np.abs(y - y2) <= bound)


def test_gk_calls_need_their_state():
    h = _capi.Handle(0)
    with pytest.raises(_capi.LanczosHipError):
        h.check(h.lib.lz_gk_begin(h._h, 4, _capi.dptr(np.ones(8))))  # no rectangular matrix
    A = random_sparse(50, 20, density=0.3)
    h.gk_set_csr(*_pack(A)[:2])
    with pytest.raises(_capi.LanczosHipError):
        h.gk_extend(0, 4)  # no basis
    with pytest.raises(_capi.LanczosHipError):
        h.gk_begin(21, np.ones(20))  # m > q
    with pytest.raises(_capi.LanczosHipError):
        h.gk_set_csr(*_pack(A)[:2][::-1])  # p < q
    h.close()


def step_matrix(p, q):
    if p >= 1_000_000:
        return _pack(random_sparse(p, q, density=4.0 / q, seed=21))[:2]
    return _pack(random_sparse(p, q, density=8.0 / q, seed=22))[:2]


def orthonormal_rows(count, n, rng):
    return np.linalg.qr(rng.standard_normal((n, count)))[0].T.copy()


@pytest.mark.parametrize("shape,k,m,force", [((1000, 40), 0, 6, False), ((1000, 40), 0, 6, True), ((4099, 1000), 5, 17, False),
                                             ((4099, 1000), 5, 17, True), ((1_000_003, 257), 30, 33, False),
                                             ((4099, 4099), 120, 128, False)])
def test_extension_steps_match_numpy(shape, k, m, force):
    p, q = shape
    A, AT = step_matrix(p, q)
    nrm = scipy.sparse.linalg.svds(A, k=1, return_singular_vectors=False)[0]
    rng = np.random.default_rng(p + k)
    V0 = orthonormal_rows(k + 1, q, rng)
    U0 = orthonormal_rows(k, p, rng) if k else np.zeros((0, p))
    be = NumpyGKBackend(A, force_second_pass=force)
    be.begin(m, V0[0])
    be.V[: k + 1], be.U[:k] = V0, U0
    h = _capi.Handle(0)
    if force:
        h.set_options(_capi.FLAG_TRL_PASS2_ALWAYS)
    h.gk_set_csr(A, AT)
    h.gk_begin(m, V0[0])
    pp, qp = h.padded_rows(p), h.padded_rows(q)
    Vp = np.zeros((k + 1, qp))
    Vp[:, :q] = V0
    h.gk_set_rows(1, 0, Vp)
    if k:
        Up = np.zeros((k, pp))
        Up[:, :p] = U0
        h.gk_set_rows(0, 0, Up)
    colproj, alpha, beta = h.gk_extend(k, m)
    rc, ra, rb = be.extend(k, m)
    U, V = h.gk_get_rows(0, 0, m + 1), h.gk_get_rows(1, 0, m + 1)
    h.close()
    print(f"\n{shape} k={k} m={m} force={force}: colproj {np.abs(colproj[k:] - rc[k:]).max() / nrm:.2e} alpha "
          f"{np.abs(alpha[k:] - ra[k:]).max() / nrm:.2e} beta {np.abs(beta[k:] - rb[k:]).max() / nrm:.2e} rows "
          f"{np.abs(U[k:m, :p] - be.U[k:m]).max():.2e} {np.abs(V[k + 1:, :q] - be.V[k + 1:]).max():.2e}")
    assert np.abs(colproj[k:] - rc[k:]).max() <= 1e-12 * nrm
    assert np.abs(alpha[k:] - ra[k:]).max() <= 1e-12 * nrm
    assert np.abs(beta[k:] - rb[k:]).max() <= 1e-12 * nrm
    assert np.linalg.norm(U[k:m, :p] - be.U[k:m], axis=1).max() <= 1e-10
    assert np.linalg.norm(V[k + 1:, :q] - be.V[k + 1:], axis=1).max() <= 1e-10
    assert np.array_equal(U[:k, :p], U0) and np.array_equal(V[: k + 1, :q], V0)  # the rows below k: bit-unchanged
    assert not U[:, p:].any() and not V[:, q:].any() and not U[m].any()  # zero padding, zero row U[m]


@pytest.mark.parametrize("m,kk", [(20, 10), (128, 100)])
def test_restart_of_both_bases(m, kk):
    p, q = 4099, 1000
    A, AT = step_matrix(p, q)
    h = _capi.Handle(0)
    h.gk_set_csr(A, AT)
    h.gk_begin(m, np.ones(q))
    rng = np.random.default_rng(m)
    U = np.zeros((m + 1, h.padded_rows(p)))
    V = np.zeros((m + 1, h.padded_rows(q)))
    U[:m, :p] = rng.standard_normal((m, p))
    V[:, :q] = rng.standard_normal((m + 1, q))
    h.gk_set_rows(0, 0, U)
    h.gk_set_rows(1, 0, V)
    P = np.linalg.qr(rng.standard_normal((m, kk)))[0]
    Q = np.linalg.qr(rng.standard_normal((m, kk)))[0]
    h.gk_restart(m, kk, P, Q)
    Uo, Vo = h.gk_get_rows(0, 0, m + 1), h.gk_get_rows(1, 0, m + 1)
    h.close()
    for out, B, S, n in ((Uo, U, P, p), (Vo, V, Q, q)):
        ref = S.T @ B[:m, :n]
        assert np.abs(out[:kk, :n] - ref).max() <= 1e-13 * np.abs(ref).max()
        assert np.array_equal(out[kk], B[m])  # V[kk] == V[m] bit for bit (U: the zero row)
        assert np.array_equal(out[kk + 1:], B[kk + 1:])


@pytest.mark.parametrize("name", ["300x120", "120x300", "400x1000-SM", "rank5"])
def test_svds_on_the_device(name):
    A, k, kw = {"300x120": (random_sparse(300, 120), 6, {}), "120x300": (random_sparse(120, 300), 6, {}),
                "400x1000-SM": (bidiagonal(400, 1000), 4, {"which": "SM", "ncv": 40}), "rank5": (rank5(), 3, {"ncv": 20})}[name]
    info = {}
    u, s, vh = lanczos_amd.svds(A, k=k, info=info, **kw)
    check_triplets(A, u, s, vh, kw.get("which", "LM"), k, info)
    if name == "rank5":
        assert info["breakdowns"] > 0
    u2, s2, vh2 = lanczos_amd.svds(A, k=k, **kw)
    assert np.array_equal(u, u2) and np.array_equal(s, s2) and np.array_equal(vh, vh2)  # same call, same bits


def test_svds_tall_million_rows_and_memory():
    p, q, k, ncv = 1_000_003, 257, 4, 20
    A = random_sparse(p, q, density=4.0 / q, seed=31) @ scipy.sparse.diags(0.9 ** np.arange(q))  # separated leading values
    A = A.tocsr()
    h = _capi.Handle(0)
    h.gk_set_csr(*_pack(random_sparse(40, 33, density=0.3))[:2])  # (the runtime's first allocations are not the solver's)
    free0 = h.device_memory()[0]
    info = {}
    u, s, vh = lanczos_amd.svds(A, k=k, ncv=ncv, handle=h, info=info)
    free1 = h.device_memory()[0]
    pad = h.padded_rows(p)
    h.close()
    assert np.all(np.diff(s) > 0)
    r1 = np.linalg.norm(A @ vh.T - u * s, axis=0)
    r2 = np.linalg.norm(A.T @ u - vh.T * s, axis=0)
    print(f"\nsvds {p} x {q}: s {s}, residuals {r1.max():.2e} {r2.max():.2e}, {info['cycles']} cycles, {(free0 - free1) / 2**20:.0f} MiB")
    assert max(r1.max(), r2.max()) <= 1e-9 * s[-1]
    assert np.abs(info["residuals"] - np.stack([r1, r2])).max() <= 1e-12 * s[-1]
    assert np.abs(u.T @ u - np.eye(k)).max() <= 1e-12 and np.abs(vh @ vh.T - np.eye(k)).max() <= 1e-12
    top = np.sqrt(np.linalg.eigvalsh((A.T @ A).toarray())[-k:])
    assert np.abs(s - top).max() <= 1e-10 * top[-1]
    matrix = 2 * (12 * A.nnz + 4 * (p + q))  # A and its transpose
    assert free0 - free1 <= (2 * ncv + 2) * pad * 8 + (64 << 20) + matrix


def test_svds_leaves_the_square_problem_of_its_handle_alone():
    S = random_sparse(500, 500, density=0.02, seed=41)
    S = (S + S.T).tocsr()
    h = _capi.Handle(0)
    theta, Y = lanczos_amd.eigsh(S, k=4, which="LA", handle=h)
    res = h.trl_residuals(4, theta)
    lanczos_amd.svds(random_sparse(300, 120), k=6, handle=h)
    assert np.array_equal(h.trl_get_vectors(4), Y) and np.array_equal(h.trl_residuals(4, theta), res)  # matrix and basis untouched
    theta2, Y2 = lanczos_amd.eigsh(S, k=4, which="LA", handle=h)
    h.close()
    assert np.array_equal(theta, theta2) and np.array_equal(Y, Y2)
