"""The thick-restart Golub-Kahan-Lanczos outer loop of lanczos_amd.svds, driven by its NumPy backend (no GPU), against numpy.linalg.svd.

Bars (tests/test_gpu_trl*.py): values 1e-10 sigma_max, residuals 1e-9 sigma_max, orthonormality 1e-12."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg
from scipy.sparse.linalg import ArpackNoConvergence

from lanczos_amd.eigsh import _SEED as EIGSH_SEED
from lanczos_amd.svds import _SEED, NumpyGKBackend, _svds, check_args, gkl


def host_svds(A, k=6, ncv=None, tol=0, which="LM", v0=None, maxiter=None, return_singular_vectors=True, solver="arpack", rng=None,
              random_state=None, options=None, info=None, backends=None):
    """lanczos_amd.svds with the NumPy backend in the device backend's place"""

    def make(Aop, AopT):
        be = NumpyGKBackend(Aop)
        if backends is not None:
            backends.append(be)
        return be

    return _svds(make, A, k, ncv, tol, which, v0, maxiter, return_singular_vectors, solver, rng, random_state, options, info)


def random_sparse(M, N, density=0.05, seed=1):
    rng = np.random.default_rng(seed)
    return scipy.sparse.random(M, N, density=density, random_state=rng, data_rvs=rng.standard_normal, format="csr")


def bidiagonal(M, N):
    n = min(M, N)
    d = 1.0 + 9.0 * np.arange(n) / n
    i = np.arange(n)
    sup = i[i + 1 < N]  # the superdiagonal as far as the shape has it
    return scipy.sparse.csr_matrix((np.concatenate([d, np.full(len(sup), 0.3)]), (np.concatenate([i, sup]), np.concatenate([i, sup + 1]))),
                                   shape=(M, N))


def rank5(seed=3):
    rng = np.random.default_rng(seed)
    X = np.linalg.qr(rng.standard_normal((200, 5)))[0]
    Y = np.linalg.qr(rng.standard_normal((90, 5)))[0].T
    return X @ np.diag([5.0, 4.0, 3.0, 2.0, 1.0]) @ Y


def dense_of(A):
    return A.toarray() if scipy.sparse.issparse(A) else np.asarray(A)


def check_triplets(A, u, s, vh, which, k, info=None):
    D = dense_of(A)
    ref = np.linalg.svd(D, compute_uv=False)
    smax = ref[0]
    want = np.sort(ref[:k]) if which == "LM" else np.sort(ref[-k:])
    assert s.shape == (k,) and u.shape == (D.shape[0], k) and vh.shape == (k, D.shape[1])
    assert np.all(np.diff(s) >= 0)
    assert np.abs(s - want).max() <= 1e-10 * smax
    r1 = np.linalg.norm(D @ vh.T - u * s, axis=0)
    r2 = np.linalg.norm(D.T @ u - vh.T * s, axis=0)
    assert max(r1.max(), r2.max()) <= 1e-9 * smax
    assert np.abs(u.T @ u - np.eye(k)).max() <= 1e-12
    assert np.abs(vh @ vh.T - np.eye(k)).max() <= 1e-12
    if info is not None:
        assert info["residuals"].shape == (2, k)
        assert np.abs(info["residuals"] - np.stack([r1, r2])).max() <= 1e-12 * smax


@pytest.mark.parametrize("shape", [(300, 120), (120, 300)])
def test_random_sparse_lm(shape):
    A = random_sparse(*shape)
    info = {}
    u, s, vh = host_svds(A, k=6, info=info)
    check_triplets(A, u, s, vh, "LM", 6, info)
    assert info["cycles"] >= 1 and info["matvecs"] > 0 and info["breakdowns"] == 0
    assert abs(info["anorm"] - s[-1]) <= 1e-10 * s[-1]


def test_square_nonsymmetric():
    A = random_sparse(257, 257, seed=5)
    u, s, vh = host_svds(A, k=3)
    check_triplets(A, u, s, vh, "LM", 3)


@pytest.mark.parametrize("shape,k", [((1000, 400), 5), ((400, 1000), 4)])
def test_bidiagonal_sm(shape, k):
    A = bidiagonal(*shape)
    u, s, vh = host_svds(A, k=k, which="SM", ncv=40)
    check_triplets(A, u, s, vh, "SM", k)


@pytest.mark.parametrize("k", [3, 4])
def test_rank5_breaks_down_and_recovers(k):
    A = rank5()
    info = {}
    u, s, vh = host_svds(A, k=k, ncv=20, info=info)
    assert info["breakdowns"] > 0
    assert np.abs(s - np.array([5.0, 4.0, 3.0, 2.0, 1.0])[:k][::-1]).max() <= 1e-10 * 5.0
    check_triplets(A, u, s, vh, "LM", k, info)


def test_exhausted_space():
    A = random_sparse(60, 25, density=0.3, seed=7)
    info = {}
    u, s, vh = host_svds(A, k=4, ncv=25, info=info)
    check_triplets(A, u, s, vh, "LM", 4, info)
    assert info["cycles"] == 1


def test_k_equal_one():
    A = random_sparse(300, 120)
    u, s, vh = host_svds(A, k=1)
    check_triplets(A, u, s, vh, "LM", 1)


def test_dense_and_float32_input(capsys):
    A = random_sparse(80, 50, density=0.2, seed=9).toarray()
    u, s, vh = host_svds(A, k=3)
    check_triplets(A, u, s, vh, "LM", 3)
    u, s32, vh = host_svds(A.astype(np.float32), k=3)
    assert "float32" in capsys.readouterr().out
    assert np.abs(s32 - s).max() <= 1e-6 * s[-1]


def test_argument_errors():
    A = random_sparse(60, 25, density=0.3)
    for k in (0, 25, 30, -1):
        with pytest.raises(ValueError):
            host_svds(A, k=k)
    for ncv in (4, 26, 200):  # k + 2 = 5 <= ncv <= min(25, 128)
        with pytest.raises(ValueError, match=r"k\+2<=ncv<=min"):
            host_svds(A, k=3, ncv=ncv)
    B = random_sparse(400, 300, density=0.01)
    with pytest.raises(ValueError, match=r"k\+2<=ncv<=min"):
        host_svds(B, k=3, ncv=129)
    assert check_args((60, 25), 3, "LM", None) == 20
    assert check_args((400, 300), 20, "LM", None) == 41
    assert check_args((60, 25), 3, "LM", 5) == 5
    with pytest.raises(ValueError):
        host_svds(A, k=3, which="LA")
    with pytest.raises(NotImplementedError):
        host_svds(A, k=3, solver="lobpcg")
    with pytest.raises(NotImplementedError):
        host_svds(A, k=3, options={})
    with pytest.raises(NotImplementedError):
        host_svds(A.astype(np.complex128), k=3)
    with pytest.raises(ValueError):
        host_svds(A, k=3, v0=np.ones(60))  # v0 has length min(M, N)
    with pytest.raises(ValueError):
        host_svds(A, k=3, v0=np.zeros(25))
    with pytest.raises(ValueError):
        host_svds(A, k=3, return_singular_vectors="v")
    with pytest.raises(ValueError):
        host_svds(np.ones((1, 5)), k=1)


def test_return_singular_vectors_forms():
    A = random_sparse(120, 300)
    u, s, vh = host_svds(A, k=4)
    s_only = host_svds(A, k=4, return_singular_vectors=False)
    assert isinstance(s_only, np.ndarray) and np.array_equal(s_only, s)
    u2, s2, none = host_svds(A, k=4, return_singular_vectors="u")
    assert none is None and np.array_equal(u2, u) and np.array_equal(s2, s)
    none, s3, vh3 = host_svds(A, k=4, return_singular_vectors="vh")
    assert none is None and np.array_equal(vh3, vh) and np.array_equal(s3, s)


@pytest.mark.parametrize("shape", [(300, 120), (120, 300)])
def test_no_convergence_carries_consistent_shapes(shape):
    A = random_sparse(*shape)
    with pytest.raises(ArpackNoConvergence) as ei:
        host_svds(A, k=6, maxiter=1)
    err = ei.value
    nconv = len(err.eigenvalues)
    assert nconv < 6
    assert err.eigenvectors.shape == (shape[1], nconv)
    assert np.all(np.diff(err.eigenvalues) >= 0)
    assert err.info["cycles"] == 1
    if nconv:
        D = A.toarray()
        assert np.abs(np.linalg.norm(D @ err.eigenvectors, axis=0) - err.eigenvalues).max() <= 1e-9 * err.eigenvalues.max()


def test_same_seed_same_bits_and_global_rng_untouched():
    A = random_sparse(300, 120)
    np.random.seed(123)
    state = np.random.get_state()[1].copy()
    a = host_svds(A, k=6)
    b = host_svds(A, k=6)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(np.random.get_state()[1], state)
    c = host_svds(A, k=6, rng=7)
    d = host_svds(A, k=6, random_state=np.random.default_rng(7))
    assert all(np.array_equal(x, y) for x, y in zip(c, d))
    assert not np.array_equal(a[0], c[0])
    assert np.abs(a[1] - c[1]).max() <= 1e-10 * a[1][-1]
    assert _SEED == EIGSH_SEED


def test_values_agree_with_scipy():
    A = random_sparse(300, 120)
    s = host_svds(A, k=6, return_singular_vectors=False)
    ref = scipy.sparse.linalg.svds(A, k=6, return_singular_vectors=False, random_state=0)
    assert np.abs(s - np.sort(ref)).max() <= 1e-10 * s[-1]


def test_numpy_backend_relations():
    """A V_m = U_m B by construction, A^T U_m = V_m B^T + beta V[m] e_m^T, both bases orthonormal"""
    A = random_sparse(300, 120)
    be = NumpyGKBackend(A)
    m = 12
    be.begin(m, np.random.default_rng(0).standard_normal(120))
    colproj, alpha, beta = be.extend(0, m)
    B = np.triu(colproj.T, 1) + np.diag(alpha)
    nrm = np.linalg.norm(A.toarray(), 2)
    U, V = be.U[:m], be.V[:m]
    assert np.abs(A @ V.T - U.T @ B).max() <= 1e-13 * nrm
    R = A.T @ U.T - V.T @ B.T
    R[:, m - 1] -= beta[m - 1] * be.V[m]
    assert np.abs(R).max() <= 1e-13 * nrm
    assert np.abs(U @ U.T - np.eye(m)).max() <= 1e-12 and np.abs(be.V @ be.V.T - np.eye(m + 1)).max() <= 1e-12
    s, info = gkl(NumpyGKBackend(A), A.shape, 3)
    assert np.abs(s - np.sort(np.linalg.svd(A.toarray(), compute_uv=False)[:3])).max() <= 1e-10 * nrm
