"""lanczos_amd.eigs without a GPU: the Krylov-Schur outer loop (lanczos_amd/eigs.py) over the NumPy backend against the dense
eigenvalues and left / right vectors (scipy.linalg.eig) and against scipy.sparse.linalg.eigs(tol=0); the total order, split pairs,
breakdowns, an exhausted Krylov space, argument errors, ArpackNoConvergence, determinism and the untouched global RNG."""
import functools

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg

import lanczos_amd
from lanczos_amd import synthetic
from lanczos_amd.eigs import NumpyCplxBackend, _eigs, check_args, krylov_schur, total_order

EPS = np.finfo(np.float64).eps


def _convdiff2d(nx, ny, px, py):
    """5-point convection-diffusion: diagonal 4, off-diagonals -1 -+ p (upwind weights px, py); real spectrum, non-symmetric"""
    def line(n, p):
        return sp.diags([np.full(n - 1, -1.0 - p), np.full(n - 1, -1.0 + p)], [-1, 1])
    return (sp.kron(sp.identity(ny), line(nx, px) + 2.0 * sp.identity(nx)) + sp.kron(line(ny, py) + 2.0 * sp.identity(ny), sp.identity(nx))).tocsr()


def _rotations():
    """100 blocks [[a, b], [-b, a]] and the 1x1 blocks 1.5 and -1.7: a normal matrix with known conjugate pairs a +- i b"""
    rng = np.random.default_rng(11)
    a, b = rng.uniform(-1.0, 1.0, 100), rng.uniform(0.1, 1.0, 100)
    blocks = [np.array([[a[i], b[i]], [-b[i], a[i]]]) for i in range(100)] + [np.array([[1.5]]), np.array([[-1.7]])]
    return sp.block_diag(blocks).tocsr()


def _sprandn():
    """300 rows, 5 standard normal entries per row at random columns, plus diag(linspace(-2, 2))"""
    rng = np.random.default_rng(12)
    n = 300
    cols = np.concatenate([rng.choice(n, 5, replace=False) for _ in range(n)])
    A = sp.csr_matrix((rng.standard_normal(5 * n), (np.repeat(np.arange(n), 5), cols)), shape=(n, n))
    return (A + sp.diags(np.linspace(-2.0, 2.0, n))).tocsr()


_B3 = np.array([[1.0, 2.0, 0.0], [-1.5, 0.5, 1.0], [0.25, 0.0, -2.0]])


def _small12():
    rng = np.random.default_rng(13)
    return sp.csr_matrix(rng.standard_normal((12, 12)) + np.diag(np.arange(12.0)))


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "a":
        return _convdiff2d(20, 20, 0.3, 0.1)
    if name == "b":
        return _rotations()
    if name == "c":
        return _sprandn()
    if name == "d":
        return sp.kron(sp.identity(10), _B3).tocsr()
    if name == "e":
        return _small12()
    if name == "f":
        return synthetic.laplacian_2d_5pt(15, 15).to_scipy().tocsr()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def dense_reference(name):
    """the dense eigenvalues, ``|y^H x|`` of their unit left and right vectors and ``max|lambda|``: computed once, never changed"""
    lam, vl, vr = scipy.linalg.eig(matrix(name).toarray(), left=True, right=True)
    lam = np.asarray(lam, dtype=np.complex128)
    # LAPACK returns a pair as exact conjugates but a rounded real eigenvalue may carry no imaginary part at all: nothing to clean
    yx = np.abs(np.einsum("ij,ij->j", vl.conj(), vr))
    lam.setflags(write=False)
    yx.setflags(write=False)
    return {"lam": lam, "yx": yx, "amax": float(np.abs(lam).max())}


def true_residuals(A, w, X):
    return np.linalg.norm(A @ X - X * w, axis=0)


# (case, which, k, ncv); ncv None: the default.  scipy.sparse.linalg.eigs(tol=0)'s worst true residual |A x - lambda x| / max|lambda(A)|
# on the same case, measured on the host (ARPACK; the worst of its default start vector and two seeded ones), is the first value
# of SCIPY_RES; the bar of a case is ten times the larger of that and 1e-14 (the level the eigsh and svds tests hold).  The factor
# ten covers another summation order on the device.  This loop's own worst on the NumPy backend is recorded beside it for comparison
# only: it does not set the bar.
CASES = [
    ("a", "LM", 4, None), ("a", "LR", 4, None), ("a", "SR", 4, None), ("a", "LI", 4, None),
    ("b", "LM", 1, None), ("b", "LM", 4, None), ("b", "LR", 1, None), ("b", "LR", 4, None),
    ("b", "SR", 1, None), ("b", "SR", 4, None), ("b", "LI", 1, None), ("b", "LI", 4, None),
    ("c", "LM", 1, None), ("c", "LM", 4, None), ("c", "LR", 1, None), ("c", "LR", 4, None),
    ("c", "SR", 1, None), ("c", "SR", 4, None), ("c", "LI", 1, None), ("c", "LI", 4, None),
    ("d", "LM", 2, None), ("d", "LR", 2, None),
    ("e", "LM", 4, 12), ("e", "LR", 4, 8), ("e", "LI", 3, 12),
    ("f", "LR", 4, None), ("f", "SR", 4, None),
]
SCIPY_RES = {  # (case, which, k, ncv): (scipy's worst, this loop's worst on the NumPy backend),  # cycles and breakdowns of this loop
    ('a', 'LM', 4, None): (4.1e-15, 9.0e-15),  # cyc=20 bd=0
    ('a', 'LR', 4, None): (3.8e-15, 9.0e-15),  # cyc=20 bd=0
    ('a', 'SR', 4, None): (8.3e-16, 1.6e-15),  # cyc=20 bd=0
    ('a', 'LI', 4, None): (2.8e-15, 1.1e-14),  # cyc=24 bd=0
    ('b', 'LM', 1, None): (2.5e-15, 7.7e-15),  # cyc=7 bd=0
    ('b', 'LM', 4, None): (7.6e-15, 9.5e-15),  # cyc=23 bd=0
    ('b', 'LR', 1, None): (5.0e-15, 1.9e-15),  # cyc=11 bd=0
    ('b', 'LR', 4, None): (5.4e-15, 2.3e-14),  # cyc=80 bd=0
    ('b', 'SR', 1, None): (2.2e-15, 1.3e-14),  # cyc=8 bd=0
    ('b', 'SR', 4, None): (2.3e-14, 8.3e-14),  # cyc=339 bd=0
    ('b', 'LI', 1, None): (2.4e-15, 8.1e-15),  # cyc=26 bd=0
    ('b', 'LI', 4, None): (4.6e-15, 1.2e-14),  # cyc=97 bd=0
    ('c', 'LM', 1, None): (6.7e-15, 8.4e-15),  # cyc=14 bd=0
    ('c', 'LM', 4, None): (1.2e-14, 1.5e-14),  # cyc=30 bd=0
    ('c', 'LR', 1, None): (5.1e-15, 3.9e-15),  # cyc=13 bd=0
    ('c', 'LR', 4, None): (1.3e-14, 1.2e-14),  # cyc=30 bd=0
    ('c', 'SR', 1, None): (3.9e-15, 7.0e-15),  # cyc=20 bd=0
    ('c', 'SR', 4, None): (6.2e-15, 1.4e-14),  # cyc=27 bd=0
    ('c', 'LI', 1, None): (3.9e-15, 1.4e-14),  # cyc=52 bd=0
    ('c', 'LI', 4, None): (6.3e-15, 8.7e-15),  # cyc=91 bd=0
    ('d', 'LM', 2, None): (1.2e-15, 1.3e-15),  # cyc=1 bd=6
    ('d', 'LR', 2, None): (9.7e-16, 7.3e-16),  # cyc=1 bd=6
    ('e', 'LM', 4, 12): (1.0e-15, 1.3e-15),  # cyc=1 bd=0
    ('e', 'LR', 4, 8): (2.8e-15, 4.7e-15),  # cyc=25 bd=0
    ('e', 'LI', 3, 12): (1.0e-15, 1.0e-15),  # cyc=1 bd=0
    ('f', 'LR', 4, None): (4.4e-15, 4.5e-15),  # cyc=20 bd=0
    ('f', 'SR', 4, None): (4.1e-16, 1.2e-15),  # cyc=18 bd=0
}


def bar(case):
    return 10.0 * max(SCIPY_RES[case][0], 1e-14)


def primary(lam, which):
    lam = np.asarray(lam)
    return {"LM": -np.abs(lam), "LR": -lam.real, "SR": lam.real, "LI": -np.abs(lam.imag)}[which]


def wanted(name, which, k):
    """the k most wanted dense eigenvalues, most wanted first, and whether the k-th is the first half of a pair"""
    ref = dense_reference(name)
    order = total_order(ref["lam"], which)
    lam = ref["lam"][order[: k + 1]]
    split = bool(lam[k - 1].imag > 0 and lam[k] == lam[k - 1].conjugate())
    return lam[:k], split


def check_result(case, A, w, X, residuals=None):
    """the issue's bars on one result: true residuals, eigenvalues against the dense ones (first-order perturbation bound with a factor 2),
    completeness, order, unit columns"""
    name, which, k, _ = case
    ref = dense_reference(name)
    amax, b = ref["amax"], bar(case)
    assert w.dtype == np.complex128 and w.shape == (k,) and X.dtype == np.complex128 and X.shape == (A.shape[0], k)
    assert np.abs(np.linalg.norm(X, axis=0) - 1.0).max() <= 1e-13
    res = true_residuals(A, w, X)
    print(case, "true residual / max|lambda| =", res.max() / amax, "bar", b)
    assert res.max() <= b * amax
    near = np.abs(w[:, None] - ref["lam"][None, :]).argmin(axis=1)
    bound = 2.0 * b * amax / ref["yx"][near]
    print(case, "eigenvalue error / bound =", (np.abs(w - ref["lam"][near]) / bound).max())
    assert np.all(np.abs(w - ref["lam"][near]) <= bound)
    want, split = wanted(name, which, k)
    slack = max(bound.max(), (2.0 * b * amax / ref["yx"][total_order(ref["lam"], which)[:k]]).max())
    assert np.abs(np.sort(primary(w, which)) - np.sort(primary(want, which))).max() <= slack
    assert np.all(np.diff(primary(w, which)) >= -2 * slack)  # most wanted first
    if name != "d":  # (d has every eigenvalue ten times over: the order among rounded copies of one value is not pinned)
        assert np.array_equal(total_order(w, which), np.arange(k))
    if split:  # the k-th value is half of a pair: the positive-imaginary member comes back, without its conjugate
        assert w[-1].imag > 0 and not np.any(np.abs(w[:-1] - w[-1].conjugate()) <= slack)
    for i in range(k):  # every other complex value comes with its conjugate right behind it
        if w[i].imag > 0 and not (split and i == k - 1):
            assert w[i + 1] == w[i].conjugate() and np.array_equal(X[:, i + 1], X[:, i].conjugate())
    if residuals is not None:
        assert np.abs(np.asarray(residuals) - res).max() <= 10 * A.shape[0] * EPS * amax
    return res.max() / amax


def run_host(case, **kw):
    name, which, k, ncv = case
    A = matrix(name)
    be = NumpyCplxBackend(A)
    info = {}
    w, X = _eigs(be, A.shape[0], k, which, ncv, kw.get("maxiter"), kw.get("tol", 0), kw.get("v0"), True, info)
    return A, w, X, info


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-k{c[2]}" + (f"-ncv{c[3]}" if c[3] else ""))
def test_krylov_schur_on_the_numpy_backend(case):
    A, w, X, info = run_host(case)
    check_result(case, A, w, X, info["residuals"])
    assert info["cycles"] >= 1 and info["matvecs"] >= (case[3] or 20) and info["anorm"] > 0
    if case[0] == "d":  # the Krylov space of any start vector has dimension 3
        assert info["breakdowns"] >= 3
    else:
        assert info["breakdowns"] == 0
    if case[3] == 12:  # ncv = n: the space is exhausted after one cycle
        assert info["cycles"] == 1


def test_split_pairs_occur_for_every_which():
    """kq = k + 1: for every ``which`` at least one of the cases above ends in the first half of a conjugate pair"""
    seen = {which for name, which, k, _ in CASES if wanted(name, which, k)[1]}
    assert seen == {"LM", "LR", "SR", "LI"}


def test_symmetric_matrix_agrees_with_eigvalsh():
    A = matrix("f")
    ev = np.linalg.eigvalsh(A.toarray())
    for which, ref in (("LR", ev[::-1][:4]), ("SR", ev[:4])):
        _, w, _, _ = run_host(("f", which, 4, None))
        assert np.all(w.imag == 0)
        assert np.abs(w.real - ref).max() <= 2 * bar(("f", which, 4, None)) * np.abs(ev).max()


def test_against_scipy_eigs():
    for case in (("a", "LR", 4, None), ("b", "LI", 4, None), ("c", "LM", 4, None)):
        name, which, k, _ = case
        A, w, _, _ = run_host(case)
        ws = scipy.sparse.linalg.eigs(A, k=k, which=which, tol=0, return_eigenvectors=False)
        ref = dense_reference(name)
        tol = 4 * bar(case) * ref["amax"] / ref["yx"].min()
        assert np.abs(np.sort(primary(ws, which)) - np.sort(primary(w, which))).max() <= tol


def test_total_order():
    lam = np.array([1 + 2j, 1 - 2j, 3.0, -3.0, 0.5j, -0.5j, 2.0])
    assert list(total_order(lam, "LM")) == [2, 3, 0, 1, 6, 4, 5]
    assert list(total_order(lam, "LR")) == [2, 6, 0, 1, 4, 5, 3]
    assert list(total_order(lam, "SR")) == [3, 4, 5, 0, 1, 6, 2]
    assert list(total_order(lam, "LI")) == [0, 1, 4, 5, 2, 3, 6]
    assert list(total_order(np.array([1.0, -2.0, 2.0, 0.5]), "LI")) == [2, 1, 0, 3]  # a real spectrum: all ties, broken by -|.|, -Re


def test_argument_errors():
    A = matrix("e")
    for kw in ({"M": A}, {"sigma": 0.5}, {"Minv": A}, {"OPinv": A}, {"OPpart": "r"}, {"which": "SM"}, {"which": "SI"}):
        with pytest.raises(NotImplementedError):
            lanczos_amd.eigs(A, k=2, **kw)
    with pytest.raises(NotImplementedError):
        lanczos_amd.eigs(A.astype(np.complex128), k=2)
    with pytest.raises(NotImplementedError):
        lanczos_amd.eigs(A.toarray() + 0j, k=2)
    for which in ("LA", "SA", "BE", "lm", ""):
        with pytest.raises(ValueError):
            lanczos_amd.eigs(A, k=2, which=which)
    for k in (0, -1):
        with pytest.raises(ValueError):
            lanczos_amd.eigs(A, k=k)
    for k in (11, 12, 40):
        with pytest.raises(TypeError):
            lanczos_amd.eigs(A, k=k)
    for k, ncv in ((4, 6), (4, 13), (9, 11), (2, 4)):
        with pytest.raises(ValueError):
            lanczos_amd.eigs(A, k=k, ncv=ncv)
    with pytest.raises(ValueError):
        lanczos_amd.eigs(matrix("c"), k=4, ncv=129)
    with pytest.raises(ValueError):
        lanczos_amd.eigs(sp.csr_matrix(np.ones((4, 5))), k=1)
    assert check_args(400, 6, "LM", None) == 20 and check_args(400, 12, "LR", None) == 25 and check_args(12, 4, "LI", None) == 12
    assert check_args(12, 4, "SR", 7) == 7  # k + 3
    be = NumpyCplxBackend(A)
    for v0 in (np.zeros(12), np.ones(11)):
        with pytest.raises(ValueError):
            krylov_schur(be, 12, 2, v0=v0)
    be.begin(4, np.ones(12))
    with pytest.raises(ValueError):
        be.residuals_cplx(2, [1.0, 1.0], [0.0, 0.5])  # a lone positive im at k - 1


def test_no_convergence_carries_the_converged_pairs():
    case = ("c", "LM", 4, None)
    A = matrix("c")
    with pytest.raises(scipy.sparse.linalg.ArpackNoConvergence) as e:
        run_host(case, maxiter=2)
    err = e.value
    assert err.info["cycles"] == 2 and err.eigenvectors.shape == (300, len(err.eigenvalues)) and len(err.eigenvalues) < 4
    if len(err.eigenvalues):
        assert true_residuals(A, err.eigenvalues, err.eigenvectors).max() <= bar(case) * dense_reference("c")["amax"]
    # a loose tolerance converges some pairs but not all within two cycles: they pass the bar that tolerance sets
    with pytest.raises(scipy.sparse.linalg.ArpackNoConvergence) as e:
        run_host(("c", "LR", 4, None), maxiter=8, tol=1e-6)
    err = e.value
    assert 0 < len(err.eigenvalues) < 4 and err.eigenvalues.dtype == np.complex128
    res = true_residuals(A, err.eigenvalues, err.eigenvectors)
    assert res.max() <= 10 * 1e-6 * dense_reference("c")["amax"]
    for i, l in enumerate(err.eigenvalues):  # no half pairs
        if l.imag != 0:
            assert np.any(err.eigenvalues == l.conjugate())


def test_same_call_same_bits_and_global_rng_untouched():
    case = ("d", "LM", 2, None)  # (breakdowns: the private generator is drawn from)
    state = np.random.get_state()
    _, w1, X1, i1 = run_host(case)
    _, w2, X2, i2 = run_host(case)
    assert np.array_equal(w1, w2) and np.array_equal(X1, X2) and np.array_equal(i1["residuals"], i2["residuals"])
    assert i1["breakdowns"] == i2["breakdowns"] > 0
    now = np.random.get_state()
    assert now[0] == state[0] and np.array_equal(now[1], state[1]) and now[2:] == state[2:]
    case = ("c", "LI", 1, None)
    _, w1, X1, _ = run_host(case)
    _, w2, X2, _ = run_host(case)
    assert np.array_equal(w1, w2) and np.array_equal(X1, X2)
