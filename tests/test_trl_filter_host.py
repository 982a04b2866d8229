"""The Chebyshev-filtered thick-restart driver of lanczos_amd.eigsh (trl_filtered), driven by its NumPy backend (no GPU)."""
import functools

import numpy as np
import pytest
from test_trl_host import _matrix, reference

import lanczos_amd
from lanczos_amd.eigsh import ChebFilter, NumpyBackend, check_filter_args, trl, trl_filtered

# (fixture, which, k): the cases of the filter's prototype
CASES = [
    ("deuteron1d_N1001_n1001", "SA", 6),
    ("deuteron1d_N1001_n1001", "SA", 20),
    ("lap2d_32x32_n30", "SA", 10),
    ("box1d_N500_n50", "SA", 20),
    ("deuteron3d_N12_27pt_n100", "SA", 6),
    ("deuteron3d_N12_27pt_n100", "SA", 10),
    ("graph_M2000_E7000_n40", "LA", 6),
    ("lap3d_8x8x8_n40", "LA", 8),
    ("c1_dense512_n20", "LA", 6),
    ("ragged_M700_n25", "LA", 4),
]


def start_vector(n):
    return np.random.default_rng(3).standard_normal(n)


@functools.lru_cache(maxsize=None)
def plain_steps(name, which, k):
    """Gram-Schmidt steps of the unfiltered loop on the same start vector (computed once per case)"""
    A, dense = _matrix(name)
    _, info = trl(NumpyBackend(A), dense.shape[0], k, which, v0=start_vector(dense.shape[0]))
    return info["matvecs"]


@pytest.mark.parametrize("degree", [16, 64])
@pytest.mark.parametrize("name,which,k", CASES)
def test_filtered_loop_finds_the_wanted_eigenpairs(name, which, k, degree):
    """ragged_M700_n25 LA 4 at degree 64 is the case that returns values wrong by 0.46 |A| without the range cap"""
    A, dense = _matrix(name)
    n = dense.shape[0]
    ref, nrm = reference(dense, which, k)
    be = NumpyBackend(A)
    theta, info = trl_filtered(be, n, k, which, degree, v0=start_vector(n))
    assert np.all(np.diff(theta) >= 0)
    assert np.abs(theta - ref).max() <= 1e-12 * nrm
    Y = be.get_vectors(k)
    assert np.linalg.norm(dense @ Y - Y * theta, axis=0).max() <= 1e-9 * nrm
    assert be.residuals(k, theta).max() <= 1e-9 * nrm
    assert np.abs(Y.T @ Y - np.eye(k)).max() <= 1e-12
    f = info["filter"]
    assert f["requested"] == degree and 2 <= f["degree"] <= degree
    assert info["matvecs"] == (info["steps"] - be.V.shape[0] + 1) * f["degree"] + be.V.shape[0] - 1 + k
    ev = np.linalg.eigvalsh(dense)  # the bounds are safe: the spectrum lies between the anchor and the far end of the damped interval
    assert min(f["anchor"], f["lo"]) <= ev[0] and ev[-1] <= max(f["anchor"], f["hi"])
    assert be.filter is None  # the backend is left unfiltered


@pytest.mark.parametrize("name,which,k", CASES)
def test_filter_halves_the_steps(name, which, k):
    A, dense = _matrix(name)
    n = dense.shape[0]
    _, info = trl_filtered(NumpyBackend(A), n, k, which, 16, v0=start_vector(n))
    assert info["steps"] <= plain_steps(name, which, k) / 2


@pytest.mark.parametrize("degree", [2, 3, 16])
@pytest.mark.parametrize("side", ["SA", "LA"])
def test_filter_matches_its_closed_form(degree, side):
    lo, hi, anchor = (1.0, 9.0, -0.5) if side == "SA" else (-3.0, 4.0, 5.5)
    far = hi if side == "SA" else lo
    d = np.linspace(anchor, far, 301)  # a diagonal matrix whose entries span the anchor .. the far end of the damped interval
    f = ChebFilter(lo, hi, anchor, degree)
    x = np.random.default_rng(degree).standard_normal(d.size)
    got = f.apply(lambda v: d * v, x)
    assert np.abs(got - f.poly(d) * x).max() <= 1e-13 * np.abs(x).max()
    p = f.poly(d)
    assert abs(f.poly(anchor) - 1.0) <= 1e-13 and np.abs(p).max() <= 1.0 + 1e-13
    inside = (d >= lo) & (d <= hi)
    assert np.abs(p[inside]).max() <= 1.0 / np.cosh(degree * np.arccosh(abs(anchor - f.c) / f.e)) * (1 + 1e-12)
    near = np.sort(np.abs(p[~inside]))  # monotone growth from the near edge to the anchor
    order = np.argsort(np.abs(d[~inside] - f.c))
    assert np.array_equal(np.abs(p[~inside])[order], near)
    D = np.diag(d)
    assert np.abs(ChebFilter(lo, hi, anchor, degree, A=D) @ x - got).max() <= 1e-14 * np.abs(x).max()  # `@`: a matrix to NumpyBackend


@pytest.mark.parametrize("degree", [2, 3, 16])
def test_coefficients_reproduce_apply(degree):
    A, dense = _matrix("lap2d_32x32_n30")
    f = ChebFilter(1.5, 8.1, -0.1, degree)
    coef = f.coefficients()
    assert coef.shape == (degree, 2) and coef[0, 1] == 0.0
    x = np.random.default_rng(1).standard_normal(dense.shape[0])
    prev, cur = x, x
    for a, b in coef:
        prev, cur = cur, a * (A @ cur - f.c * cur) - b * prev
    ref = f.apply(lambda v: A @ v, x)
    assert np.abs(cur - ref).max() <= 1e-14 * np.abs(ref).max()
    be = NumpyBackend(A)  # the backend's filtered product is the same statement
    be.set_filter(coef, f.c)
    assert np.array_equal(be._op(x), cur)
    be.set_filter(None)
    assert np.array_equal(be._op(x), A @ x)
    G = NumpyBackend(A)
    G.begin(5, x)
    G.extend(0, 5)
    assert np.abs(G.rayleigh(4) - G.V[:4] @ dense @ G.V[:4].T).max() <= 1e-13 * np.abs(dense).max()


def test_argument_errors():
    A, dense = _matrix("lap2d_32x32_n30")
    n = dense.shape[0]
    for which in ("SM", "LM"):
        with pytest.raises(ValueError, match="one end of the spectrum"):
            check_filter_args(which, 16)
        with pytest.raises(ValueError, match="one end of the spectrum"):
            trl_filtered(NumpyBackend(A), n, 4, which, 16)
        with pytest.raises(ValueError, match="one end of the spectrum"):  # raised before any device is touched
            lanczos_amd.eigsh(A, k=4, which=which, filter_degree=16)
    for bad in (1, 2.5, 0, -3, True, "16"):
        with pytest.raises(ValueError, match="filter_degree"):
            check_filter_args("SA", bad)
        with pytest.raises(ValueError, match="filter_degree"):
            lanczos_amd.eigsh(A, k=4, which="SA", filter_degree=bad)
    assert check_filter_args("LA", np.int64(2)) == 2
    with pytest.raises(ValueError):  # SciPy's own errors still come first
        trl_filtered(NumpyBackend(A), n, 0, "SA", 16)
    import scipy.sparse

    D = scipy.sparse.diags(np.repeat([1.0, 2.0, 3.0], 10)).tocsr()  # three distinct eigenvalues: the bounds stage breaks down
    with pytest.raises(ValueError, match="invariant"):
        trl_filtered(NumpyBackend(D), 30, 3, "SA", 16)


def test_no_filter_is_todays_path_and_runs_are_reproducible(monkeypatch):
    A, dense = _matrix("lap2d_32x32_n30")
    n = dense.shape[0]
    # filter_degree=None: eigsh takes the unfiltered loop with the same arguments as a call without the keyword
    import sys

    mod = sys.modules["lanczos_amd.eigsh"]  # (the package exports the function under the module's name)

    calls = []

    class FakeHandle:
        def close(self):
            pass

        def trl_get_vectors(self, k):
            return np.zeros((n, k))

        def trl_residuals(self, k, theta):
            return np.zeros(k)

    def fake_trl(backend, n_, k, **kw):
        calls.append(("trl", k, sorted(kw.items(), key=lambda t: t[0])))
        return np.arange(k, dtype=float), {"matvecs": 1}

    monkeypatch.setattr(mod, "upload_matrix", lambda h, A: n)
    monkeypatch.setattr(mod, "trl", fake_trl)
    monkeypatch.setattr(mod, "trl_filtered", lambda *a, **kw: pytest.fail("the filtered driver ran without filter_degree"))
    i1, i2 = {}, {}
    lanczos_amd.eigsh(A, k=4, which="SA", handle=FakeHandle(), info=i1)
    lanczos_amd.eigsh(A, k=4, which="SA", handle=FakeHandle(), info=i2, filter_degree=None)
    assert calls[0] == calls[1] and sorted(i1) == sorted(i2) == ["matvecs", "residuals"]
    monkeypatch.undo()
    # the unfiltered NumPy loop gives the same bits whether or not the backend ever had a filter
    a, ia = trl(NumpyBackend(A), n, 4, "SA")
    be = NumpyBackend(A)
    be.set_filter(ChebFilter(2.0, 8.0, 0.0, 4).coefficients(), 5.0)
    be.set_filter(None)
    b, ib = trl(be, n, 4, "SA")
    assert np.array_equal(a, b) and ia == ib
    # the global NumPy RNG is untouched, and the same call twice gives the same bits
    np.random.seed(7)
    before = np.random.get_state()
    be1, be2 = NumpyBackend(A), NumpyBackend(A)
    t1, info1 = trl_filtered(be1, n, 4, "SA", 16)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    t2, info2 = trl_filtered(be2, n, 4, "SA", 16)
    assert np.array_equal(t1, t2) and np.array_equal(be1.get_vectors(4), be2.get_vectors(4)) and info1 == info2
