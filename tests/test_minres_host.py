"""``lanczos_amd.minres`` on the host: ``solve`` over ``NumpyMinresBackend``, the restatement of the device calls with the same lagged
update and flush, against the true residual, the longdouble loop of tests/minres_reference.py and SciPy; the argument errors, which
need no device."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla
from minres_reference import lap1d_periodic, lap2d, loop

from lanczos_amd import minres
from lanczos_amd.minres import NumpyMinresBackend

SHIFT = 1.7003  # inside the spectrum of lap2d(33, 31): indefinite


@functools.lru_cache(maxsize=None)
def problem(name):
    """``(A, b, shift)``"""
    if name == "periodic":
        A = lap1d_periodic(200)
        b = np.random.default_rng(5).standard_normal(200)
        return A, b - b.mean(), 0.0  # mean-free: consistent with the singular matrix
    A = lap2d(33, 31)
    b = np.random.default_rng(0).standard_normal(A.shape[0])
    return A, b, (SHIFT if name == "indefinite" else 0.0)


def run(name, **kw):
    A, b, shift = problem(name)
    info = {}
    x, code = minres(A, b, shift=shift, info=info, _backend=NumpyMinresBackend(A), **kw)
    res = np.linalg.norm(b - (A @ x - shift * x)) / np.linalg.norm(b)
    return x, code, info, res


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("name", ["definite", "indefinite", "periodic"])
def test_residual_at_the_tolerance(name, rtol):
    x, code, info, res = run(name, rtol=rtol)
    print(f"{name} rtol {rtol:g}: {info['iterations']} steps, |b - (A - shift) x| / |b| = {res:.3e} = {res / rtol:.3f} rtol")
    assert code == 0
    assert res <= 2 * rtol
    h = info["history"]
    assert len(h) == info["iterations"] and np.all(np.diff(h) <= 0.0)
    assert info["residual_estimate"] == h[-1] <= rtol * info["beta1"]
    assert info["chunks"] == -(-info["iterations"] // 8)


def test_chunking_does_not_change_the_result():
    x32 = run("definite", rtol=1e-8, check_every=32)[0]
    for check_every in (1, 7, 8, 1000):
        assert np.array_equal(run("definite", rtol=1e-8, check_every=check_every)[0], x32)


def test_eigenvector_stops_after_one_step():
    A = lap2d(33, 31)
    lam, U = np.linalg.eigh(A.toarray())
    info = {}
    x, code = minres(A, U[:, 17], rtol=1e-10, info=info, _backend=NumpyMinresBackend(A))
    assert code == 0 and info["iterations"] == 1
    assert np.linalg.norm(x - U[:, 17] / lam[17]) <= 1e-12 * np.linalg.norm(x)


def test_maxiter_returns_the_fifth_iterate():
    A, b, shift = problem("indefinite")
    x, code, info, _ = run("indefinite", rtol=1e-10, maxiter=5)
    assert code == 5 and info["iterations"] == 5
    ref = np.asarray(loop(A, b, shift, 5)["x"], dtype=np.float64)
    assert np.linalg.norm(x - ref) <= 1e-12 * np.linalg.norm(ref)


def test_x0_with_a_shift_starts_from_the_right_residual():
    A, b, shift = problem("indefinite")
    x0 = np.random.default_rng(3).standard_normal(A.shape[0])
    info = {}
    x, code = minres(A, b, x0, shift=shift, rtol=1e-8, info=info, _backend=NumpyMinresBackend(A))
    r0 = np.linalg.norm(b - (A @ x0 - shift * x0))
    assert abs(info["beta1"] - r0) <= 1e-14 * r0
    assert code == 0 and np.linalg.norm(b - (A @ x - shift * x)) <= 2e-8 * r0


def test_shapes():
    A, b, _ = problem("definite")
    x1, _ = minres(A, b, rtol=1e-8, _backend=NumpyMinresBackend(A))
    x2, _ = minres(A, b[:, None], rtol=1e-8, _backend=NumpyMinresBackend(A))
    assert x1.shape == x2.shape == (A.shape[0],) and x1.dtype == np.float64 and np.array_equal(x1, x2)


def test_zero_right_hand_side():
    A = lap2d(5, 4)
    x, code = minres(A, np.zeros(20))  # (answered before any device is asked for)
    assert code == 0 and np.array_equal(x, np.zeros(20))
    x0 = np.arange(20.0)
    x, code = minres(A, np.zeros((20, 1)), x0)
    assert code == 0 and np.array_equal(x, x0)


def test_n_equals_one():
    x, code = minres(np.array([[4.0]]), np.array([2.0]), shift=-1.0)
    assert code == 0 and x.shape == (1,) and x[0] == 0.4
    x, code = minres(sp.csr_matrix(np.array([[4.0]])), np.array([[2.0]]))
    assert code == 0 and x[0] == 0.5


def test_callback_sees_every_iterate():
    seen = []
    x, code, info, _ = run("definite", rtol=1e-6, callback=lambda xk: seen.append(xk.copy()))
    assert code == 0 and len(seen) == info["iterations"] == info["chunks"]
    assert np.array_equal(seen[-1], x)
    assert np.array_equal(x, run("definite", rtol=1e-6)[0])


def test_check_raises_on_a_non_symmetric_matrix():
    A = lap2d(6, 5).tolil()
    A[0, 7] = 3.0
    A = A.tocsr()
    with pytest.raises(ValueError, match="non-symmetric"):
        minres(A, np.ones(30), check=True, _backend=NumpyMinresBackend(A))
    S = lap2d(6, 5)
    x, code = minres(S, np.ones(30), check=True, rtol=1e-10, _backend=NumpyMinresBackend(S))
    assert code == 0


def test_argument_errors_need_no_device():
    A = lap2d(4, 3)
    b = np.ones(12)
    with pytest.raises(NotImplementedError, match="M"):
        minres(A, b, M=sp.eye(12))
    with pytest.raises(NotImplementedError, match="complex A"):
        minres(A.astype(np.complex128), b)
    with pytest.raises(NotImplementedError, match="complex b"):
        minres(A, b + 1j)
    with pytest.raises(ValueError, match="square"):
        minres(sp.csr_matrix(np.ones((3, 4))), np.ones(3))
    with pytest.raises(ValueError, match="incompatible"):
        minres(A, np.ones(11))
    with pytest.raises(ValueError, match="check_every"):
        minres(A, b, check_every=0)


def test_against_scipy():
    A, b, _ = problem("definite")
    x = run("definite", rtol=1e-10)[0]
    xs, code = sla.minres(A, b, rtol=1e-10)
    assert code == 0
    err = np.linalg.norm(x - xs) / np.linalg.norm(x)
    print(f"|x - x_scipy| / |x| = {err:.3e}")
    assert err <= 1e-7
