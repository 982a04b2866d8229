"""``lsmr`` without a GPU: the host loop over ``NumpyLsmrBackend`` - the restatement of the device's calls with its lag, its
un-normalised vectors and its one deviation from SciPy (the tests of step ``k`` use ``|x_{k-1}|``) - against
``scipy.sparse.linalg.lsmr`` on the family ``F`` of tests/lsmr_reference.py, through every ``istop`` code, and the argument
handling that runs before any device is asked for."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from lsmr_reference import family, loop, rhs

import lanczos_amd
from lanczos_amd import _capi, lsmr
from lanczos_amd.lsmr import NumpyLsmrBackend

SHAPES = [(4000, 1500), (1500, 4000), (600, 200), (200, 600)]
CASES = [(shape, consistent, damp, tol) for shape in SHAPES for consistent in (True, False) for damp in (0.0, 0.5) for tol in (1e-6, 1e-10)]


def case_id(case):
    (m, n), consistent, damp, tol = case
    return f"{m}x{n}-{'consistent' if consistent else 'inconsistent'}-damp{damp:g}-{tol:g}"


@functools.lru_cache(maxsize=None)
def problem(shape, consistent):
    A = family(*shape)
    return A, rhs(A, consistent)


@functools.lru_cache(maxsize=None)
def scipy_result(case):
    shape, consistent, damp, tol = case
    A, b = problem(shape, consistent)
    return spla.lsmr(A, b, damp=damp, atol=tol, btol=tol)


def host(A, b, *args, **kw):
    return lsmr(A, b, *args, _backend=NumpyLsmrBackend(A), **kw)


# ---------------------------------------------------------------- 1. against SciPy on F
WORST = {"x": 0.0}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_against_scipy(case):
    shape, consistent, damp, tol = case
    A, b = problem(shape, consistent)
    ref = scipy_result(case)
    info = {}
    got = host(A, b, damp, tol, tol, info=info)
    err = np.linalg.norm(got[0] - ref[0]) / np.linalg.norm(ref[0])
    WORST["x"] = max(WORST["x"], err)
    print(f"{case_id(case)}: istop {got[1]} (scipy {ref[1]}), itn {got[2]} (scipy {ref[2]}), |x - x_scipy| / |x_scipy| {err:.2e}, "
          f"worst so far {WORST['x']:.2e}")
    assert got[1] == ref[1]
    assert abs(got[2] - ref[2]) <= 1
    assert err <= 1e-12
    assert info["iterations"] == got[2] and info["history"].shape == (got[2], 2)
    assert info["history"][-1, 0] == got[3] and info["history"][-1, 1] == got[4]
    assert got[7] == np.linalg.norm(got[0])  # normx is the true norm of the returned x
    for g, r in zip(got[3:7], ref[3:7]):  # normr, normar, normA, condA: SciPy's estimates at the same step
        if got[2] == ref[2]:
            assert abs(g - r) <= 1e-6 * abs(r) + 1e-12 * np.linalg.norm(b)


# ---------------------------------------------------------------- 2. chunking
def _backend_after(A, b, damp, chunks):
    be = NumpyLsmrBackend(A)
    be.begin(b, None, damp)
    for c in chunks:
        st = be.run(c, 0.0, 0.0, 0.0)
    return be, st


@pytest.mark.parametrize("shape", [(600, 200), (200, 600)])
def test_six_single_steps_equal_one_chunk_of_six(shape):
    A, b = problem(shape, False)
    one, st1 = _backend_after(A, b, 0.25, [1] * 6)
    six, st6 = _backend_after(A, b, 0.25, [6])
    assert st1 == st6 and st6["iterations"] == 6 and not st6["done"]
    for key in ("x", "uh", "vh", "h", "hbar"):
        assert np.array_equal(getattr(one, key), getattr(six, key)), key
    assert one.s == six.s and one.nu_u == six.nu_u and one.nu_v == six.nu_v
    assert np.array_equal(one.history(6), six.history(6))
    ref = np.asarray(loop(A, b, 0.25, 6)["x_out"], dtype=np.float64)
    assert np.linalg.norm(six.x - ref) <= 1e-12 * np.linalg.norm(ref)


# ---------------------------------------------------------------- 3. every istop code
def unit(n, *entries):
    b = np.zeros(n)
    for i, v in entries:
        b[i - 1] = v
    return b


def ill_conditioned():
    rng = np.random.default_rng(0)
    Q1, _ = np.linalg.qr(rng.standard_normal((60, 40)))
    Q2, _ = np.linalg.qr(rng.standard_normal((40, 40)))
    return Q1 @ np.diag(np.logspace(0, -8, 40)) @ Q2.T, rng.standard_normal(60)


def test_istop_0_zero_is_the_solution():
    E = sp.eye(7, 4).tocsr()
    b = unit(7, (6, 2.0))  # orthogonal to the range of E
    got, ref = host(E, b), spla.lsmr(E, b)
    assert got[1] == ref[1] == 0 and got[2] == ref[2] == 0
    assert np.array_equal(got[0], np.zeros(4)) and got[3] == 2.0 and got[4] == 0.0


def test_istop_1_beta_vanishes_exactly():
    E = sp.eye(7, 4).tocsr()
    b = unit(7, (2, 3.0))
    got, ref = host(E, b), spla.lsmr(E, b)
    assert ref[1] == 1 and ref[2] == 1
    assert got[1] == 1 and got[2] == 1 and np.array_equal(got[0], unit(4, (2, 3.0)))
    assert got[3] == 0.0 and got[7] == 3.0


def test_istop_2_inconsistent():
    E = sp.eye(7, 4).tocsr()
    b = unit(7, (2, 3.0), (7, 1.0))
    got, ref = host(E, b), spla.lsmr(E, b)
    assert ref[1] == 2 and ref[2] == 1
    assert got[1] == 2 and got[2] == 1 and np.allclose(got[0], unit(4, (2, 3.0)), rtol=0, atol=1e-15)
    assert abs(got[3] - 1.0) <= 1e-15


def test_istop_1_wide():
    E = sp.eye(4, 7).tocsr()
    b = np.array([1.0, 2.0, 3.0, 4.0])
    got, ref = host(E, b), spla.lsmr(E, b)
    assert ref[1] == 1 and ref[2] == 1
    assert got[1] == 1 and got[2] == 1 and np.allclose(got[0], np.r_[b, 0, 0, 0], rtol=0, atol=1e-14)


def test_istop_3_conlim():
    D, b = ill_conditioned()
    ref = spla.lsmr(D, b, conlim=1e4, atol=1e-15, btol=1e-15, maxiter=400)
    got = host(D, b, 0.0, 1e-15, 1e-15, 1e4, 400)
    assert ref[1] == 3 and ref[2] == 55
    assert got[1] == 3 and abs(got[2] - ref[2]) <= 1 and got[6] >= 1e4


@pytest.mark.parametrize("consistent", [True, False], ids=["consistent", "inconsistent"])
def test_istop_4_or_5_machine_precision(consistent):
    A, b = problem((600, 200), consistent)
    ref = spla.lsmr(A, b, atol=0.0, btol=0.0, conlim=0.0)
    got = host(A, b, 0.0, 0.0, 0.0, 0.0)
    print(f"atol = btol = conlim = 0, consistent {consistent}: istop {got[1]} at {got[2]} (scipy {ref[1]} at {ref[2]})")
    assert ref[1] in (4, 5)
    assert got[1] == ref[1] and abs(got[2] - ref[2]) <= 1


def test_istop_7_maxiter():
    A, b = problem((600, 200), False)
    ref = spla.lsmr(A, b, atol=1e-12, btol=1e-12, maxiter=5)
    for check_every in (1, 2, 8):
        got = host(A, b, 0.0, 1e-12, 1e-12, 1e8, 5, check_every=check_every)
        assert ref[1] == 7 and got[1] == 7 and got[2] == 5
        assert np.linalg.norm(got[0] - ref[0]) <= 1e-14 * np.linalg.norm(ref[0])


def test_nan_input_stops_at_once():
    A, b = problem((600, 200), False)
    bad = b.copy()
    bad[3] = np.nan
    got = host(A, bad)
    assert got[1] == 7 and got[2] == 0
    B = A.copy()
    B.data[5] = np.inf
    got = host(B, b, maxiter=50)
    assert got[1] == 7 and got[2] <= 2


# ---------------------------------------------------------------- 4. arguments and trivial inputs
def test_x0():
    A, b = problem((600, 200), True)
    x0 = np.random.default_rng(3).standard_normal(200)
    be = NumpyLsmrBackend(A)
    be.begin(b, x0, 0.0)
    r0 = np.linalg.norm(b - A @ x0)
    assert abs(be.run(0, 0, 0, 0)["normr"] - r0) <= 1e-14 * r0
    info = {}
    x, istop, itn, normr, normar, normA, condA, normx = lsmr(A, b, 0.0, 1e-9, 1e-9, x0=x0.reshape(-1, 1), _backend=be, info=info)
    ref = spla.lsmr(A, b, atol=1e-9, btol=1e-9, x0=x0)
    assert istop == ref[1] == 1 and abs(itn - ref[2]) <= 1
    assert np.linalg.norm(b - A @ x) <= 1e-9 * np.linalg.norm(b) + 1e-9 * normA * np.linalg.norm(x)
    assert normx == np.linalg.norm(x)


def test_argument_errors_need_no_device(monkeypatch):
    def no_device(*args, **kw):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(_capi, "Handle", no_device)
    A = family(30, 20)
    b = np.ones(30)
    with pytest.raises(NotImplementedError):
        lsmr(A.astype(np.complex128), b)
    with pytest.raises(NotImplementedError):
        lsmr(A, b.astype(np.complex128))
    with pytest.raises(NotImplementedError):
        lsmr(A, b, x0=np.ones(20, dtype=np.complex128))
    with pytest.raises(NotImplementedError):
        lsmr(spla.aslinearoperator(A), b)
    for bad in (np.ones(29), np.ones((30, 2)), np.ones((1, 30))):
        with pytest.raises(ValueError):
            lsmr(A, bad)
    with pytest.raises(ValueError):
        lsmr(A, b, x0=np.ones(30))
    with pytest.raises(ValueError):
        lsmr(np.ones(30), b)
    for kw in ({"damp": -1.0}, {"atol": -1e-3}, {"btol": -1e-3}, {"maxiter": -1}, {"check_every": 0}):
        with pytest.raises(ValueError):
            lsmr(A, b, **kw)
    # the trivial answers need none either
    assert np.array_equal(lsmr(A, np.zeros(30))[0], np.zeros(20)) and lsmr(A, np.zeros((30, 1)))[1:3] == (0, 0)
    assert lsmr(np.ones((5, 1)), np.arange(5.0))[0].shape == (1,)


def test_signature_is_scipys():
    import inspect

    ours = inspect.signature(lsmr).parameters
    theirs = inspect.signature(spla.lsmr).parameters
    assert list(ours)[: len(theirs)] == list(theirs)
    for name, p in theirs.items():
        assert ours[name].default == p.default and ours[name].kind == p.kind
    assert all(ours[name].kind == inspect.Parameter.KEYWORD_ONLY for name in list(ours)[len(theirs):])
    assert lanczos_amd.lsmr is lsmr and "lsmr" in lanczos_amd.__all__


@pytest.mark.parametrize("damp", [0.0, 0.7])
@pytest.mark.parametrize("shape", [(9, 1), (1, 9)])
def test_one_row_or_one_column(shape, damp):
    rng = np.random.default_rng(sum(shape))
    for A in (rng.standard_normal(shape), sp.csr_matrix(rng.standard_normal(shape))):
        b = rng.standard_normal(shape[0])
        x = lsmr(A, b, damp)[0]
        Ad = A.toarray() if sp.issparse(A) else A
        aug = np.vstack([Ad, damp * np.eye(shape[1])])
        ref = np.linalg.lstsq(aug, np.r_[b, np.zeros(shape[1])], rcond=None)[0]
        assert x.shape == (shape[1],) and np.linalg.norm(x - ref) <= 1e-14 * np.linalg.norm(ref)


def test_b_zero():
    A = family(30, 20)
    out = lsmr(A, np.zeros(30), x0=np.ones(20))
    assert np.array_equal(out[0], np.zeros(20)) and out[1:] == (0, 0, 0.0, 0.0, 0.0, 1.0, 0.0)


def test_show_prints_a_line_per_chunk(capsys):
    A, b = problem((600, 200), True)
    info = {}
    host(A, b, show=True, check_every=4, info=info)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("lsmr: chunk")]
    assert len(lines) == info["chunks"] == -(-info["iterations"] // 4)
