"""``cg`` on the host: the loop of lanczos_amd/cg.py on its NumPy backend (a restatement of the device calls) against SciPy's ``cg``
with the same diagonal preconditioner and the loops of tests/cg_reference.py, on cases admitted by that file's rule; the chunking,
the forms of ``M``, the exits, the deviations from SciPy and every argument error.  No GPU."""
import functools
import inspect

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla
from bicgstab_reference import skew64
from cg_reference import MATRICES, admission, diagonal_of, loop

import lanczos_amd
from lanczos_amd import StencilOperator, _capi, cg
from lanczos_amd.cg import NumpyCgBackend, check_cg_args, solve

# (matrix, preconditioner, rtol) -> the two seeds used, each admitted (test_every_case_is_admitted); found among seeds 0 .. 11
SEEDS = {
    ("lap24x20", "plain", 1e-6): (0, 2), ("lap24x20", "plain", 1e-10): (0, 1),
    ("lap24x20", "jacobi", 1e-6): (0, 2), ("lap24x20", "jacobi", 1e-10): (0, 1),
    ("lap33x31", "plain", 1e-6): (0, 1), ("lap33x31", "plain", 1e-10): (1, 2),
    ("sym401", "plain", 1e-6): (0, 2), ("sym401", "plain", 1e-10): (0, 1),
    ("dense130", "plain", 1e-6): (1, 2), ("dense130", "plain", 1e-10): (0, 1),
    ("dense130", "jacobi", 1e-6): (0, 1), ("dense130", "jacobi", 1e-10): (0, 1),
    ("well33x31", "jacobi", 1e-6): (0, 1), ("well33x31", "jacobi", 1e-10): (0, 1),
}
CASES = [(name, pre, rtol, seed) for (name, pre, rtol), seeds in SEEDS.items() for seed in seeds]
X_MARGIN = 16.0  # a further summation order may sit this many times the admission runs' own spread in x away


@functools.lru_cache(maxsize=None)
def matrix(name):
    return MATRICES[name]()


@functools.lru_cache(maxsize=None)
def jacobi(name):
    d = 1.0 / diagonal_of(matrix(name))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def problem(name, pre, rtol, seed):
    """``(A, b, d or None, admission record)``, computed once and shared (tests/test_gpu_cg.py reads it too); nothing changes it"""
    A = matrix(name)
    b = np.random.default_rng(seed).standard_normal(A.shape[0])
    b.setflags(write=False)
    d = jacobi(name) if pre == "jacobi" else None
    return A, b, d, admission(A, b, rtol, d)


@functools.lru_cache(maxsize=None)
def well_plain(rtol, seed):
    """``well33x31`` without a preconditioner: admitted for no seed, so only the longdouble run's count is kept"""
    A = matrix("well33x31")
    b = np.random.default_rng(seed).standard_normal(A.shape[0])
    b.setflags(write=False)
    atol_eff = rtol * float(np.linalg.norm(b))
    return A, b, atol_eff, loop(A, b, atol_eff, 10 * A.shape[0], "longdouble")["iterations"]


def _count():
    calls = []
    return calls, (lambda xk: calls.append(np.array(xk)))


def _M(d):
    return None if d is None else sp.diags(d)


# ---------------------------------------------------------------- admission and stops
@pytest.mark.parametrize("name,pre,rtol,seed", CASES)
def test_every_case_is_admitted(name, pre, rtol, seed):
    adm = problem(name, pre, rtol, seed)[3]
    print(f"{name} {pre} rtol {rtol:g} seed {seed}: {adm['runs']['dot']['iterations']} iterations, margin {adm['margin']:.3f}, "
          f"spread {adm['spread']:.2e}")
    assert adm["same_stop"] and adm["admitted"]


# ---------------------------------------------------------------- agreement with SciPy
@pytest.mark.parametrize("name,pre,rtol,seed", CASES)
def test_numpy_backend_against_scipy_and_the_reference(name, pre, rtol, seed):
    A, b, d, adm = problem(name, pre, rtol, seed)
    calls_s, cb_s = _count()
    xs, info_s = sla.cg(A, b, rtol=rtol, M=_M(d), callback=cb_s)
    calls, cb = _count()
    run = {}
    x, info = cg(A, b, rtol=rtol, M=_M(d), callback=cb, info=run, _backend=NumpyCgBackend(A))
    assert info == info_s == 0 and len(calls) == len(calls_s)
    ref = adm["runs"]["dot"]
    assert (run["exit"], run["iterations"], run["code"]) == ("converged", ref["iterations"], 0)
    assert len(calls) == ref["callbacks"] == run["iterations"] and run["products"] == run["iterations"]
    assert run["preconditioner"] == (None if d is None else "diagonal") and run["indefinite_at"] is None
    dist = float(np.linalg.norm(x - xs))
    print(f"{name} {pre} rtol {rtol:g} seed {seed}: {run['iterations']} iterations, |x - x_scipy| {dist:.2e}, spread in x "
          f"{adm['x_spread']:.2e}, ratio {dist / adm['x_spread']:.2f}")
    assert dist <= X_MARGIN * adm["x_spread"]
    assert run["residual_norm"] < run["atol_effective"] == adm["atol_eff"]
    # the recurrence's tested norms are the reference run's, and the true residual meets the bar
    assert np.array_equal(run["history"], ref["tests"]) and run["history"][-1] == run["residual_norm"]
    true = np.asarray(A @ x).ravel() - b
    assert np.linalg.norm(true) <= 2.0 * adm["atol_eff"]
    assert np.array_equal(calls[-1], x)


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
def test_the_well_needs_its_preconditioner(rtol):
    """``well33x31`` plain is admitted for no seed (its hundreds of iterations amplify the summation order): it is held to the code,
    the true residual and to needing at least four times the iterations of its Jacobi run, never to a count"""
    A, b, atol_eff, ref_its = well_plain(rtol, 0)
    jac = problem("well33x31", "jacobi", rtol, 0)[3]["runs"]["dot"]["iterations"]
    run = {}
    x, info = cg(A, b, rtol=rtol, info=run, _backend=NumpyCgBackend(A))
    true = np.linalg.norm(np.asarray(A @ x).ravel() - b)
    print(f"well33x31 rtol {rtol:g}: plain {run['iterations']} iterations (longdouble {ref_its}), jacobi {jac}, true residual / atol_eff "
          f"{true / atol_eff:.3f}")
    assert info == 0 and run["code"] == 0 and true <= 2.0 * atol_eff
    assert run["iterations"] >= 4 * jac and ref_its >= 11 * jac


# ---------------------------------------------------------------- check_every and the forms of M
@pytest.mark.parametrize("name,pre,rtol,seed", [("lap24x20", "plain", 1e-10, 0), ("sym401", "plain", 1e-6, 0), ("dense130", "jacobi", 1e-10, 1),
                                                ("well33x31", "jacobi", 1e-6, 0)])
def test_check_every_does_not_change_a_bit(name, pre, rtol, seed):
    A, b, d, _ = problem(name, pre, rtol, seed)
    out = []
    for every in (1, 8, 256):
        run = {}
        x, info = cg(A, b, rtol=rtol, M=_M(d), check_every=every, info=run, _backend=NumpyCgBackend(A))
        out.append((x, info, run["iterations"], run["exit"], run["history"]))
    for x, info, its, kind, hist in out[1:]:
        assert np.array_equal(x, out[0][0]) and (info, its, kind) == out[0][1:4] and np.array_equal(hist, out[0][4])
    assert out[0][1] == 0


@pytest.mark.parametrize("name", ["well33x31", "dense130"])
def test_the_forms_of_a_diagonal_M_give_the_same_bits(name):
    A, b, d, _ = problem(name, "jacobi", 1e-6, 0)
    forms = ["jacobi", sp.diags(1.0 / diagonal_of(A)), sp.diags(d).tocsr(), sp.diags(d).tocoo(), np.diag(d)]
    explicit_zero = sp.csr_matrix(sp.diags(d))
    explicit_zero = (explicit_zero + sp.csr_matrix(([0.0], ([0], [1])), shape=explicit_zero.shape)).tocsr()  # a stored off-diagonal zero
    out = [cg(A, b, rtol=1e-6, M=M, _backend=NumpyCgBackend(A)) for M in forms + [explicit_zero]]
    for x, info in out:
        assert info == 0 and np.array_equal(x, out[0][0])
    plain, _ = cg(A, b, rtol=1e-6, _backend=NumpyCgBackend(A))
    assert not np.array_equal(plain, out[0][0])


# ---------------------------------------------------------------- start vectors and trivial sizes
@pytest.mark.parametrize("pre", ["plain", "jacobi"])
def test_a_nonzero_x0(pre):
    A, b, d, _ = problem("lap24x20", pre, 1e-6, 0)
    x0 = np.random.default_rng(77).standard_normal(A.shape[0])
    xs, info_s = sla.cg(A, b, x0=x0.copy(), rtol=1e-8, M=_M(d))
    run = {}
    x, info = cg(A, b, x0, rtol=1e-8, M=_M(d), info=run, _backend=NumpyCgBackend(A))
    assert info == info_s == 0
    assert np.linalg.norm(x - xs) <= 1e-12 * np.linalg.norm(xs)
    assert run["products"] == run["iterations"] + 1
    # an all-zero guess is no guess: the bits of the call without one, and no product for it
    run0 = {}
    xa, _ = cg(A, b, np.zeros(A.shape[0]), rtol=1e-8, M=_M(d), info=run0, _backend=NumpyCgBackend(A))
    xb, _ = cg(A, b, rtol=1e-8, M=_M(d), _backend=NumpyCgBackend(A))
    assert np.array_equal(xa, xb) and run0["products"] == run0["iterations"]


def test_zero_b_and_n_equal_one():
    A = matrix("dense130")
    run = {}
    x, info = cg(A, np.zeros(130), np.ones(130), M="jacobi", info=run)  # (no backend, no device: answered before either)
    assert info == 0 and np.array_equal(x, np.zeros(130)) and run["iterations"] == 0 and run["preconditioner"] == "diagonal"
    xs, info_s = sla.cg(A, np.zeros(130), x0=np.ones(130))
    assert info_s == 0 and np.array_equal(xs, x)
    calls, cb = _count()
    x, info = cg(np.array([[4.0]]), np.array([2.0]), callback=cb)
    assert info == 0 and np.array_equal(x, [0.5]) and len(calls) == 1
    x, info = cg(sp.csr_matrix(np.array([[8.0]])), np.array([[2.0]]), M="jacobi")
    assert info == 0 and np.array_equal(x, [0.25])


# ---------------------------------------------------------------- maxiter
def test_the_deviation_at_maxiter_and_maxiter_exhausted():
    A, b, d, adm = problem("lap24x20", "jacobi", 1e-6, 0)
    ref = adm["runs"]["dot"]
    its = ref["iterations"]
    # the last permitted iteration ends with |r| < atol_eff: SciPy would test at the head of the next one only and reports maxiter
    xs, info_s = sla.cg(A, b, rtol=1e-6, maxiter=its, M=_M(d))
    run = {}
    x, info = cg(A, b, rtol=1e-6, maxiter=its, M=_M(d), info=run, _backend=NumpyCgBackend(A))
    assert info_s == its and info == 0 and run["exit"] == "converged" and run["iterations"] == its
    assert np.linalg.norm(x - xs) <= X_MARGIN * adm["x_spread"]
    assert loop(A, b, adm["atol_eff"], its, "dot", d=d)["code"] == its
    # maxiter exhausted
    for every in (1, 4, 8):
        run = {}
        x5, info5 = cg(A, b, rtol=1e-6, maxiter=5, M=_M(d), check_every=every, info=run, _backend=NumpyCgBackend(A))
        xs5, info_s5 = sla.cg(A, b, rtol=1e-6, maxiter=5, M=_M(d))
        assert info5 == info_s5 == 5 and run["exit"] == "maxiter" and run["iterations"] == 5 and run["code"] == 5
        assert len(run["history"]) == 6 and np.linalg.norm(x5 - xs5) <= 1e-13 * np.linalg.norm(xs5)
    x0, info0 = cg(A, b, rtol=1e-6, maxiter=0, _backend=NumpyCgBackend(A))
    assert info0 == 0 and not np.any(x0)


# ---------------------------------------------------------------- breakdown and indefiniteness
def _state(n, seed=5):
    rng = np.random.default_rng(seed)
    return {name: rng.standard_normal(n) for name in ("x", "r", "p")}


@pytest.mark.parametrize("what", ["pq", "rho"])
def test_breakdowns_through_set_state(what):
    """-1: ``p`` orthogonal to ``A p`` (the skew matrix; integer entries, so ``p . A p`` is exactly zero in any order), or ``rho = nan``;
    ``x`` stays as it was"""
    A = skew64()
    s = _state(64)
    s["p"] = np.random.default_rng(6).integers(-4, 5, 64).astype(np.float64)
    backend = NumpyCgBackend(A)
    backend.set_state(3, s["x"], s["r"], s["p"], None, [float("nan") if what == "rho" else 1.3])
    run = {}
    x, info = solve(backend, None, None, 1e-9, 50, 8, info=run, begun=True)
    assert info == -1 and run["code"] == -1 and run["exit"] == "breakdown" and run["iterations"] == 0 and np.array_equal(x, s["x"])
    assert run["products"] == (1 if what == "pq" else 0)
    # the same state with nothing wrong runs on
    backend = NumpyCgBackend(matrix("dense130"))
    s = _state(130)
    backend.set_state(3, s["x"], s["r"], s["p"], None, [1.3])
    st = backend.run(1, 1e-9)
    assert st["iterations"] == 4 and not st["done"] and st["alpha"] == 1.3 / st["pq"]


@pytest.mark.parametrize("b_last,at", [(5.0, 0), (0.1, 1)])
def test_indefinite_at_on_a_matrix_with_one_negative_eigenvalue(b_last, at):
    diag = np.ones(64)
    diag[-1] = -1.0
    A = sp.diags(diag).tocsr()
    b = np.full(64, 0.1)
    b[-1] = b_last
    ref = loop(A, b, 1e-6 * float(np.linalg.norm(b)), 640, "dot")
    assert ref["indefinite_at"] == at
    xs, info_s = sla.cg(A, b, rtol=1e-6)
    run = {}
    x, info = cg(A, b, rtol=1e-6, info=run, _backend=NumpyCgBackend(A))
    assert info == info_s == 0 and run["indefinite_at"] == at and run["iterations"] == ref["iterations"]  # (p . q <= 0 does not stop it)
    assert np.allclose(x, xs, rtol=1e-12, atol=0) and np.allclose(A @ x, b, rtol=0, atol=2e-6 * np.linalg.norm(b))


# ---------------------------------------------------------------- argument errors
def test_every_argument_error_is_raised_with_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(_capi, "Handle", no_device)
    A = matrix("sym401")
    n = A.shape[0]
    b = np.ones(n)
    good = np.full(n, 2.0)
    with pytest.raises(ValueError, match="square"):
        cg(sp.csr_matrix(np.ones((3, 4))), np.ones(3))
    with pytest.raises(NotImplementedError, match="cg: complex A"):
        cg(A.astype(np.complex128), b)
    with pytest.raises(NotImplementedError, match="complex b"):
        cg(A, b + 0j)
    with pytest.raises(NotImplementedError, match="complex x0"):
        cg(A, b, x0=b + 0j)
    with pytest.raises(NotImplementedError, match="complex M"):
        cg(A, b, M=sp.diags(good + 0j))
    with pytest.raises(NotImplementedError, match="complex M"):
        cg(A, b, M=np.diag(good + 0j))
    with pytest.raises(NotImplementedError, match="cg: LinearOperator"):
        cg(sla.aslinearoperator(A), b)
    with pytest.raises(ValueError, match="incompatible"):
        cg(A, np.ones(n + 1))
    with pytest.raises(ValueError, match="incompatible"):
        cg(A, b, x0=np.ones(n - 1))
    with pytest.raises(ValueError, match="maxiter"):
        cg(A, b, maxiter=-1)
    with pytest.raises(ValueError, match="check_every"):
        cg(A, b, check_every=0)
    with pytest.raises(ValueError, match="non-negative"):
        cg(A, b, rtol=-1e-3)
    # M: only diagonal preconditioners are built
    off = sp.diags(good).tolil()
    off[3, 7] = 1e-300
    for M in (off.tocsr(), off.toarray(), A, sla.aslinearoperator(sp.diags(good)), (lambda r: r)):
        with pytest.raises(NotImplementedError, match="only diagonal preconditioners are built"):
            cg(A, b, M=M)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        dvec = good.copy()
        dvec[5] = bad
        for M in (sp.diags(dvec), np.diag(dvec)):
            with pytest.raises(ValueError, match="finite and strictly positive"):
                cg(A, b, M=M)
    for M in (sp.diags(np.ones(n + 1)), np.eye(n - 1), np.ones(n)):
        with pytest.raises(ValueError, match="incompatible"):
            cg(A, b, M=M)
    with pytest.raises(ValueError, match="unknown preconditioner"):
        cg(A, b, M="ilu")
    stencil = StencilOperator((4, 4, 4), 7, potential=np.full(64, 7.0))
    with pytest.raises(NotImplementedError, match="no host diagonal"):
        cg(stencil, np.ones(64), M="jacobi")
    zero_diagonal = sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))
    with pytest.raises(ValueError, match="finite and strictly positive"):
        cg(zero_diagonal, np.ones(2), M="jacobi")
    n_, b_, x0_, maxiter_, d_ = check_cg_args(A, b.reshape(n, 1), None, "jacobi", None, 8, 1e-5, 0.0)
    assert (n_, b_.shape, x0_, maxiter_) == (n, (n,), None, 10 * n) and np.array_equal(d_, 1.0 / A.diagonal())
    with pytest.raises(AssertionError, match="a device was asked for"):  # (the patch is in place: a good call does reach for one)
        cg(A, b)


# ---------------------------------------------------------------- signature and export
def test_signature_is_scipys_plus_the_projects_extras():
    ours = inspect.signature(cg).parameters
    theirs = inspect.signature(sla.cg).parameters
    for name, p in theirs.items():
        assert name in ours and ours[name].default == p.default and ours[name].kind == p.kind, name
    assert [k for k in ours if k not in theirs] == ["check_every", "device_id", "handle", "info", "_backend"]
    assert "cg" in lanczos_amd.__all__ and lanczos_amd.cg is cg
