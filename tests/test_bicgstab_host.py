"""``bicgstab`` on the host: the loop of lanczos_amd/bicgstab.py on its NumPy backend (a restatement of the device calls) against
SciPy's ``bicgstab`` and the longdouble loop of tests/bicgstab_reference.py, on cases admitted by that file's rule; the chunking, the
exits, the two deviations from SciPy and every argument error.  No GPU."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla
from bicgstab_reference import MATRICES, admission, loop, skew64

import lanczos_amd
from lanczos_amd import bicgstab
from lanczos_amd.bicgstab import NumpyBicgstabBackend, check_bicgstab_args, solve

# (matrix, rtol) -> the two seeds used, each admitted (test_every_case_is_admitted); found among seeds 0 .. 11
SEEDS = {
    ("convdiff24x20", 1e-6): (0, 3), ("convdiff24x20", 1e-10): (0, 10),
    ("convdiff33x31", 1e-6): (9, 11), ("convdiff33x31", 1e-10): (0, 9),
    ("random401", 1e-6): (0, 5), ("random401", 1e-10): (0, 11),
    ("dense130", 1e-6): (1, 10), ("dense130", 1e-10): (0, 2),
}
CASES = [(name, rtol, seed) for (name, rtol), seeds in SEEDS.items() for seed in seeds]
X_MARGIN = 16.0  # a further summation order may sit this many times the admission runs' own spread in x away


@functools.lru_cache(maxsize=None)
def matrix(name):
    return MATRICES[name]()


@functools.lru_cache(maxsize=None)
def problem(name, rtol, seed):
    """``(A, b, admission record)``, computed once and shared (tests/test_gpu_bicgstab.py reads it too); nothing changes it"""
    A = matrix(name)
    b = np.random.default_rng(seed).standard_normal(A.shape[0])
    b.setflags(write=False)
    return A, b, admission(A, b, rtol)


def _count():
    calls = []
    return calls, (lambda xk: calls.append(np.array(xk)))


@pytest.mark.parametrize("name,rtol,seed", CASES)
def test_every_case_is_admitted(name, rtol, seed):
    adm = problem(name, rtol, seed)[2]
    print(f"{name} rtol {rtol:g} seed {seed}: exit {adm['runs']['dot']['exit']}, margin {adm['margin']:.3f}, spread {adm['spread']:.2e}")
    assert adm["same_stop"] and adm["admitted"]


def test_both_exits_are_among_the_cases():
    kinds = {problem(*case)[2]["runs"]["dot"]["exit"] for case in CASES}
    assert kinds == {"half", "full"}


@pytest.mark.parametrize("name,rtol,seed", CASES)
def test_numpy_backend_against_scipy_and_longdouble(name, rtol, seed):
    A, b, adm = problem(name, rtol, seed)
    calls_s, cb_s = _count()
    xs, info_s = sla.bicgstab(A, b, rtol=rtol, callback=cb_s)
    calls, cb = _count()
    run = {}
    x, info = bicgstab(A, b, rtol=rtol, callback=cb, info=run, _backend=NumpyBicgstabBackend(A))
    assert info == info_s == 0 and len(calls) == len(calls_s)
    ref = adm["runs"]["dot"]
    assert (run["exit"], run["iterations"], run["code"]) == (ref["exit"], ref["iterations"], 0)
    assert len(calls) == ref["callbacks"] == run["iterations"] - (1 if run["exit"] == "half" else 0)
    assert run["products"] == 2 * run["iterations"] - (1 if run["exit"] == "half" else 0)
    dist = float(np.linalg.norm(x - xs))
    print(f"{name} rtol {rtol:g} seed {seed}: |x - x_scipy| {dist:.2e}, spread in x {adm['x_spread']:.2e}, ratio {dist / adm['x_spread']:.2f}")
    assert dist <= X_MARGIN * adm["x_spread"]
    assert run["residual_norm"] < run["atol_effective"] == adm["atol_eff"]
    assert run["history"].shape == (run["iterations"], 2) and run["history"][-1, 1] == run["residual_norm"]
    # the recurrence's tested norms are the reference run's, and the true residual meets the bar
    tested = [t[2] for t in ref["tests"] if t[0] == "s"]
    assert np.array_equal(run["history"][:, 0], tested)
    true = np.asarray(A @ x).ravel() - b
    assert np.linalg.norm(true) <= 2.0 * adm["atol_eff"]
    if calls:
        full = x if run["exit"] == "full" else None
        assert full is None or np.array_equal(calls[-1], full)


@pytest.mark.parametrize("name,rtol,seed", [("convdiff24x20", 1e-10, 0), ("random401", 1e-6, 0), ("dense130", 1e-10, 2)])
def test_check_every_does_not_change_a_bit(name, rtol, seed):
    A, b, _ = problem(name, rtol, seed)
    out = []
    for every in (1, 8, 256):
        run = {}
        x, info = bicgstab(A, b, rtol=rtol, check_every=every, info=run, _backend=NumpyBicgstabBackend(A))
        out.append((x, info, run["iterations"], run["exit"], run["history"]))
    for x, info, its, kind, hist in out[1:]:
        assert np.array_equal(x, out[0][0]) and (info, its, kind) == out[0][1:4] and np.array_equal(hist, out[0][4])
    assert out[0][1] == 0


def test_a_nonzero_x0():
    A, b, _ = problem("convdiff24x20", 1e-6, 0)
    x0 = np.random.default_rng(77).standard_normal(A.shape[0])
    xs, info_s = sla.bicgstab(A, b, x0=x0.copy(), rtol=1e-8)
    run = {}
    x, info = bicgstab(A, b, x0, rtol=1e-8, info=run, _backend=NumpyBicgstabBackend(A))
    assert info == info_s == 0
    assert np.linalg.norm(x - xs) <= 1e-12 * np.linalg.norm(xs)
    assert run["products"] == 2 * run["iterations"] - (1 if run["exit"] == "half" else 0) + 1
    # an all-zero guess is no guess: the bits of the call without one
    xa, _ = bicgstab(A, b, np.zeros(A.shape[0]), rtol=1e-8, _backend=NumpyBicgstabBackend(A))
    xb, _ = bicgstab(A, b, rtol=1e-8, _backend=NumpyBicgstabBackend(A))
    assert np.array_equal(xa, xb)


def test_zero_b_and_n_equal_one():
    A = matrix("dense130")
    run = {}
    x, info = bicgstab(A, np.zeros(130), np.ones(130), info=run)  # (no backend, no device: answered before either)
    assert info == 0 and np.array_equal(x, np.zeros(130)) and run["iterations"] == 0
    xs, info_s = sla.bicgstab(A, np.zeros(130), x0=np.ones(130))
    assert info_s == 0 and np.array_equal(xs, x)
    calls, cb = _count()
    x, info = bicgstab(np.array([[4.0]]), np.array([2.0]), callback=cb)
    assert info == 0 and np.array_equal(x, [0.5]) and len(calls) == 1
    x, info = bicgstab(sp.csr_matrix(np.array([[-8.0]])), np.array([[2.0]]))
    assert info == 0 and np.array_equal(x, [-0.25])


def test_the_deviation_at_maxiter_and_maxiter_exhausted():
    A, b, adm = problem("convdiff24x20", 1e-6, 3)
    ref = adm["runs"]["dot"]
    assert ref["exit"] == "full"
    its = ref["iterations"]
    # the last permitted iteration ends with |r| < atol_eff: SciPy would test at the head of the next one only and reports maxiter
    xs, info_s = sla.bicgstab(A, b, rtol=1e-6, maxiter=its)
    run = {}
    x, info = bicgstab(A, b, rtol=1e-6, maxiter=its, info=run, _backend=NumpyBicgstabBackend(A))
    assert info_s == its and info == 0 and run["exit"] == "full" and run["iterations"] == its
    assert np.array_equal(x, xs)
    assert loop(A, b, adm["atol_eff"], its, "dot")["code"] == its
    # maxiter exhausted
    for every in (1, 4, 8):
        run = {}
        x5, info5 = bicgstab(A, b, rtol=1e-6, maxiter=5, check_every=every, info=run, _backend=NumpyBicgstabBackend(A))
        xs5, info_s5 = sla.bicgstab(A, b, rtol=1e-6, maxiter=5)
        assert info5 == info_s5 == 5 and run["exit"] == "maxiter" and run["iterations"] == 5 and run["code"] == 5
        assert np.array_equal(x5, xs5)
    x0, info0 = bicgstab(A, b, rtol=1e-6, maxiter=0, _backend=NumpyBicgstabBackend(A))
    assert info0 == 0 and not np.any(x0)


def test_breakdown_of_the_skew_matrix():
    A = skew64()
    b = np.random.default_rng(0).standard_normal(64)
    xs, info_s = sla.bicgstab(A, b)
    calls, cb = _count()
    run = {}
    x, info = bicgstab(A, b, info=run, callback=cb, _backend=NumpyBicgstabBackend(A))
    assert info == info_s == -11 and not np.any(x) and not np.any(xs) and not calls
    assert run["exit"] == "breakdown" and run["iterations"] == 0 and run["products"] == 1
    x0 = np.random.default_rng(1).standard_normal(64)
    x, info = bicgstab(A, b, x0, _backend=NumpyBicgstabBackend(A))
    assert info == -11 and np.array_equal(x, x0)


def _state(n, k, seed=5):
    rng = np.random.default_rng(seed)
    return {name: rng.standard_normal(n) for name in ("x", "r", "rtilde", "p", "v")}


@pytest.mark.parametrize("what", ["rho", "omega"])
def test_breakdowns_through_set_state(what):
    """-10 (``rtilde`` orthogonal to ``r``) and the ``omega`` form of -11, from an uploaded state; ``x`` stays as it was"""
    A, b, _ = problem("random401", 1e-6, 0)
    n = A.shape[0]
    s = _state(n, 3)
    scalars = [1.3, 0.7, -0.45]
    if what == "rho":
        s["r"][1::2] = 0.0
        s["rtilde"][0::2] = 0.0
    else:
        scalars[2] = 1e-40
    backend = NumpyBicgstabBackend(A)
    backend.set_state(3, s["x"], s["r"], s["rtilde"], s["p"], s["v"], scalars)
    run = {}
    x, info = solve(backend, b, None, 1e-9, 50, 8, info=run, begun=True)
    assert info == (-10 if what == "rho" else -11)
    assert run["exit"] == "breakdown" and run["iterations"] == 0 and run["products"] == 0 and np.array_equal(x, s["x"])
    # the same state with nothing wrong runs on
    backend.set_state(3, s["x"], _state(n, 3)["r"], _state(n, 3)["rtilde"], s["p"], s["v"], [1.3, 0.7, -0.45])
    st = backend.run(1, 1e-9)
    assert st["iterations"] == 4 and not st["done"]


def test_every_argument_error_is_raised_with_no_device():
    A = matrix("random401")
    n = A.shape[0]
    b = np.ones(n)
    with pytest.raises(NotImplementedError, match="preconditioning"):
        bicgstab(A, b, M=sp.identity(n))
    with pytest.raises(NotImplementedError, match="complex A"):
        bicgstab(A.astype(np.complex128), b)
    with pytest.raises(NotImplementedError, match="complex b"):
        bicgstab(A, b + 0j)
    with pytest.raises(NotImplementedError, match="complex x0"):
        bicgstab(A, b, x0=b + 0j)
    with pytest.raises(NotImplementedError, match="LinearOperator"):
        bicgstab(sla.aslinearoperator(A), b)
    with pytest.raises(ValueError, match="square"):
        bicgstab(sp.csr_matrix(np.ones((3, 4))), np.ones(3))
    with pytest.raises(ValueError, match="square"):
        bicgstab(np.ones(5), np.ones(5))
    with pytest.raises(ValueError, match="incompatible"):
        bicgstab(A, np.ones(n + 1))
    with pytest.raises(ValueError, match="incompatible"):
        bicgstab(A, b, x0=np.ones(n - 1))
    with pytest.raises(ValueError, match="maxiter"):
        bicgstab(A, b, maxiter=-1)
    with pytest.raises(ValueError, match="check_every"):
        bicgstab(A, b, check_every=0)
    with pytest.raises(ValueError, match="non-negative"):
        bicgstab(A, b, rtol=-1e-3)
    with pytest.raises(ValueError, match="non-negative"):
        bicgstab(A, b, atol=float("nan"))
    n_, b_, x0_, maxiter_ = check_bicgstab_args(A, b.reshape(n, 1), None, None, None, 8, 1e-5, 0.0)
    assert (n_, b_.shape, x0_, maxiter_) == (n, (n,), None, 10 * n)


def test_signature_is_scipys_plus_the_projects_extras():
    import inspect

    ours = inspect.signature(bicgstab).parameters
    theirs = inspect.signature(sla.bicgstab).parameters
    for name, p in theirs.items():
        assert name in ours and ours[name].default == p.default and ours[name].kind == p.kind, name
    assert [k for k in ours if k not in theirs] == ["check_every", "device_id", "handle", "info", "_backend"]
    assert "bicgstab" in lanczos_amd.__all__ and lanczos_amd.bicgstab is bicgstab
