"""``cg`` on the device: one iteration of ``lz_cg_run`` from an uploaded state against longdouble with forward-error bounds
(tests/cg_reference.py) on every product form and at the block edges of the passes, with and without a diagonal preconditioner; the
chunking and the gate; the function end to end at the bars of tests/test_cg_host.py on every product plan; the breakdown exit and
``indefinite_at``; the status codes; and the life of a handle that serves ``eigsh``, ``cg`` and ``minres`` in turn."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from bicgstab_reference import skew64
from cg_reference import LD, Operator, admission, dot_bound, lap, norm_bound, one_iteration, random_state, worst
from minres_reference import named
from test_cg_host import CASES, X_MARGIN, problem, well_plain

from lanczos_amd import StencilOperator, _capi, cg, eigsh, minres
from lanczos_amd.cg import NumpyCgBackend
from lanczos_amd.eigsh import upload_matrix

pytestmark = pytest.mark.gpu

VECTORS = ("x", "r", "p", "q", "d")
ERR_ARG, ERR_STATE = -1, -4  # LZ_ERR_ARG, LZ_ERR_STATE (include/lanczos_hip.h)


def _handle(A):
    h = _capi.Handle(0)
    upload_matrix(h, A)
    return h


@pytest.fixture(scope="module")
def shared():
    h = _capi.Handle(0)
    yield h
    h.close()


def status_of(call, *args):
    with pytest.raises(_capi.LanczosHipError) as e:
        call(*args)
    return e.value.status


@functools.lru_cache(maxsize=None)
def step_matrix(name):
    """tests/test_gpu_minres.py's: symmetric, not definite - one iteration from a random state needs neither"""
    if name in ("ragged1000", "band70001"):
        return named(name)
    kind, n = name.split("_")
    n = int(n)
    rng = np.random.default_rng(n)
    if kind == "dense":
        G = rng.standard_normal((n, n))
        return np.ascontiguousarray(G + G.T)
    if n <= 5:
        G = rng.standard_normal((n, n))
        A = sp.csr_matrix(G + G.T)
    else:  # about seven entries per row, ragged
        S = sp.random(n, n, density=3.0 / n, random_state=rng, data_rvs=rng.standard_normal)
        A = (S + S.T + sp.diags(rng.standard_normal(n))).tocsr()
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def step_operator(name):
    """the longdouble operator of ``step_matrix(name)``; a sparse matrix with an empty row goes through its dense copy with the rows'
    true lengths (an empty row's product is exactly zero)"""
    A = step_matrix(name)
    if sp.issparse(A) and np.diff(A.indptr).min() < 1:
        op = Operator(A.toarray())
        op.rowlen = np.diff(A.indptr).astype(np.float64)
        return op
    return Operator(A)


def _vectors(h, raw=False):
    return {name: h.cg_get(name, raw=raw) for name in VECTORS}


# ---------------------------------------------------------------- a. one iteration against longdouble
STEP_CASES = ["csr_2", "csr_5", "csr_255", "csr_256", "csr_257", "ragged1000", "band70001", "dense_64", "dense_513"]


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "diagonal"])
@pytest.mark.parametrize("name", STEP_CASES)
def test_one_iteration_against_longdouble(name, pre):
    A = step_matrix(name)
    n = A.shape[0]
    s = random_state(n, n + 11, pre)
    ref, bound = one_iteration(A, s, step_operator(name))
    h = _handle(A)
    h.cg_set_state(3, s["x"], s["r"], s["p"], s["d"], [s["rho"]])
    assert h.cg_info() == {"launches_per_iteration": 5, "preconditioned": pre, "live": True}
    st = h.cg_run(1, 0.0)
    got = _vectors(h)
    raw = _vectors(h, raw=True)
    assert st["iterations"] == 4 and not st["done"] and st["exit"] is None and st["code"] == 0
    # with the device's own scalars and its own q the vectors are exact: the element-wise updates round like NumPy
    alpha, beta = st["alpha"], st["beta"]
    assert st["rho_prev"] == s["rho"] and alpha == s["rho"] / st["pq"] and beta == st["rho"] / s["rho"]
    assert st["indefinite_at"] == (3 if st["pq"] <= 0.0 else None)
    r = s["r"] - alpha * got["q"]
    z = r if not pre else s["d"] * r
    assert np.array_equal(got["r"], r) and np.array_equal(got["x"], s["x"] + alpha * s["p"]) and np.array_equal(got["p"], z + beta * s["p"])
    assert np.array_equal(got["d"], s["d"] if pre else np.zeros(n))
    # against longdouble, every error within its forward bound
    err = lambda a, b: np.abs(np.asarray(a - b, dtype=np.float64))  # noqa: E731
    figures = {key: worst(err(got[key], ref[key]), bound[key]) for key in ("q", "r", "p", "x")}
    figures.update({key: abs(float(st[key] - ref[key])) / bound[key] for key in ("pq", "alpha", "rnorm", "rho", "beta")})
    r0 = s["r"].astype(LD)
    r0norm = np.sqrt(np.dot(r0, r0))
    hist = h.cg_history(5)
    figures["rnorm0"] = abs(float(hist[3] - r0norm)) / norm_bound(dot_bound(s["r"], s["r"]), r0norm)
    print(f"{name:12s} {'diagonal' if pre else 'plain':8s} error / bound: " + "  ".join(f"{key} {val:.2e}" for key, val in figures.items()))
    for key, val in figures.items():
        assert val <= 1.0, key
    assert hist[4] == st["rnorm"] and not np.any(hist[:3])
    for key in VECTORS:
        assert np.all(np.isfinite(raw[key])) and np.all(raw[key][n:] == 0.0), key
        assert np.array_equal(raw[key][:n], got[key])
    # the same call from the same state: the same bits
    h.cg_set_state(3, s["x"], s["r"], s["p"], s["d"], [s["rho"]])
    assert h.cg_run(1, 0.0) == st
    again = _vectors(h)
    for key in VECTORS:
        assert np.array_equal(again[key], got[key]), key
    h.close()


# ---------------------------------------------------------------- b. chunking
@functools.lru_cache(maxsize=None)
def stencil():
    """a 7-point stencil with a potential, assembled on the device: the coded-stencil product"""
    pot = np.random.default_rng(8).uniform(6.5, 7.5, 12 * 10 * 8)
    return StencilOperator((12, 10, 8), 7, potential=pot)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "diagonal"])
@pytest.mark.parametrize("name", ["lap33x31", "stencil"])
def test_six_single_iterations_equal_one_chunk_of_six(name, pre):
    A = lap(33, 31) if name == "lap33x31" else stencil()
    n = A.shape[0]
    b = np.random.default_rng(2).standard_normal(n)
    d = np.random.default_rng(3).uniform(0.5, 2.0, n) if pre else None
    h = _handle(A)
    assert h.spmv_coding()[0] != "none"  # the row-class coded kernel
    h.cg_begin(b, None, d)
    for _ in range(6):
        st1 = h.cg_run(1, 0.0)
    single = _vectors(h)
    hist1 = h.cg_history(7)
    h.cg_begin(b, None, d)
    st6 = h.cg_run(6, 0.0)
    chunk = _vectors(h)
    assert st1 == st6 and st6["iterations"] == 6 and not st6["done"]
    assert np.array_equal(hist1, h.cg_history(7)) and np.all(hist1 > 0.0)
    for key in VECTORS:
        assert np.array_equal(single[key], chunk[key]), key
    # and the sixth iterate is the NumPy backend's to rounding
    ref = NumpyCgBackend(A)
    ref.begin(b, None, d)
    ref.run(6, 0.0)
    assert np.linalg.norm(chunk["x"] - ref.x) <= 1e-12 * np.linalg.norm(ref.x)
    assert np.linalg.norm(chunk["p"] - ref.p) <= 1e-12 * np.linalg.norm(ref.p)
    h.close()


# ---------------------------------------------------------------- c. the gate
@pytest.mark.parametrize("name,pre,rtol,seed", [("lap24x20", "jacobi", 1e-6, 0), ("sym401", "plain", 1e-10, 0), ("well33x31", "jacobi", 1e-10, 1)])
def test_a_chunk_past_the_exit_changes_nothing(shared, name, pre, rtol, seed):
    A, b, d, adm = problem(name, pre, rtol, seed)
    M = None if d is None else sp.diags(d)
    its = adm["runs"]["dot"]["iterations"]
    one, big, host = {}, {}, {}
    x1, c1 = cg(A, b, rtol=rtol, M=M, check_every=1, handle=shared, info=one)
    x256, c256 = cg(A, b, rtol=rtol, M=M, check_every=256, handle=shared, info=big)
    xh, ch = cg(A, b, rtol=rtol, M=M, info=host, _backend=NumpyCgBackend(A))
    assert c1 == c256 == ch == 0 and one["exit"] == big["exit"] == "converged"
    assert one["iterations"] == big["iterations"] == host["iterations"] == its < 256 and big["chunks"] == 1 and one["chunks"] == its
    assert np.array_equal(x1, x256) and np.array_equal(one["history"], big["history"]) and len(big["history"]) == its + 1
    assert one["residual_norm"] == big["residual_norm"] < one["atol_effective"]
    # x of the exit iteration has had its update: it is the NumPy backend's to the host tests' bar
    assert np.linalg.norm(x256 - xh) <= X_MARGIN * adm["x_spread"]
    # what the exit leaves on the device, and that the iterations enqueued behind it changed no vector and no history entry
    assert np.array_equal(shared.cg_get("x"), x256)
    behind = {key: shared.cg_get(key) for key in ("x", "r", "p")}
    raw = shared.cg_history(257)
    assert np.array_equal(raw[: its + 1], big["history"]) and np.all(raw[its + 1:] == 0.0)
    shared.cg_begin(b, None, d)
    st = shared.cg_run(its, adm["atol_eff"])  # exactly the iterations that ran: nothing is enqueued behind the exit
    assert st["done"] and st["exit"] == "converged" and st["head"] and st["iterations"] == its
    for key in ("x", "r", "p"):
        assert np.array_equal(shared.cg_get(key), behind[key]), key
    assert shared.cg_run(256, adm["atol_eff"]) == st  # a state that is done stays as it is
    rvec = shared.cg_get("r")
    assert np.sqrt(np.dot(rvec, rvec)) == pytest.approx(big["residual_norm"], rel=1e-12)
    true = b - np.asarray(A @ x256).ravel()
    assert np.linalg.norm(true - rvec) <= 1e-10 * np.linalg.norm(b)  # (r = b - A x to the recurrence's drift)


# ---------------------------------------------------------------- d. end to end at the host tests' bars on every product plan
def _end_to_end(h, A, b, d, rtol, adm, host_matrix, label):
    host, dev = {}, {}
    M = None if d is None else sp.diags(d)
    xh, ch = cg(host_matrix, b, rtol=rtol, M=M, info=host, _backend=NumpyCgBackend(host_matrix))
    x, code = cg(A, b, rtol=rtol, M=M, handle=h, info=dev)
    assert code == ch == 0
    assert dev["iterations"] == host["iterations"] == adm["runs"]["dot"]["iterations"] and dev["exit"] == "converged"
    assert dev["products"] == host["products"] and dev["launches_per_iteration"] == 5
    assert dev["preconditioner"] == (None if d is None else "diagonal") and dev["indefinite_at"] is None
    true = np.asarray(Operator(host_matrix).matvec(x) - b.astype(LD), dtype=np.float64)
    dist = float(np.linalg.norm(x - xh))
    print(f"{label} rtol {rtol:g}: {dev['iterations']} iterations, plan {h.spmv_plan()}, coding {h.spmv_coding()[0]}, |x - x_host| {dist:.2e}, "
          f"spread in x {adm['x_spread']:.2e}, ratio {dist / adm['x_spread']:.2f}, true residual / atol_eff "
          f"{np.linalg.norm(true) / adm['atol_eff']:.3f}")
    assert np.linalg.norm(true) <= 2.0 * adm["atol_eff"]
    assert dist <= X_MARGIN * adm["x_spread"]


@pytest.mark.parametrize("form", ["csr", "dense"])
@pytest.mark.parametrize("name,pre,rtol,seed", CASES)
def test_end_to_end_on_the_admitted_cases(shared, name, pre, rtol, seed, form):
    A, b, d, adm = problem(name, pre, rtol, seed)
    if form == "csr":
        M = A if sp.issparse(A) else sp.csr_matrix(A)
    else:
        M = np.ascontiguousarray(A.toarray()) if sp.issparse(A) else A
    _end_to_end(shared, M, b, d, rtol, adm, M, f"{name} {pre} {form} seed {seed}")
    if form == "dense":
        assert shared.spmv_plan() == "dense"
    elif name.startswith("lap"):
        assert shared.spmv_coding()[0] == "offsets+values"  # constant coefficients: the row-class coded kernel
    elif name == "sym401":
        assert shared.spmv_coding()[0] == "none" and shared.spmv_plan() != "two-phase"  # ragged rows: a CSR kernel


@pytest.mark.parametrize("name,pre,rtol,seed", [("lap33x31", "plain", 1e-10, 1), ("well33x31", "jacobi", 1e-6, 0)])
def test_end_to_end_on_the_ell_product(name, pre, rtol, seed):
    """tuning knob 17 = 2 keeps the uncoded ELL copy of a matrix with five entries in every row and makes it the product"""
    A, b, d, adm = problem(name, pre, rtol, seed)
    h = _capi.Handle(0)
    h.set_tuning(17, 2)
    _end_to_end(h, A, b, d, rtol, adm, A, f"{name} {pre} ell seed {seed}")
    assert h.spmv_coding()[0] == "none"
    h.close()


@functools.lru_cache(maxsize=None)
def stencil_problem(rtol, pre):
    """``(S, b, d, admission record)`` of the first of the seeds 0 .. 5 that tests/cg_reference.py's rule admits: the matrix is
    assembled on the device, so its admitted seeds cannot be listed ahead of a run; the choice reads the reference runs alone"""
    S = stencil().to_scipy().tocsr()
    d = 1.0 / S.diagonal() if pre == "diagonal" else None
    for seed in range(6):
        b = np.random.default_rng(seed).standard_normal(S.shape[0])
        adm = admission(S, b, rtol, d)
        if adm["admitted"]:
            b.setflags(write=False)
            return S, b, d, adm
    raise AssertionError("no seed among 0 .. 5 is admitted")


@pytest.mark.parametrize("pre", ["plain", "diagonal"])
@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
def test_end_to_end_on_the_coded_stencil(shared, rtol, pre):
    S, b, d, adm = stencil_problem(rtol, pre)
    _end_to_end(shared, stencil(), b, d, rtol, adm, S, f"stencil {pre}")
    assert shared.spmv_coding()[0] != "none"


@functools.lru_cache(maxsize=None)
def scattered(n):
    """two normal entries in random columns of every row, symmetrised, plus ``diag(3 rowabs + 1)``: positive definite, ragged and
    without column locality - past 2^20 columns the product is the column-blocked two-phase one"""
    rng = np.random.default_rng(3)
    rows = np.repeat(np.arange(n), 2)
    cols = rng.integers(0, n, size=2 * n)
    S = sp.csr_matrix((rng.standard_normal(2 * n), (rows, cols)), shape=(n, n))
    T = (S + S.T).tocsr()
    A = (T + sp.diags(3.0 * np.asarray(abs(T).sum(axis=1)).ravel() + 1.0)).tocsr()
    A.sort_indices()
    return A


def test_end_to_end_on_the_column_blocked_two_phase_product():
    A = scattered(2**20 + 513)
    b = np.random.default_rng(0).standard_normal(A.shape[0])
    d = 1.0 / A.diagonal()  # (Jacobi brings the condition number to 2: about ten iterations, which keeps the reference runs short)
    adm = admission(A, b, 1e-6, d)
    assert adm["admitted"]
    h = _capi.Handle(0)
    _end_to_end(h, A, b, d, 1e-6, adm, A, "scattered jacobi")
    assert h.spmv_plan() == "two-phase"
    h.close()


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
def test_the_well_needs_its_preconditioner_on_the_device(shared, rtol):
    """``well33x31`` plain is admitted for no seed: held to the code, the true residual and four times its Jacobi run's iterations"""
    A, b, atol_eff, _ = well_plain(rtol, 0)
    run, jac = {}, {}
    x, code = cg(A, b, rtol=rtol, handle=shared, info=run)
    xj, cj = cg(A, b, rtol=rtol, M="jacobi", handle=shared, info=jac)
    true = np.linalg.norm(np.asarray(A @ x).ravel() - b)
    print(f"well33x31 rtol {rtol:g}: plain {run['iterations']} iterations, jacobi {jac['iterations']}, true residual / atol_eff {true / atol_eff:.3f}")
    assert code == cj == 0 and run["code"] == 0 and true <= 2.0 * atol_eff
    assert jac["iterations"] == problem("well33x31", "jacobi", rtol, 0)[3]["runs"]["dot"]["iterations"]
    assert run["iterations"] >= 4 * jac["iterations"]


def test_x0_callback_and_identical_bits(shared):
    A, b, d, adm = problem("lap24x20", "jacobi", 1e-10, 0)
    n = A.shape[0]
    x0 = np.random.default_rng(77).standard_normal(n)
    host, dev = {}, {}
    xh, ch = cg(A, b, x0, rtol=1e-8, M="jacobi", info=host, _backend=NumpyCgBackend(A))
    x, code = cg(A, b, x0, rtol=1e-8, M="jacobi", handle=shared, info=dev)
    assert code == ch == 0 and dev["products"] == dev["iterations"] + 1  # (one product more: A x0)
    assert np.linalg.norm(np.asarray(A @ x).ravel() - b) <= 2.0 * dev["atol_effective"]
    # the spectrum lies in [0.5, 8.5]: two solutions with residuals below 2 atol_eff lie within 8 atol_eff
    assert np.linalg.norm(x - xh) <= 8.0 * dev["atol_effective"]
    x2, _ = cg(A, b, x0, rtol=1e-8, M="jacobi", handle=shared)
    assert np.array_equal(x, x2)
    # callback: one iteration per synchronisation, the last xk is x
    calls, run = [], {}
    xc, code = cg(A, b, rtol=1e-10, M=sp.diags(d), handle=shared, info=run, callback=lambda xk: calls.append(xk.copy()))
    plain, code2 = cg(A, b, rtol=1e-10, M="jacobi", handle=shared)
    assert code == code2 == 0 and np.array_equal(xc, plain) and run["chunks"] == run["iterations"] == adm["runs"]["dot"]["iterations"]
    assert len(calls) == run["iterations"] and np.array_equal(calls[-1], xc)


# ---------------------------------------------------------------- e. breakdown and indefinite_at
@pytest.mark.parametrize("form", ["dense", "csr"])
@pytest.mark.parametrize("what", ["pq", "rho"])
def test_breakdowns_through_set_state_on_the_device(what, form):
    A = skew64() if form == "dense" else sp.csr_matrix(skew64())
    rng = np.random.default_rng(5)
    x, r = rng.standard_normal(64), rng.standard_normal(64)
    p = np.random.default_rng(6).integers(-4, 5, 64).astype(np.float64)  # (integers: p . A p is exactly zero in any order)
    h = _handle(A)
    h.cg_set_state(3, x, r, p, None, [float("nan") if what == "rho" else 1.3])
    st = h.cg_run(8, 1e-9)
    assert st["done"] and st["exit"] == "breakdown" and st["code"] == -1 and st["iterations"] == 3
    assert st["head"] == (what == "rho") and (what == "rho" or st["pq"] == 0.0)
    assert np.array_equal(h.cg_get("x"), x) and np.array_equal(h.cg_get("r"), r) and np.array_equal(h.cg_get("p"), p)
    again = h.cg_run(8, 1e-9)  # a state that is done stays as it is (the uploaded NaN is no number to compare)
    assert {k: v for k, v in again.items() if k != "rho"} == {k: v for k, v in st.items() if k != "rho"}
    assert np.isnan(again["rho"]) == np.isnan(st["rho"]) == (what == "rho")
    host = NumpyCgBackend(A)
    host.set_state(3, x, r, p, None, [float("nan") if what == "rho" else 1.3])
    hs = host.run(8, 1e-9)
    assert (hs["done"], hs["exit"], hs["code"], hs["iterations"], hs["head"]) == (True, "breakdown", -1, 3, what == "rho")
    h.close()


def test_indefinite_at_on_the_device(shared):
    diag = np.ones(64)
    diag[-1] = -1.0
    A = sp.diags(diag).tocsr()
    for b_last, at in ((5.0, 0), (0.1, 1)):
        b = np.full(64, 0.1)
        b[-1] = b_last
        host, dev = {}, {}
        xh, ch = cg(A, b, rtol=1e-6, info=host, _backend=NumpyCgBackend(A))
        x, code = cg(A, b, rtol=1e-6, handle=shared, info=dev)
        assert code == ch == 0 and dev["indefinite_at"] == host["indefinite_at"] == at and dev["iterations"] == host["iterations"]
        assert np.allclose(x, xh, rtol=1e-12, atol=0)
    # and through an uploaded state: p = e_n gives p . q = -1 at iteration 3; the solve goes on
    p = np.zeros(64)
    p[-1] = 1.0
    rng = np.random.default_rng(5)
    shared.cg_set_state(3, rng.standard_normal(64), rng.standard_normal(64), p, None, [1.3])
    st = shared.cg_run(1, 0.0)
    assert st["indefinite_at"] == 3 and st["pq"] == -1.0 and st["alpha"] == -1.3 and not st["done"] and st["iterations"] == 4


# ---------------------------------------------------------------- f. the status codes and the handle's life
def _begin_without_matrix(h):
    b = np.ones(8)
    h.check(h.lib.lz_cg_begin(h._h, _capi.dptr(b), None, None))


def _begin_with_null_b(h):
    h.check(h.lib.lz_cg_begin(h._h, None, None, None))


def test_state_errors():
    A, b, d, _ = problem("sym401", "plain", 1e-6, 0)
    h = _capi.Handle(0)
    assert status_of(_begin_without_matrix, h) == ERR_STATE
    upload_matrix(h, A)
    assert not h.cg_info()["live"]
    assert status_of(h.cg_run, 1, 0.0) == ERR_STATE
    assert status_of(h.cg_get, "x") == ERR_STATE
    assert status_of(h.cg_history, 1) == ERR_STATE
    assert status_of(_begin_with_null_b, h) == ERR_ARG
    h.cg_begin(b)
    assert h.cg_info()["live"]
    assert status_of(h.cg_step_time, 2) == ERR_STATE  # (nothing has run yet)
    assert h.cg_run(2, 0.0)["iterations"] == 2
    assert all(t > 0.0 for t in h.cg_step_time(2))  # (the probe's timer spends the state)
    assert status_of(h.cg_run, 1, 0.0) == ERR_STATE
    h.cg_begin(b)
    upload_matrix(h, A)  # a new matrix (lz_set_csr) drops the state
    assert not h.cg_info()["live"]
    assert status_of(h.cg_run, 1, 0.0) == ERR_STATE
    assert status_of(h.cg_get, "x") == ERR_STATE
    h.set_options(_capi.FLAG_REORTH_PARTIAL)
    assert status_of(h.cg_begin, b) == ERR_STATE
    h.set_options(0)
    h.cg_begin(b)
    assert status_of(h.cg_run, -1, 0.0) == ERR_ARG
    assert status_of(h.cg_run, 1, -1.0) == ERR_ARG
    assert status_of(h.cg_history, 10**6) == ERR_ARG  # (past what lz_cg_run was asked for)
    h.set_dense_cplx(np.eye(4, dtype=np.complex128))
    assert status_of(h.cg_begin, np.ones(4)) == ERR_STATE
    h.close()


def test_one_handle_serves_eigsh_cg_minres_cg():
    A, b, d, _ = problem("well33x31", "jacobi", 1e-6, 0)
    other = np.random.default_rng(4).uniform(0.5, 2.0, A.shape[0])
    fresh_w = eigsh(A, k=3, which="LA", return_eigenvectors=False)
    fresh_x, _ = cg(A, b, rtol=1e-8, M="jacobi")
    fresh_m, _ = minres(A, b, rtol=1e-8)
    fresh_o, _ = cg(A, b, rtol=1e-8, M=sp.diags(other), maxiter=40)
    fresh_p, _ = cg(A, b, rtol=1e-8, maxiter=40)
    h = _capi.Handle(0)
    assert np.array_equal(eigsh(A, k=3, which="LA", return_eigenvectors=False, handle=h), fresh_w)
    assert np.array_equal(cg(A, b, rtol=1e-8, M="jacobi", handle=h)[0], fresh_x)
    assert np.array_equal(minres(A, b, rtol=1e-8, handle=h)[0], fresh_m)
    assert np.array_equal(cg(A, b, rtol=1e-8, M=sp.diags(other), maxiter=40, handle=h)[0], fresh_o)
    assert np.array_equal(cg(A, b, rtol=1e-8, maxiter=40, handle=h)[0], fresh_p)  # (no M behind one: d is not read)
    assert not np.array_equal(fresh_o, fresh_p)
    # the two solvers' states live side by side on one matrix
    h.minres_begin(b)
    h.cg_begin(b, None, d)
    h.minres_run(3, 0.0)
    assert h.cg_run(3, 0.0)["iterations"] == 3 and h.minres_run(1, 0.0)["iterations"] == 4
    h.close()
