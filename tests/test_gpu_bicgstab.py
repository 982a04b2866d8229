"""``bicgstab`` on the device: one iteration of ``lz_bicgstab_run`` from an uploaded state against longdouble with forward-error bounds
(tests/bicgstab_reference.py) on every product form and at every length where the passes take another path, the chunking and both
exits, the function end to end on every admitted case of tests/test_bicgstab_host.py, the breakdown codes, and the life of a handle
that serves ``eigs``, ``bicgstab`` and ``minres`` in turn."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from bicgstab_reference import LD, Operator, convdiff, dot_bound, norm_bound, product_bound, random_csr, random_state, skew64, worst
from test_bicgstab_host import CASES, X_MARGIN, problem

from lanczos_amd import _capi, bicgstab, eigs, minres
from lanczos_amd.bicgstab import NumpyBicgstabBackend
from lanczos_amd.eigsh import upload_matrix

pytestmark = pytest.mark.gpu

VECTORS = ("x", "r", "rtilde", "p", "v", "t")
ERR_ARG, ERR_STATE = -1, -4  # LZ_ERR_ARG, LZ_ERR_STATE (include/lanczos_hip.h)
# the passes' launch rule (lz_bicgstab.hip: k_minres_step's): at most 2048 blocks of 256 lanes, two 16-byte positions of a lane in
# flight - above 2 x 2048 x 256 x 2 doubles every lane takes a second trip of the grid-stride loop
SECOND_TRIP = 2 * 2048 * 256 * 2


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


@functools.lru_cache(maxsize=4)
def step_matrix(name):
    kind, size = name.split("_")
    if kind == "convdiff":
        nx, ny = (int(v) for v in size.split("x"))
        return convdiff(nx, ny, 0.6, -0.3, 0.5)
    n = int(size)
    if kind == "dense":
        return np.ascontiguousarray(np.random.default_rng(n).standard_normal((n, n)) + np.sqrt(n) * np.eye(n))
    return random_csr(n, min(3, n))


def _vectors(h, raw=False):
    return {name: h.bicgstab_get(name, raw=raw) for name in VECTORS}


# ---------------------------------------------------------------- a. one iteration against longdouble
LENGTHS = (2, 3, 63, 64, 65, 511, 513)
BIG = SECOND_TRIP + 513
STEP_CASES = ([(f"csr_{n}", k) for n in LENGTHS for k in (0, 3)] + [(f"dense_{n}", k) for n in LENGTHS for k in (0, 3)]
              + [("convdiff_24x20", 0), ("convdiff_24x20", 3), ("convdiff_33x31", 3), (f"csr_{BIG}", 3), ("convdiff_1449x1448", 3)])


@pytest.mark.parametrize("name,k", STEP_CASES)
def test_one_iteration_against_longdouble(name, k):
    A = step_matrix(name)
    n = A.shape[0]
    assert not name.startswith("convdiff_1449") or n > SECOND_TRIP
    op = Operator(A)
    s = random_state(n, k, n + 11 + k)
    h = _handle(A)
    if name.startswith("convdiff"):
        assert h.spmv_coding()[0] == "offsets+values"  # the row-class coded kernel
    h.bicgstab_set_state(k, s["x"], s["r"], s["rtilde"], s["p"], s["v"], s["scalars"])
    plan = h.bicgstab_info()
    assert plan["live"] and plan["launches_per_iteration"] == (9 if plan["dots_in_product"] else 10)
    # (the long random matrix has no column locality: it takes the column-blocked two-phase product, whose epilogue cannot form the dots)
    assert plan["dots_in_product"] == (n < SECOND_TRIP or name.startswith("convdiff"))
    st = h.bicgstab_run(1, 0.0)
    got = _vectors(h)
    raw = _vectors(h, raw=True)
    assert st["iterations"] == k + 1 and not st["done"] and st["exit"] is None and st["code"] == 0
    rho_prev0, alpha0, omega0 = (float(v) for v in s["scalars"])
    rho0 = st["rho_prev"]  # the device's rho of the uploaded state
    figures = {"rho0": abs(float(rho0 - np.dot(s["rtilde"].astype(LD), s["r"].astype(LD)))) / dot_bound(s["rtilde"], s["r"])}
    # p, with the device's own scalars: exact
    if k == 0:
        p = s["r"].copy()
    else:
        beta0 = (rho0 / rho_prev0) * (alpha0 / omega0)
        p = (s["p"] - omega0 * s["v"]) * beta0 + s["r"]
    assert np.array_equal(got["p"], p)
    assert np.array_equal(got["rtilde"], s["rtilde"])
    # v = A p and rv = rtilde . v
    v_ld, dv = op.matvec(p), product_bound(op, p)
    figures["v"] = worst(np.abs(np.asarray(got["v"] - v_ld, dtype=np.float64)), dv)
    figures["rv"] = abs(float(st["rv"] - np.dot(s["rtilde"].astype(LD), v_ld))) / dot_bound(s["rtilde"], got["v"], db=dv)
    alpha = st["alpha"]
    assert alpha == rho0 / st["rv"]
    # s = r - alpha v (through r below, which overwrites it), |s|
    svec = s["r"] - alpha * got["v"]
    s_ld = svec.astype(LD)
    snorm_ld = np.sqrt(np.dot(s_ld, s_ld))
    figures["snorm"] = abs(float(st["snorm"] - snorm_ld)) / norm_bound(dot_bound(svec, svec), snorm_ld)
    # t = A s, t . s, t . t
    t_ld, dt = op.matvec(svec), product_bound(op, svec)
    figures["t"] = worst(np.abs(np.asarray(got["t"] - t_ld, dtype=np.float64)), dt)
    figures["ts"] = abs(float(st["ts"] - np.dot(t_ld, s_ld))) / dot_bound(got["t"], svec, da=dt)
    figures["tt"] = abs(float(st["tt"] - np.dot(t_ld, t_ld))) / dot_bound(got["t"], got["t"], da=dt, db=dt)
    omega = st["omega"]
    assert omega == st["ts"] / st["tt"]
    # x and r: exact
    assert np.array_equal(got["x"], (s["x"] + alpha * p) + omega * svec)
    r = svec - omega * got["t"]
    assert np.array_equal(got["r"], r)
    # rho and |r| of the next iteration, its beta
    r_ld = r.astype(LD)
    figures["rho"] = abs(float(st["rho"] - np.dot(s["rtilde"].astype(LD), r_ld))) / dot_bound(s["rtilde"], r)
    rnorm_ld = np.sqrt(np.dot(r_ld, r_ld))
    figures["rnorm"] = abs(float(st["rnorm"] - rnorm_ld)) / norm_bound(dot_bound(r, r), rnorm_ld)
    assert st["beta"] == (st["rho"] / rho0) * (alpha / omega)
    print(f"{name:20s} k {k} error / bound: " + "  ".join(f"{key} {val:.2e}" for key, val in figures.items()))
    for key, val in figures.items():
        assert val <= 1.0, key
    hist = h.bicgstab_history(k + 1)
    assert np.array_equal(hist[k], [st["snorm"], st["rnorm"]]) and not np.any(hist[:k])
    for key in VECTORS:
        assert np.all(np.isfinite(raw[key])) and np.all(raw[key][n:] == 0.0), key
        assert np.array_equal(raw[key][:n], got[key])
    # the same call from the same state: the same bits
    h.bicgstab_set_state(k, s["x"], s["r"], s["rtilde"], s["p"], s["v"], s["scalars"])
    assert h.bicgstab_run(1, 0.0) == st
    again = _vectors(h)
    for key in VECTORS:
        assert np.array_equal(again[key], got[key]), key
    h.close()


# ---------------------------------------------------------------- b. chunking and the two exits
@pytest.mark.parametrize("name", ["csr_1023", "convdiff_33x31"])
def test_six_single_iterations_equal_one_chunk_of_six(name):
    A = step_matrix(name)
    n = A.shape[0]
    b = np.random.default_rng(2).standard_normal(n)
    h = _handle(A)
    h.bicgstab_begin(b)
    for _ in range(6):
        st1 = h.bicgstab_run(1, 0.0)
    single = _vectors(h)
    hist1 = h.bicgstab_history(6)
    h.bicgstab_begin(b)
    st6 = h.bicgstab_run(6, 0.0)
    chunk = _vectors(h)
    assert st1 == st6 and st6["iterations"] == 6 and not st6["done"]
    assert np.array_equal(hist1, h.bicgstab_history(6)) and np.all(hist1 > 0.0)
    for key in VECTORS:
        assert np.array_equal(single[key], chunk[key]), key
    # and the sixth iterate is the NumPy backend's to rounding
    ref = NumpyBicgstabBackend(A)
    ref.begin(b, None)
    ref.run(6, 0.0)
    assert np.linalg.norm(chunk["x"] - ref.x) <= 1e-12 * np.linalg.norm(ref.x)
    h.close()


@pytest.mark.parametrize("name,rtol,seed,kind", [("convdiff24x20", 1e-6, 0, "half"), ("convdiff24x20", 1e-6, 3, "full"),
                                                 ("random401", 1e-10, 0, "full"), ("random401", 1e-6, 5, "half")])
def test_a_chunk_past_the_exit_changes_nothing(shared, name, rtol, seed, kind):
    A, b, adm = problem(name, rtol, seed)
    one, big = {}, {}
    x1, c1 = bicgstab(A, b, rtol=rtol, check_every=1, handle=shared, info=one)
    x256, c256 = bicgstab(A, b, rtol=rtol, check_every=256, handle=shared, info=big)
    assert c1 == c256 == 0 and one["exit"] == big["exit"] == kind
    assert one["iterations"] == big["iterations"] == adm["runs"]["dot"]["iterations"] < 256 and big["chunks"] == 1
    assert np.array_equal(x1, x256) and np.array_equal(one["history"], big["history"])
    assert one["residual_norm"] == big["residual_norm"] < one["atol_effective"]
    # what the exit leaves on the device: x, and r = the residual of the recurrence (s behind a half step)
    assert np.array_equal(shared.bicgstab_get("x"), x256)
    rvec = shared.bicgstab_get("r")
    assert np.sqrt(np.dot(rvec, rvec)) == pytest.approx(big["residual_norm"], rel=1e-12)
    true = np.asarray(A @ x256).ravel() - b
    assert np.linalg.norm(true + rvec) <= 1e-10 * np.linalg.norm(b)  # (r = b - A x to the recurrence's drift)


# ---------------------------------------------------------------- c. end to end on every admitted case
@pytest.mark.parametrize("form", ["csr", "dense"])
@pytest.mark.parametrize("name,rtol,seed", CASES)
def test_end_to_end_on_the_admitted_cases(shared, name, rtol, seed, form):
    A, b, adm = problem(name, rtol, seed)
    if form == "csr":
        M = A if sp.issparse(A) else sp.csr_matrix(A)
    else:
        M = np.ascontiguousarray(A.toarray()) if sp.issparse(A) else A
    host, dev = {}, {}
    xh, ch = bicgstab(M, b, rtol=rtol, info=host, _backend=NumpyBicgstabBackend(M))
    x, code = bicgstab(M, b, rtol=rtol, handle=shared, info=dev)
    assert code == ch == 0
    assert (dev["iterations"], dev["exit"], dev["code"]) == (host["iterations"], host["exit"], 0)
    assert dev["products"] == host["products"] and dev["launches_per_iteration"] in (9, 10)
    true = np.asarray(Operator(M).matvec(x) - b.astype(LD), dtype=np.float64)
    assert np.linalg.norm(true) <= 2.0 * adm["atol_eff"]
    dist = float(np.linalg.norm(x - xh))
    print(f"{name} {form} rtol {rtol:g} seed {seed}: |x - x_host| {dist:.2e}, spread in x {adm['x_spread']:.2e}, ratio {dist / adm['x_spread']:.2f}, "
          f"true residual / atol_eff {np.linalg.norm(true) / adm['atol_eff']:.3f}")
    assert dist <= X_MARGIN * adm["x_spread"]


# ---------------------------------------------------------------- d. the other exits, x0, callback, the handle's life
def test_breakdown_of_the_skew_matrix_on_the_device(shared):
    A = skew64()
    b = np.random.default_rng(0).standard_normal(64)
    run = {}
    x, code = bicgstab(A, b, handle=shared, info=run)
    assert code == -11 and not np.any(x) and run["exit"] == "breakdown" and run["iterations"] == 0 and run["products"] == 1
    x0 = np.random.default_rng(1).standard_normal(64)
    x, code = bicgstab(A, b, x0, handle=shared)
    assert code == -11 and np.array_equal(x, x0)


@pytest.mark.parametrize("what", ["rho", "omega"])
def test_breakdowns_through_set_state_on_the_device(what):
    A, b, _ = problem("random401", 1e-6, 0)
    n = A.shape[0]
    s = random_state(n, 3, 5)
    scalars = [1.3, 0.7, -0.45]
    if what == "rho":
        s["r"][1::2] = 0.0
        s["rtilde"][0::2] = 0.0
    else:
        scalars[2] = 1e-40
    h = _handle(A)
    h.bicgstab_set_state(3, s["x"], s["r"], s["rtilde"], s["p"], s["v"], scalars)
    st = h.bicgstab_run(8, 1e-9)
    assert st["done"] and st["head"] and st["exit"] == "breakdown" and st["iterations"] == 3
    assert st["code"] == (-10 if what == "rho" else -11)
    assert np.array_equal(h.bicgstab_get("x"), s["x"]) and np.array_equal(h.bicgstab_get("p"), s["p"])
    assert h.bicgstab_run(8, 1e-9) == st  # a state that is done stays as it is
    h.close()


def test_x0_callback_and_identical_bits(shared):
    A, b, _ = problem("convdiff24x20", 1e-10, 10)
    n = A.shape[0]
    x0 = np.random.default_rng(77).standard_normal(n)
    host, dev = {}, {}
    xh, ch = bicgstab(A, b, x0, rtol=1e-8, info=host, _backend=NumpyBicgstabBackend(A))
    x, code = bicgstab(A, b, x0, rtol=1e-8, handle=shared, info=dev)
    assert code == ch == 0 and dev["products"] % 2 == (0 if dev["exit"] == "half" else 1)  # (one product more: A x0)
    assert np.linalg.norm(np.asarray(A @ x).ravel() - b) <= 2.0 * dev["atol_effective"]
    # the matrix is normal with its spectrum right of shift = 0.5: two solutions with residuals below 2 atol_eff lie within 8 atol_eff
    assert np.linalg.norm(x - xh) <= 8.0 * dev["atol_effective"]
    x2, _ = bicgstab(A, b, x0, rtol=1e-8, handle=shared)
    assert np.array_equal(x, x2)
    # callback: one iteration per synchronisation, none for a half-step exit, the last xk is x behind a full step
    calls = []
    run = {}
    xc, code = bicgstab(A, b, rtol=1e-10, handle=shared, info=run, callback=lambda xk: calls.append(xk.copy()))
    plain, code2 = bicgstab(A, b, rtol=1e-10, handle=shared)
    assert code == code2 == 0 and np.array_equal(xc, plain) and run["chunks"] == run["iterations"]
    assert run["exit"] == "full" and len(calls) == run["iterations"] and np.array_equal(calls[-1], xc)
    A2, b2, _ = problem("convdiff24x20", 1e-6, 0)
    calls = []
    run = {}
    bicgstab(A2, b2, rtol=1e-6, handle=shared, info=run, callback=lambda xk: calls.append(xk.copy()))
    assert run["exit"] == "half" and len(calls) == run["iterations"] - 1


def test_one_handle_serves_eigs_bicgstab_minres_bicgstab():
    A, b, _ = problem("convdiff24x20", 1e-6, 0)
    S = (A + A.T).tocsr()
    fresh_w = eigs(A, k=4, which="LM", return_eigenvectors=False)
    fresh_x, _ = bicgstab(A, b, rtol=1e-8)
    fresh_m, _ = minres(S, b, rtol=1e-8)
    h = _capi.Handle(0)
    assert np.array_equal(eigs(A, k=4, which="LM", return_eigenvectors=False, handle=h), fresh_w)
    assert np.array_equal(bicgstab(A, b, rtol=1e-8, handle=h)[0], fresh_x)
    assert np.array_equal(minres(S, b, rtol=1e-8, handle=h)[0], fresh_m)
    assert np.array_equal(bicgstab(A, b, rtol=1e-8, handle=h)[0], fresh_x)
    # the two solvers' states live side by side on one matrix
    h.minres_begin(b)
    h.bicgstab_begin(b)
    h.minres_run(3, 0.0)
    assert h.bicgstab_run(3, 0.0)["iterations"] == 3 and h.minres_run(1, 0.0)["iterations"] == 4
    h.close()


def _begin_without_matrix(h):
    b = np.ones(8)
    h.check(h.lib.lz_bicgstab_begin(h._h, _capi.dptr(b), None))


def test_state_errors():
    A, b, _ = problem("random401", 1e-6, 0)
    h = _capi.Handle(0)
    assert status_of(_begin_without_matrix, h) == ERR_STATE
    upload_matrix(h, A)
    assert not h.bicgstab_info()["live"]
    assert status_of(h.bicgstab_run, 1, 0.0) == ERR_STATE
    assert status_of(h.bicgstab_get, "x") == ERR_STATE
    assert status_of(h.bicgstab_history, 1) == ERR_STATE
    h.bicgstab_begin(b)
    assert h.bicgstab_info()["live"]
    assert status_of(h.bicgstab_step_time, 2) == ERR_STATE  # (nothing has run yet)
    assert h.bicgstab_run(2, 0.0)["iterations"] == 2
    assert all(t > 0.0 for t in h.bicgstab_step_time(2))  # (the probe's timer spends the state)
    assert status_of(h.bicgstab_run, 1, 0.0) == ERR_STATE
    h.bicgstab_begin(b)
    upload_matrix(h, A)  # a new matrix drops the state
    assert not h.bicgstab_info()["live"]
    assert status_of(h.bicgstab_run, 1, 0.0) == ERR_STATE
    assert status_of(h.bicgstab_get, "x") == ERR_STATE
    h.set_options(_capi.FLAG_REORTH_PARTIAL)
    assert status_of(h.bicgstab_begin, b) == ERR_STATE
    h.set_options(0)
    h.bicgstab_begin(b)
    assert status_of(h.bicgstab_run, -1, 0.0) == ERR_ARG
    assert status_of(h.bicgstab_run, 1, -1.0) == ERR_ARG
    h.set_dense_cplx(np.eye(4, dtype=np.complex128))
    assert status_of(h.bicgstab_begin, np.ones(4)) == ERR_STATE
    h.close()
