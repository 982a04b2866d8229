"""``lsmr`` on the device: one step of ``lz_lsmr_run`` from an uploaded state against longdouble with forward-error bounds
(tests/lsmr_reference.py), the lagged update against its flush, the gate of a chunk, the function end to end on the cases of
tests/test_lsmr_host.py with the stopping inequality each result claims, and the life of a handle that serves ``svds``, ``lsmr``
and ``eigsh`` in turn."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from lsmr_reference import CHECKED, SCALARS, family, ld_operator, loop, random_state, step, step_bounds, worst
from minres_reference import named
from test_lsmr_host import CASES, case_id, host, problem, unit

from lanczos_amd import _capi, eigsh, lsmr, svds
from lanczos_amd.lsmr import DeviceLsmrBackend, NumpyLsmrBackend, solve
from lanczos_amd.svds import _pack

pytestmark = pytest.mark.gpu

VECTORS = ("x", "u", "v", "h", "hbar")
ERR_ARG, ERR_STATE = -1, -4  # LZ_ERR_ARG, LZ_ERR_STATE (include/lanczos_hip.h)


def set_matrix(h, A):
    """the rectangular matrix of ``h`` = ``A`` as ``lsmr`` packs it -> ``transposed``"""
    Aop, AopT, transposed = _pack(A)
    if isinstance(Aop, np.ndarray):
        wide = not Aop.flags.c_contiguous
        h.gk_set_dense(AopT if wide else Aop, stored_transposed=wide)
    else:
        h.gk_set_csr(Aop, AopT)
    return transposed


def status_of(call, *args):
    with pytest.raises(_capi.LanczosHipError) as e:
        call(*args)
    return e.value.status


@functools.lru_cache(maxsize=None)
def step_matrix(name):
    """-> (A, tuning knob 4 or None)"""
    if name.startswith("ragged700"):
        A = named("ragged1000")[:, :700].tocsr()  # empty rows and a row of some 200 entries
        assert (np.diff(A.indptr) == 0).sum() >= 5 and np.diff(A.indptr).max() >= 150
        A = A.T.tocsr() if name.endswith("T") else A
        A.sort_indices()
        return A, None
    if name.startswith("band"):  # three entries a row: both streaming loops take a second trip past 2048 x 256 positions
        m = 1200001
        rng = np.random.default_rng(5)
        rows = np.repeat(np.arange(m), 3)
        cols = (rows + np.tile([0, 1, 2], m)) % 65
        A = sp.csr_matrix((rng.standard_normal(3 * m), (rows, cols)), shape=(m, 65))
        A = A.T.tocsr() if name.endswith("T") else A
        A.sort_indices()
        return A, None
    kind, shape = name.split("_")
    m, n = (int(v) for v in shape.split("x"))
    rng = np.random.default_rng(m + 3 * n)
    if kind == "dense":
        return np.ascontiguousarray(rng.standard_normal((m, n))), None
    if kind == "denseF":
        return np.asfortranarray(rng.standard_normal((m, n))), None
    if kind == "long":  # rows of some 600 entries on the short side, cut into segments of 256: the segment path, in both roles
        A = sp.random(m, n, density=0.6, random_state=rng, data_rvs=rng.standard_normal).tocsr()
        A.sort_indices()
        return A, 256
    if min(m, n) <= 5:
        A = sp.csr_matrix(rng.standard_normal((m, n)))
        A.sort_indices()
        return A, None
    return family(m, n), None


def _set(h, s, transposed):
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    h.lsmr_set_state(s["k"], f(s["x"]), f(s["u"]), f(s["v"]), f(s["h"]), f(s["hbar"]), [float(s[key]) for key in SCALARS],
                     transposed=transposed)


def _state_vectors(h, raw=False):
    return {name: h.lsmr_get(name, raw=raw) for name in VECTORS}


# ---------------------------------------------------------------- a. one step against longdouble
STEP_CASES = ["csr_2x2", "csr_5x3", "csr_3x5", "csr_255x257", "csr_256x256", "csr_257x255", "long_1000x37", "long_37x1000", "ragged700",
              "ragged700T", "band", "bandT", "dense_64x64", "dense_513x130", "dense_130x513", "denseF_513x130"]


@pytest.mark.parametrize("name", STEP_CASES)
def test_one_step_against_longdouble(name):
    A, knob = step_matrix(name)
    m, n = A.shape
    s = random_state(A, 3, m + n + 11, damp=0.3)
    Ad = ld_operator(A)
    out = step(Ad, s)
    bound = step_bounds(A, s, out)
    h = _capi.Handle(0)
    if knob is not None:
        h.set_tuning(_capi.TUNE_STREAM_ENTRIES, knob)
    transposed = set_matrix(h, A)
    assert transposed == (m < n)
    assert h.gk_plan()[0] == (1 if name.startswith("dense") else 0)
    _set(h, s, transposed)
    plan = h.lsmr_info()
    assert plan == {"own_launches_per_iteration": 4, "live": True, "transposed": transposed}
    st = h.lsmr_run(1, 0.0, 0.0, 0.0)
    got = _state_vectors(h)
    raw = _state_vectors(h, raw=True)
    assert st["iterations"] == 3  # (on the tiny shapes step 3 meets a machine-precision test: the flush ends the step all the same)
    assert st["done"] == (st["istop"] != 0) and (min(m, n) <= 5 or not st["done"])
    err = lambda a, ref: np.abs(np.asarray(a - ref, dtype=np.float64))  # noqa: E731
    figures = {
        "uh": worst(err(raw["u"][:m], out["uh"]), bound["uh"]),
        "vh": worst(err(raw["v"][:n], out["vh"]), bound["vh"]),
        "u": worst(err(got["u"], out["u"]), bound["u"]),
        "v": worst(err(got["v"], out["v"]), bound["v"]),
        "x": worst(err(got["x"], out["x_out"]), bound["x"]),
        "h": worst(err(got["h"], out["h_out"]), bound["h"]),
        "hbar": worst(err(got["hbar"], out["hbar_out"]), bound["hbar"]),
    }
    for key in CHECKED + ("normx", "normx_lagged"):
        figures[key] = abs(float(st[key] - out[key])) / bound[key]
    print(f"{name:14s} error / bound: " + "  ".join(f"{key} {val:.2e}" for key, val in figures.items()))
    for key, val in figures.items():
        assert val <= 1.0, key
    hist = h.lsmr_history(3)
    assert np.array_equal(hist, [[0.0, 0.0], [0.0, 0.0], [st["normr"], st["normar"]]])
    for key in VECTORS:
        length = m if key == "u" else n
        assert np.all(np.isfinite(raw[key])) and np.all(raw[key][length:] == 0.0), key
        if key not in ("u", "v"):
            assert np.array_equal(raw[key][:length], got[key])
    # u and v are formed on read: the raw vectors divided by beta and alpha
    assert np.array_equal(raw["u"][:m] / st["beta"], got["u"]) and np.array_equal(raw["v"][:n] / st["alpha"], got["v"])
    # the same call from the same state: the same bits
    _set(h, s, transposed)
    st2 = h.lsmr_run(1, 0.0, 0.0, 0.0)
    again = _state_vectors(h, raw=True)
    assert st2 == st
    for key in VECTORS:
        assert np.array_equal(again[key], raw[key]), key
    h.close()


def test_what_a_step_only_moves_is_equal_bit_for_bit():
    """from the empty pending update on ``h = hbar = 0`` (the state ``lz_lsmr_begin`` leaves) a step only moves ``v_k``: the lagged pass
    makes ``h_k = v_k`` and keeps ``x``, and the flush makes ``hbar_k = h_k - c1 0 = v_k``"""
    A, _ = step_matrix("csr_257x255")
    n = A.shape[1]
    s = random_state(A, 3, 5)
    for key in ("c1", "c2", "c3"):
        s[key] = np.longdouble(0)
    s["h"] = s["hbar"] = np.zeros(n, dtype=np.longdouble)
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    h = _capi.Handle(0)
    transposed = set_matrix(h, A)
    _set(h, s, transposed)
    h.lsmr_run(0, 0.0, 0.0, 0.0)  # (no step: nothing is applied)
    before = _state_vectors(h)
    for key in VECTORS:
        assert np.array_equal(before[key], f(s[key])), key
    # one step, stopped by tolerances nothing misses: the flag is set behind it and the flush, which is not gated, ends the step
    st = h.lsmr_run(1, 1e300, 1e300, 0.0)
    assert st["done"] and st["istop"] == 1 and st["iterations"] == 3
    assert st["normx_lagged"] == np.sqrt(np.sum(f(s["x"]) ** 2)) or abs(st["normx_lagged"] - np.linalg.norm(f(s["x"]))) <= 1e-13 * st["normx_lagged"]
    assert np.array_equal(h.lsmr_get("hbar"), f(s["v"]))
    h.close()


# ---------------------------------------------------------------- b. the lag and its flush
@pytest.mark.parametrize("name", ["csr_257x255", "csr_255x257", "dense_513x130", "dense_130x513"])
def test_six_single_steps_equal_one_chunk_of_six(name):
    A, _ = step_matrix(name)
    m, n = A.shape
    b = np.random.default_rng(2).standard_normal(m)
    h = _capi.Handle(0)
    transposed = set_matrix(h, A)
    h.lsmr_begin(b, None, 0.25, transposed=transposed)
    for _ in range(6):
        st1 = h.lsmr_run(1, 0.0, 0.0, 0.0)
    single = _state_vectors(h, raw=True)
    hist1 = h.lsmr_history(6)
    h.lsmr_begin(b, None, 0.25, transposed=transposed)
    st6 = h.lsmr_run(6, 0.0, 0.0, 0.0)
    chunk = _state_vectors(h, raw=True)
    assert st1 == st6 and st6["iterations"] == 6
    assert np.array_equal(hist1, h.lsmr_history(6))
    for key in VECTORS:
        assert np.array_equal(single[key], chunk[key]), key
    # and the sixth iterate is the longdouble loop's
    ref = np.asarray(loop(A, b, 0.25, 6)["x_out"], dtype=np.float64)
    assert np.linalg.norm(chunk["x"][:n] - ref) <= 1e-12 * np.linalg.norm(ref)
    h.close()


# ---------------------------------------------------------------- c. the gate
def test_gate_inside_the_first_chunk():
    A, b = problem((600, 200), True)
    info = {}
    x, istop, itn, normr, normar, normA, condA, normx = lsmr(A, b, atol=1e-6, btol=1e-6, check_every=256, info=info)
    ref = host(A, b, atol=1e-6, btol=1e-6)
    print(f"gate: {itn} steps on the device, {ref[2]} on the host, istop {istop}")
    assert istop == ref[1] and info["chunks"] == 1 and abs(itn - ref[2]) <= 1
    # the history past the stopping step is untouched: the gated kernels of the rest of the chunk wrote nothing
    h = _capi.Handle(0)
    transposed = set_matrix(h, A)
    h.lsmr_begin(b, transposed=transposed)
    st = h.lsmr_run(200, 1e-6, 1e-6, 1e8)
    assert st["done"] and st["iterations"] == itn and st["istop"] == istop
    raw = h.lsmr_history(200)
    assert np.array_equal(raw[:itn], info["history"]) and itn < 100 and np.all(raw[itn:] == 0.0)
    assert np.array_equal(h.lsmr_get("x"), x) and st["normx"] == normx
    vectors = _state_vectors(h, raw=True)
    assert h.lsmr_run(200, 1e-6, 1e-6, 1e8) == st  # a call on a state that is done changes nothing
    for key in VECTORS:
        assert np.array_equal(h.lsmr_get(key, raw=True), vectors[key]), key
    h.close()


# ---------------------------------------------------------------- d. end to end
@functools.lru_cache(maxsize=None)
def host_result(case):
    shape, consistent, damp, tol = case
    A, b = problem(shape, consistent)
    return host(A, b, damp, tol, tol)


def _e2e(case, dense):
    shape, consistent, damp, tol = case
    A, b = problem(shape, consistent)
    info = {}
    if dense:  # F as one dense array on the device (through lsmr itself it would be packed as CSR: 12 nnz < 8 size), the same host loop
        h = _capi.Handle(0)
        D = A.toarray()
        wide = shape[0] < shape[1]
        h.gk_set_dense(D, stored_transposed=wide)
        assert h.gk_plan()[:2] == (1, 1 if wide else 0)
        x, istop, itn, normr, normar, normA, condA, normx = solve(DeviceLsmrBackend(h, wide, "dense"), b, None, damp, tol, tol, 1e8,
                                                                  min(shape), 8, info=info)
        h.close()
    else:
        x, istop, itn, normr, normar, normA, condA, normx = lsmr(A, b, damp, tol, tol, info=info)
    ref = host_result(case)
    r = b - A @ x
    rbar = np.sqrt(r @ r + damp * damp * (x @ x))
    ar = np.linalg.norm(A.T @ r - damp * damp * x)
    nb, nx = np.linalg.norm(b), np.linalg.norm(x)
    claim = rbar / (tol * nb + tol * normA * nx) if istop == 1 else ar / (tol * normA * rbar)

    def rel(est, true):
        return 0.0 if est < 1e-12 * nb and true < 1e-12 * nb else abs(est - true) / true

    figures = {"normr": rel(normr, rbar), "normar": rel(normar, ar), "normx": rel(normx, nx)}
    print(f"{case_id(case)} {'dense' if dense else 'csr'}: istop {istop} (host {ref[1]}), itn {itn} (host {ref[2]}), claimed inequality at "
          f"{claim:.3f} of its bound, estimates off by " + "  ".join(f"{key} {val:.2e}" for key, val in figures.items()))
    assert info["plan"] == ("dense" if dense else "csr") and info["transposed"] == (shape[0] < shape[1])
    assert info["own_launches_per_iteration"] == 4 and info["iterations"] == itn and info["history"].shape == (itn, 2)
    assert istop == ref[1] and istop in (1, 2)
    assert abs(itn - ref[2]) <= 1
    assert claim <= 2.0
    for key, val in figures.items():
        assert val <= 1e-6, key


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_end_to_end_csr(case):
    _e2e(case, dense=False)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ((600, 200), (200, 600))], ids=case_id)
def test_end_to_end_dense(case):
    _e2e(case, dense=True)


@pytest.mark.parametrize("name", ["dense_513x130", "dense_130x513", "denseF_513x130", "float32_130x513"])
def test_dense_input_through_lsmr(name, capsys):
    """a dense array stays dense through ``lsmr`` itself: C- and F-ordered, tall and wide, and float32 with its notice"""
    from lanczos_amd._solver import LanczosBase

    A, _ = step_matrix(name.replace("float32", "dense"))
    if name.startswith("float32"):
        A = A.astype(np.float32)
    b = np.random.default_rng(6).standard_normal(A.shape[0])
    info = {}
    verbose, LanczosBase.verbose = LanczosBase.verbose, True
    try:
        got = lsmr(A, b, 0.2, 1e-9, 1e-9, info=info)
    finally:
        LanczosBase.verbose = verbose
    assert ("float32 input is converted" in capsys.readouterr().out) == name.startswith("float32")
    A64 = np.asarray(A, dtype=np.float64)
    ref = lsmr(A64, b, 0.2, 1e-9, 1e-9, _backend=NumpyLsmrBackend(A64))
    assert info["plan"] == "dense" and info["transposed"] == (A.shape[0] < A.shape[1])
    assert got[1] == ref[1] and abs(got[2] - ref[2]) <= 1
    assert np.linalg.norm(got[0] - ref[0]) <= 1e-7 * np.linalg.norm(ref[0])  # (a step more or less at 1e-9)


# ---------------------------------------------------------------- e. check_every does not change x
@pytest.mark.parametrize("shape", [(600, 200), (200, 600)])
def test_check_every_gives_the_same_bits(shape):
    A, b = problem(shape, False)
    outs = [lsmr(A, b, 0.1, 1e-8, 1e-8, check_every=ce) for ce in (1, 8, 32)]
    for out in outs[1:]:
        assert np.array_equal(out[0], outs[0][0]) and out[1:] == outs[0][1:]


def test_x0_and_maxiter_on_the_device():
    A, b = problem((600, 200), True)
    x0 = np.random.default_rng(3).standard_normal(200)
    h = _capi.Handle(0)
    transposed = set_matrix(h, A)
    h.lsmr_begin(b, x0, 0.0, transposed=transposed)
    r0 = np.linalg.norm(b - A @ x0)
    st = h.lsmr_run(0, 0.0, 0.0, 0.0)
    assert abs(st["normr"] - r0) <= 1e-13 * r0 and abs(st["normb"] - np.linalg.norm(b)) <= 1e-13 * np.linalg.norm(b)
    h.close()
    x, istop, itn, normr, normar, normA, condA, normx = lsmr(A, b, atol=1e-9, btol=1e-9, x0=x0)
    assert istop == 1 and np.linalg.norm(b - A @ x) <= 2 * (1e-9 * np.linalg.norm(b) + 1e-9 * normA * np.linalg.norm(x))
    ref = host(A, b, atol=1e-12, btol=1e-12, maxiter=5)
    got = lsmr(A, b, atol=1e-12, btol=1e-12, maxiter=5, check_every=2)
    assert got[1] == ref[1] == 7 and got[2] == 5 and np.linalg.norm(got[0] - ref[0]) <= 1e-13 * np.linalg.norm(ref[0])


# ---------------------------------------------------------------- f. the life of a handle
def test_handle_serves_svds_lsmr_svds_and_eigsh():
    A, b = problem((600, 200), False)
    S = family(300, 300)
    S = (S + S.T).tocsr()
    h = _capi.Handle(0)
    lam = eigsh(S, k=3, which="LA", handle=h, return_eigenvectors=False)
    u1, s1, vh1 = svds(A, k=3, handle=h)
    x = lsmr(A, b, atol=1e-9, btol=1e-9, handle=h)
    assert x[1] in (1, 2) and np.array_equal(x[0], lsmr(A, b, atol=1e-9, btol=1e-9)[0])
    assert h.lsmr_info()["live"]
    u2, s2, vh2 = svds(A, k=3, handle=h)
    assert np.array_equal(s1, s2) and np.array_equal(u1, u2) and np.array_equal(vh1, vh2)
    assert not h.lsmr_info()["live"]  # (svds set the matrix again)
    # the square matrix set for eigsh still answers
    y = np.random.default_rng(1).standard_normal(300)
    assert np.allclose(h.spmv_host(y), S @ y, rtol=0, atol=1e-12 * np.linalg.norm(y) * 30)
    lam2 = eigsh(S, k=3, which="LA", handle=h, return_eigenvectors=False)
    assert np.array_equal(lam, lam2)
    h.close()


# ---------------------------------------------------------------- g. state errors
def _begin_without_matrix(h):
    b = np.ones(8)
    h.check(h.lib.lz_lsmr_begin(h._h, 0, _capi.dptr(b), None, 0.0))


def test_state_errors():
    A = family(30, 20)
    b = np.ones(30)
    h = _capi.Handle(0)
    assert status_of(_begin_without_matrix, h) == ERR_STATE
    transposed = set_matrix(h, A)
    h.lsmr_transposed = transposed
    assert not h.lsmr_info()["live"]
    assert status_of(h.lsmr_run, 1, 0.0, 0.0, 0.0) == ERR_STATE
    h.lsmr_begin(b)
    assert h.lsmr_info()["live"] and h.lsmr_run(2, 0.0, 0.0, 0.0)["iterations"] == 2
    assert status_of(h.lsmr_run, -1, 0.0, 0.0, 0.0) == ERR_ARG
    assert status_of(h.lsmr_run, 1, -1.0, 0.0, 0.0) == ERR_ARG
    assert status_of(lambda: h.check(h.lib.lz_lsmr_get(h._h, 5, _capi.dptr(np.zeros(64))))) == ERR_ARG
    assert status_of(lambda: h.check(h.lib.lz_lsmr_get(h._h, -1, _capi.dptr(np.zeros(64))))) == ERR_ARG
    assert status_of(h.lsmr_history, 5000) == ERR_ARG
    assert status_of(lambda: h.check(h.lib.lz_lsmr_begin(h._h, 2, _capi.dptr(b), None, 0.0))) == ERR_ARG
    h.lsmr_begin(b)
    assert all(t > 0.0 for t in h.lsmr_step_time(2))  # (the probe's timer spends the state)
    assert status_of(h.lsmr_run, 1, 0.0, 0.0, 0.0) == ERR_STATE
    h.lsmr_begin(b)
    set_matrix(h, A)  # a new matrix drops the state
    assert not h.lsmr_info()["live"]
    assert status_of(h.lsmr_run, 1, 0.0, 0.0, 0.0) == ERR_STATE
    assert status_of(h.lsmr_get, "x") == ERR_STATE
    h.set_options(_capi.FLAG_REORTH_PARTIAL)
    assert status_of(h.lsmr_begin, b) == ERR_STATE
    h.set_options(0)
    h.lsmr_begin(b)
    assert h.lsmr_run(1, 0.0, 0.0, 0.0)["iterations"] == 1
    h.close()


# ---------------------------------------------------------------- h. the breakdown cases
@pytest.mark.parametrize("name", ["zero", "exact", "inconsistent", "wide"])
def test_breakdown_cases_equal_the_host(name):
    E = sp.eye(4, 7).tocsr() if name == "wide" else sp.eye(7, 4).tocsr()
    b = {"zero": unit(7, (6, 2.0)), "exact": unit(7, (2, 3.0)), "inconsistent": unit(7, (2, 3.0), (7, 1.0)),
         "wide": np.array([1.0, 2.0, 3.0, 4.0])}[name]
    got, ref = lsmr(E, b), lsmr(E, b, _backend=NumpyLsmrBackend(E))
    print(name, got[1:], ref[1:])
    assert got[1:3] == ref[1:3] == {"zero": (0, 0), "exact": (1, 1), "inconsistent": (2, 1), "wide": (1, 1)}[name]
    assert np.allclose(got[0], ref[0], rtol=0, atol=1e-15)
    for g, r in zip(got[3:], ref[3:]):
        assert abs(g - r) <= 1e-14 * max(abs(r), 1.0)
