"""``minres`` on the device: one step of ``lz_minres_run`` from an uploaded state against longdouble with forward-error bounds
(tests/minres_reference.py), the lagged update against its flush, the gate of a chunk, the function end to end at the host tests'
bars (tests/test_minres_host.py) on every product plan, and the life of a handle that serves ``eigsh``, ``minres`` and
``expm_multiply`` in turn."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from minres_reference import SCALARS, dense_ld, lap2d, loop, named, random_state, step, step_bounds, worst
from test_minres_host import problem

from lanczos_amd import StencilOperator, _capi, eigsh, expm_multiply, minres
from lanczos_amd.eigsh import upload_matrix
from lanczos_amd.minres import NumpyMinresBackend

pytestmark = pytest.mark.gpu

VECTORS = ("x", "v", "v_prev", "w1", "w2", "r")
ERR_ARG, ERR_STATE = -1, -4  # LZ_ERR_ARG, LZ_ERR_STATE (include/lanczos_hip.h)


def _handle(A):
    h = _capi.Handle(0)
    upload_matrix(h, A)
    return h


def status_of(call, *args):
    with pytest.raises(_capi.LanczosHipError) as e:
        call(*args)
    return e.value.status


@functools.lru_cache(maxsize=None)
def step_matrix(name):
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


def _set(h, s):
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    h.minres_set_state(s["k"], f(s["x"]), f(s["v"]), f(s["v_prev"]), f(s["w1"]), f(s["w2"]), [float(s[key]) for key in SCALARS])


def _state_vectors(h, raw=False):
    return {name: h.minres_get(name, raw=raw) for name in VECTORS}


# ---------------------------------------------------------------- a. one step against longdouble
STEP_CASES = ["csr_2", "csr_5", "csr_255", "csr_256", "csr_257", "ragged1000", "band70001", "dense_64", "dense_513"]


@pytest.mark.parametrize("name", STEP_CASES)
def test_one_step_against_longdouble(name):
    A = step_matrix(name)
    n = A.shape[0]
    s = random_state(A, 3, n + 11)
    out = step(dense_ld(A), s)
    bound = step_bounds(A, s, out)
    h = _handle(A)
    _set(h, s)
    plan = h.minres_info()  # (csr_5 is a full 5 x 5 matrix: five entries in every row, so its product is the ELL one and scales on read)
    assert plan["launches_per_iteration"] == 4 and plan["live"] and plan["scale_on_read"] == (name == "csr_5")
    st = h.minres_run(1, 0.0)
    got = _state_vectors(h)
    raw = _state_vectors(h, raw=True)
    assert st["iterations"] == 3 and not st["done"]
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    err = lambda a, ref: np.abs(np.asarray(a - ref, dtype=np.float64))  # noqa: E731
    figures = {
        "r": worst(err(got["r"], out["r"]), bound["r"]),
        "w": worst(err(got["w1"], out["w1"]), bound["w"]),
        "x": worst(err(got["x"], out["x"]), bound["x"]),
        "v": worst(err(got["v"], out["v"]), bound["v"]),
        "alpha": abs(float(st["alpha"] - out["alpha"])) / bound["alpha"],
        "beta": abs(float(st["beta"] - out["beta"])) / bound["beta"],
        "phi": abs(float(st["phi"] - out["phi"])) / bound["phi"],
        "phibar": abs(float(st["phibar"] - out["phibar"])) / bound["phibar"],
    }
    print(f"{name:12s} error / bound: " + "  ".join(f"{key} {val:.2e}" for key, val in figures.items()))
    for key, val in figures.items():
        assert val <= 1.0, key
    # what the step moves and what it leaves: v_k is the new v_{k-1} bit for bit, w_{k-1} the new w_{k-2}
    assert np.array_equal(got["v_prev"], f(s["v"])) and np.array_equal(got["w2"], f(s["w1"]))
    assert np.array_equal(h.minres_history(3), [0.0, 0.0, st["phibar"]])
    for key in VECTORS:
        assert np.all(np.isfinite(raw[key])) and np.all(raw[key][n:] == 0.0), key
        assert np.array_equal(raw[key][:n], got[key])
    # the same call from the same state: the same bits
    _set(h, s)
    st2 = h.minres_run(1, 0.0)
    again = _state_vectors(h)
    assert st2 == st
    for key in VECTORS:
        assert np.array_equal(again[key], got[key]), key
    h.close()


# ---------------------------------------------------------------- b. the lag and its flush
@pytest.mark.parametrize("name", ["lap2d", "stencil"])
def test_six_single_steps_equal_one_chunk_of_six(name):
    A = lap2d(33, 31) if name == "lap2d" else stencil()
    n = A.shape[0]
    b = np.random.default_rng(2).standard_normal(n)
    h = _handle(A)
    h.minres_begin(b, None, 0.25)
    for _ in range(6):
        st1 = h.minres_run(1, 0.0)
    single = _state_vectors(h)
    hist1 = h.minres_history(6)
    h.minres_begin(b, None, 0.25)
    st6 = h.minres_run(6, 0.0)
    chunk = _state_vectors(h)
    assert st1 == st6 and st6["iterations"] == 6
    assert np.array_equal(hist1, h.minres_history(6))
    for key in VECTORS:
        assert np.array_equal(single[key], chunk[key]), key
    # and the sixth iterate is the longdouble loop's
    ref = np.asarray(loop(A.to_scipy() if name == "stencil" else A, b, 0.25, 6)["x"], dtype=np.float64)
    assert np.linalg.norm(chunk["x"] - ref) <= 1e-12 * np.linalg.norm(ref)
    h.close()


# ---------------------------------------------------------------- c. the gate
def test_gate_inside_the_first_chunk():
    A, b, _ = problem("definite")
    info, ref = {}, {}
    x, code = minres(A, b, rtol=1e-6, check_every=256, info=info)
    minres(A, b, rtol=1e-6, info=ref, _backend=NumpyMinresBackend(A))
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print(f"gate: {info['iterations']} steps on the device, {ref['iterations']} on the host, residual {res / 1e-6:.3f} rtol")
    assert code == 0 and info["chunks"] == 1
    assert abs(info["iterations"] - ref["iterations"]) <= 1
    assert res <= 2e-6
    # the history past the stopping step is untouched: the gated kernels of the rest of the chunk wrote nothing
    h = _handle(A)
    h.minres_begin(b)
    st = h.minres_run(256, 1e-6)
    assert st["done"] and st["iterations"] == info["iterations"]
    k = st["iterations"]
    raw = h.minres_history(256)
    assert np.array_equal(raw[:k], info["history"]) and raw[k - 1] <= 1e-6 * st["beta1"] < raw[k - 2]
    assert k < 200 and np.all(raw[k:] == 0.0)
    assert np.array_equal(h.minres_get("x"), x)
    assert h.minres_run(256, 1e-6) == st  # a call on a state that is done changes nothing
    assert np.array_equal(h.minres_get("x"), x)
    h.close()


# ---------------------------------------------------------------- d. end to end at the host tests' bars
@functools.lru_cache(maxsize=None)
def stencil():
    """a 7-point stencil with a potential, assembled on the device: row-class coded, so the product scales on read"""
    pot = np.random.default_rng(8).uniform(6.5, 7.5, 12 * 10 * 8)
    return StencilOperator((12, 10, 8), 7, potential=pot)


def _e2e(A, b, shift, rtol, ref_matrix, scale_on_read=False, **kw):
    info, ref = {}, {}
    h = _capi.Handle(0)
    x, code = minres(A, b, shift=shift, rtol=rtol, info=info, handle=h, **kw)
    plan = h.minres_info()
    h.close()
    minres(ref_matrix, b, shift=shift, rtol=rtol, info=ref, _backend=NumpyMinresBackend(ref_matrix))
    res = np.linalg.norm(b - (ref_matrix @ x - shift * x)) / np.linalg.norm(b)
    print(f"shift {shift:g} rtol {rtol:g}: {info['iterations']} steps (host {ref['iterations']}), residual {res / rtol:.3f} rtol, "
          f"scale on read {plan['scale_on_read']}")
    assert code == 0 and res <= 2 * rtol
    assert np.all(np.diff(info["history"]) <= 0.0)
    assert plan == {"launches_per_iteration": 4, "scale_on_read": scale_on_read, "live": True}
    assert info["launches_per_iteration"] == 4
    return info["iterations"], ref["iterations"]


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("dense", [False, True], ids=["csr", "dense"])
@pytest.mark.parametrize("name", ["definite", "indefinite"])
def test_end_to_end_lap2d(name, dense, rtol):
    A, b, shift = problem(name)
    it, ref = _e2e(A.toarray() if dense else A, b, shift, rtol, A)
    if name == "definite":
        assert abs(it - ref) <= 1
    else:
        assert abs(it - ref) <= 0.03 * ref


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
def test_end_to_end_consistent_singular(rtol):
    A, b, shift = problem("periodic")
    it, ref = _e2e(A, b, shift, rtol, A)
    assert abs(it - ref) <= 1


@pytest.mark.parametrize("rtol", [1e-6, 1e-10])
@pytest.mark.parametrize("shift", [0.0, 7.0], ids=["far", "inside"])  # 7.0 lies among the potential's values: many more steps
def test_end_to_end_scale_on_read(shift, rtol):
    A = stencil()
    S = A.to_scipy()
    b = np.random.default_rng(9).standard_normal(S.shape[0])
    it, ref = _e2e(A, b, shift, rtol, S, scale_on_read=True)
    assert abs(it - ref) <= max(1, 0.03 * ref)


# ---------------------------------------------------------------- e. check_every and callback do not change x
def test_check_every_one_and_callback_give_the_same_bits():
    A, b, _ = problem("definite")
    x32, code = minres(A, b, rtol=1e-8, check_every=32)
    assert code == 0
    x1, _ = minres(A, b, rtol=1e-8, check_every=1)
    seen = []
    info = {}
    xc, _ = minres(A, b, rtol=1e-8, callback=lambda xk: seen.append(xk.copy()), info=info)
    assert np.array_equal(x1, x32) and np.array_equal(xc, x32)
    assert len(seen) == info["iterations"] and np.array_equal(seen[-1], x32)


def test_x0_shift_and_symmetry_check_on_the_device():
    A, b, shift = problem("indefinite")
    x0 = np.random.default_rng(3).standard_normal(A.shape[0])
    info = {}
    x, code = minres(A, b, x0, shift=shift, rtol=1e-8, check=True, info=info)
    r0 = np.linalg.norm(b - (A @ x0 - shift * x0))
    assert abs(info["beta1"] - r0) <= 1e-13 * r0
    assert code == 0 and np.linalg.norm(b - (A @ x - shift * x)) <= 2e-8 * r0
    B = A.tolil()
    B[0, 40] = 3.0
    with pytest.raises(ValueError, match="non-symmetric"):
        minres(B.tocsr(), b, check=True)


# ---------------------------------------------------------------- f. the life of a handle
def test_handle_serves_eigsh_minres_expm_minres():
    A, b, _ = problem("definite")
    h = _capi.Handle(0)
    lam = eigsh(A, k=3, which="LA", handle=h, return_eigenvectors=False)
    assert np.allclose(np.sort(lam), np.linalg.eigvalsh(A.toarray())[-3:], rtol=1e-9, atol=0)
    x, code = minres(A, b, rtol=1e-9, handle=h)
    assert code == 0 and np.linalg.norm(b - A @ x) <= 2e-9 * np.linalg.norm(b)
    y = expm_multiply(A, b, a=-0.1, handle=h)
    lam_all, U = np.linalg.eigh(A.toarray())
    exact = U @ (np.exp(-0.1 * lam_all) * (U.T @ b))
    assert np.linalg.norm(y - exact) <= 1e-10 * np.linalg.norm(exact)
    x2, code = minres(A, b, rtol=1e-9, handle=h)
    assert code == 0 and np.array_equal(x2, x)
    h.close()


# ---------------------------------------------------------------- g. state errors
def test_state_errors():
    A = lap2d(9, 7)
    b = np.ones(63)
    h = _capi.Handle(0)
    assert status_of(_begin_without_matrix, h) == ERR_STATE
    upload_matrix(h, A)
    assert not h.minres_info()["live"]
    assert status_of(h.minres_run, 1, 0.0) == ERR_STATE
    h.minres_begin(b)
    assert h.minres_info()["live"] and h.minres_run(2, 0.0)["iterations"] == 2
    assert all(t > 0.0 for t in h.minres_step_time(2))  # (the probe's timer spends the state)
    assert status_of(h.minres_run, 1, 0.0) == ERR_STATE
    h.minres_begin(b)
    upload_matrix(h, A)  # a new matrix drops the state
    assert not h.minres_info()["live"]
    assert status_of(h.minres_run, 1, 0.0) == ERR_STATE
    assert status_of(h.minres_get, "x") == ERR_STATE
    h.set_options(_capi.FLAG_REORTH_PARTIAL)
    assert status_of(h.minres_begin, b) == ERR_STATE
    h.set_options(0)
    h.minres_begin(b)
    assert status_of(h.minres_run, -1, 0.0) == ERR_ARG
    assert status_of(h.minres_run, 1, -1.0) == ERR_ARG
    h.set_dense_cplx(np.eye(4, dtype=np.complex128))
    assert status_of(h.minres_begin, np.ones(4)) == ERR_STATE
    h.close()


def _begin_without_matrix(h):
    b = np.ones(8)
    h.check(h.lib.lz_minres_begin(h._h, _capi.dptr(b), None, 0.0))
