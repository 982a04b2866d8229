"""``gmres`` on the device.  From uploaded states (``lz_gmres_set_state``): one inner step - the rotated column, the rotations, ``S`` and
``presid`` of k_gmres_column against longdouble within the bounds of tests/gmres_reference.py, the flags at ``ptol`` just above and
just below ``presid`` -, the freeze behind a set flag, and one cycle end - k_gmres_solve (a planted zero pivot included),
k_gmres_update at every length where the pass takes another path with NaN in the rows it must not read, k_gmres_residual with NaN
planted in the padding it must clear, k_gmres_cycle's branches.  End to end: every admitted case of tests/test_gmres_host.py, the
chunking, the breakdown case, a handle that serves ``eigs``, ``gmres`` and ``bicgstab`` in turn, and the error answers.  NaN is only
ever data in buffers the kernels are meant to skip or overwrite."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from bicgstab_reference import LD, Operator, convdiff, product_bound, random_csr, worst

import gmres_reference as gr
from lanczos_amd import _capi, bicgstab, eigs, gmres
from lanczos_amd.eigsh import upload_matrix
from lanczos_amd.gmres import NumpyGmresBackend

pytestmark = pytest.mark.gpu

X_MARGIN = 16  # the project's figure (test_bicgstab_host.py)
ERR_ARG, ERR_STATE = -1, -4  # LZ_ERR_ARG, LZ_ERR_STATE (include/lanczos_hip.h)
EPS = float(np.finfo(np.float64).eps)
# the passes' launch rule (lz_gmres.hip: k_minres_step's): at most 2048 blocks of 256 lanes, two 16-byte positions of a lane in
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
    if name == "convdiff":
        return convdiff(24, 20)
    if name == "dense":
        return gr.matrix("dense130")
    if name == "csr":
        return gr.matrix("random401")
    n = int(name)
    if n > 1000:  # the long one: a bidiagonal matrix, built without a random draw per entry
        return sp.diags([np.full(n, 2.0), np.full(n - 1, -0.5)], [0, 1], format="csr")
    return random_csr(n, min(3, n))


def host_state(A, restart, k, seed=0):
    """the state behind ``k`` inner steps of a solve on the host backend (no flag set): what the device is given to start from"""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    ref = NumpyGmresBackend(A)
    ref.begin(restart, rng.standard_normal(n), rng.standard_normal(n))
    ref.run(k, 1e-300)
    assert ref.cols == k and not ref.inner and not ref.done
    return ref


def upload(h, ref, restart, **changes):
    small = ref.get("small")
    small.update(changes)
    h.gmres_set_state(restart, ref.x, ref.b, ref.w, ref.V[: min(ref.cols + 1, restart)] if "rows" not in changes else changes["rows"], small)
    return small


# ---------------------------------------------------------------- a. one inner step against longdouble
@pytest.mark.parametrize("k", [0, 1, 4, 6])
@pytest.mark.parametrize("name", ["csr", "dense", "convdiff"])
def test_one_inner_step_against_longdouble(name, k):
    A = step_matrix(name)
    restart = 8
    ref = host_state(A, restart, k, seed=k + 1)
    h = _handle(A)
    if name == "convdiff":
        assert h.spmv_coding()[0] == "offsets+values"  # the row-class coded kernel
    before = upload(h, ref, restart, ptol=0.0)
    st = h.gmres_run(1, 1e-300)
    assert st["iterations"] == ref.iters + 1 and st["cols"] == k + 1 and not st["inner"] and not st["done"]
    assert st["cycles"] == 0  # (the column that ends a cycle: test_the_last_column_of_a_cycle_ends_it)
    got = h.gmres_get("small")
    j = k
    (col, c, s, sj, sj1), (ecol, ec, es, esj, esj1) = gr.column_reference(got["proj"][: j + 1], got["h1"], before["gc"][:j], before["gs"][:j],
                                                                            before["S"][j])
    figures = {"column": worst(np.abs(np.asarray(got["R"][j, : j + 1] - col, dtype=np.float64)), ecol),
               "c": abs(float(got["gc"][j] - c)) / ec, "s": abs(float(got["gs"][j] - s)) / es,
               "S[j]": abs(float(got["S"][j] - sj)) / esj, "S[j+1]": abs(float(got["S"][j + 1] - sj1)) / esj1,
               "presid": abs(float(got["presid"] - abs(sj1))) / esj1}
    print(f"{name} step {k} error / bound: " + "  ".join(f"{key} {val:.2e}" for key, val in figures.items()))
    for key, val in figures.items():
        assert val <= 1.0, key
    assert got["h1"] > EPS * np.sqrt(got["h0sq"][j]) and not got["breakdown"]
    # everything the step does not own is as it was
    assert np.array_equal(got["R"][:j], before["R"][:j]) and np.array_equal(got["gc"][:j], before["gc"][:j])
    assert np.array_equal(got["S"][:j], before["S"][:j]) and got["ptol"] == 0.0
    hist, _ = h.gmres_history(ref.iters + 1, 0)
    assert hist[-1] == got["presid"] == st["presid"]
    # the new row is the host backend's to rounding, and of unit length
    rows = h.gmres_get("rows")
    ref._step(j)
    assert np.linalg.norm(rows[j + 1, : ref.n] - ref.V[j + 1]) <= 1e-12 and abs(np.linalg.norm(rows[j + 1]) - 1.0) <= 1e-14
    assert np.all(rows[: j + 2, ref.n:] == 0.0)
    # the flags at ptol just below, at and just above presid; the same state gives the same bits
    ref = host_state(A, restart, k, seed=k + 1)
    for ptol, flag in ((np.nextafter(got["presid"], 0.0), False), (got["presid"], True), (np.nextafter(got["presid"], np.inf), True)):
        upload(h, ref, restart, ptol=ptol)
        st2 = h.gmres_run(1, 1e-300)
        assert st2["inner"] == flag and st2["presid"] == got["presid"] and st2["cols"] == k + 1 and not st2["breakdown"] and not st2["done"]
    h.close()


def test_the_last_column_of_a_cycle_ends_it():
    A = step_matrix("csr")
    ref = host_state(A, 8, 7, seed=8)
    h = _handle(A)
    upload(h, ref, 8)
    st = h.gmres_run(1, 1e-300)
    ref.run(1, 1e-300)
    assert (st["cycles"], st["cols"], st["hcol"], st["iterations"]) == (1, 0, 0, ref.iters) and ref.cycles == 1
    assert np.linalg.norm(h.gmres_get("x") - ref.x) <= 1e-13 * np.linalg.norm(ref.x)
    assert abs(st["rnorm"] - ref.rnorm) <= 1e-12 * ref.rnorm and abs(st["ptol"] - ref.ptol) <= 1e-9 * ref.ptol
    h.close()


def test_a_breakdown_step_sets_both_flags():
    A, b = gr.breakdown_case()
    ref = NumpyGmresBackend(A)
    ref.begin(10, b, None)
    ref.run(2, 1e-300)
    h = _handle(A)
    upload(h, ref, 10)
    st = h.gmres_run(1, 1e-300)
    got = h.gmres_get("small")
    assert st["inner"] and st["breakdown"] and not st["done"] and st["cols"] == 3
    assert got["h1"] <= EPS * np.sqrt(got["h0sq"][2])
    assert got["gc"][2] == 1.0 and got["gs"][2] == 0.0 and got["S"][3] == 0.0 and got["presid"] == 0.0  # lartg(f, 0)
    h.close()


# ---------------------------------------------------------------- b. the freeze
@pytest.mark.parametrize("name", ["csr", "dense"])
def test_steps_behind_a_set_flag_change_nothing(name):
    A = step_matrix(name)
    restart, k = 20, 3
    ref = host_state(A, restart, k, seed=5)
    h = _handle(A)
    upload(h, ref, restart, ptol=1e300)  # the next step passes the inner test
    st1 = h.gmres_run(1, 1e-300)
    small1, rows1, x1 = h.gmres_get("small"), h.gmres_get("rows"), h.gmres_get("x")
    assert st1["inner"] and st1["cols"] == k + 1
    upload(h, ref, restart, ptol=1e300)
    st4 = h.gmres_run(4, 1e-300)
    small4, rows4 = h.gmres_get("small"), h.gmres_get("rows")
    assert st4["hcol"] == k + 4 and {**st4, "hcol": 0} == {**st1, "hcol": 0}
    for key in ("R", "gc", "gs", "S") + _capi.Handle.GMRES_SCALARS:
        assert np.array_equal(small4[key], small1[key]), key
    assert np.array_equal(rows4[: k + 1], rows1[: k + 1]) and np.array_equal(h.gmres_get("x"), x1)
    assert not np.array_equal(rows4[k + 2:], rows1[k + 2:])  # (the frozen steps did write their scratch rows)
    hist, _ = h.gmres_history(ref.iters + 4, 0)
    assert hist[ref.iters] == st1["presid"] and not np.any(hist[ref.iters + 1:])
    # the next call begins with the end of that cycle, from the frozen state
    st = h.gmres_run(0, 1e-300)
    assert st["cycles"] == 1 and st["cols"] == 0 and not st["inner"]
    _, cyc = h.gmres_history(0, 1)
    assert cyc[0, 1] == k + 1 and cyc[0, 2] == 1e300
    h.close()


# ---------------------------------------------------------------- c. one cycle end: solve, update, residual, cycle
LENGTHS = (2, 3, 63, 64, 65, 511, 513, SECOND_TRIP + 513)


def chosen_state(n, restart, cols, seed, zero_pivot=False):
    """numbers of order one for everything a cycle end reads; NaN in every basis row it must not read and in the padding of w"""
    rng = np.random.default_rng(seed)
    R = np.zeros((restart, restart))
    for j in range(restart):
        R[j, : j + 1] = rng.standard_normal(j + 1)
        R[j, j] = (2.0 + abs(R[j, j])) * (-1.0) ** j
    if zero_pivot:
        R[cols - 1, cols - 1] = 0.0
    rows = rng.standard_normal((restart + 1, n))
    rows[cols:] = np.nan
    small = {"R": R, "gc": rng.uniform(0.1, 0.9, restart), "gs": rng.uniform(0.1, 0.9, restart), "S": rng.standard_normal(restart + 1),
             "cols": cols, "ptol": 0.3, "factor": 0.5, "presid": 0.2, "rnorm": 0.0, "bnorm": 1.0, "inner": 0, "breakdown": 0, "done": 0,
             "converged": 0, "iters": cols, "cycles": 0}
    return {"x": rng.standard_normal(n), "b": rng.standard_normal(n), "rows": rows, "small": small}


@pytest.mark.parametrize("which_cols", ["one", "two", "restart"])
@pytest.mark.parametrize("n", LENGTHS)
def test_cycle_end_from_an_uploaded_state(n, which_cols):
    A = step_matrix(str(n))
    restart = min(5, n)
    cols = min({"one": 1, "two": 2, "restart": restart}[which_cols], restart)
    zero_pivot = which_cols == "two" and n in (3, 65)
    s = chosen_state(n, restart, cols, n + cols, zero_pivot)
    h = _handle(A)
    pad = h.padded_rows(n)
    w = np.full(pad, np.nan)  # all of w is overwritten: the product writes [0, n), k_gmres_residual must clear [n, pad)
    h.gmres_set_state(restart, s["x"], s["b"], w, s["rows"], s["small"])
    assert n < SECOND_TRIP or pad // 2 > 2 * 2048 * 256  # the long one: a second trip of the grid-stride loop
    st = h.gmres_end_cycle(0.0)
    y, x, small = h.gmres_get("y"), h.gmres_get("x"), h.gmres_get("small")
    figures = {}
    # k_gmres_solve
    S0 = s["small"]["S"].copy()
    y_ld, ybound = gr.solve_reference(s["small"]["R"], S0, cols, y)
    figures["y"] = worst(np.abs(np.asarray(y[:cols] - y_ld, dtype=np.float64)), ybound)
    assert not np.any(y[cols:])
    if zero_pivot:
        assert y[cols - 1] == 0.0
    # k_gmres_update, given the device's y: rows >= cols hold NaN and were not read
    x_ld, xbound = gr.update_reference(s["x"], y[:cols], s["rows"][:cols])
    figures["x"] = worst(np.abs(np.asarray(x - x_ld, dtype=np.float64)), xbound)
    assert np.all(np.isfinite(x)) and not np.any(h.gmres_get("x", raw=True)[n:])
    # k_gmres_residual, given the device's own product
    Ax = h.spmv_host(x)
    wraw = h.gmres_get("w", raw=True)
    rnorm = st["rnorm"]
    r = s["b"] - Ax
    r_ld, rbound = gr.rnorm_reference(r)
    figures["rnorm"] = abs(float(rnorm - r_ld)) / rbound
    print(f"n {n} cols {cols} error / bound: " + "  ".join(f"{key} {val:.2e}" for key, val in figures.items()))
    for key, val in figures.items():
        assert val <= 1.0, key
    # k_gmres_cycle: the outer test failed (atol = 0) and presid = 0.2 <= ptol = 0.3, so the factor tightens; then the restart
    assert not st["done"] and st["cycles"] == 1 and st["cols"] == 0 and not st["inner"] and st["hcol"] == 0
    assert st["factor"] == 0.125 and st["ptol"] == 0.2 * min(0.125, 0.0 / rnorm)
    assert small["S"][0] == rnorm and not np.any(small["S"][1:]) and not np.any(small["gc"]) and not np.any(small["gs"])
    _, cyc = h.gmres_history(0, 1)
    assert cyc[0].tolist() == [rnorm, float(cols), 0.3]
    # w = b - A x exactly, its padding all zero although NaN was planted there; V[0] = w / |w| exactly
    assert np.array_equal(wraw[:n], r) and not np.any(wraw[n:])
    row0 = h.gmres_get("rows")[0]
    assert np.array_equal(row0[:n], r / rnorm) and not np.any(row0[n:])
    h.close()


@pytest.mark.parametrize("branch", ["converged", "breakdown", "relax", "tighten", "done"])
def test_the_branches_of_the_cycle_kernel(branch):
    n, restart, cols = 513, 5, 3
    A = step_matrix(str(n))
    s = chosen_state(n, restart, cols, 17)
    s["small"].update({"breakdown": int(branch == "breakdown"), "done": int(branch == "done"), "presid": 0.4 if branch == "relax" else 0.2})
    h = _handle(A)
    h.gmres_set_state(restart, s["x"], s["b"], np.zeros(n), s["rows"], s["small"])
    r0 = np.linalg.norm(s["b"] - A @ s["x"])
    atol = 100.0 * r0 if branch == "converged" else 1e-3 * r0
    st = h.gmres_end_cycle(atol)
    if branch == "done":  # nothing runs behind the done flag
        assert st["done"] and st["cycles"] == 0 and st["cols"] == cols and np.array_equal(h.gmres_get("x"), s["x"])
    elif branch == "converged":
        assert st["done"] and st["converged"] and st["cycles"] == 1 and st["rnorm"] <= atol and st["factor"] == 0.5 and st["ptol"] == 0.3
        assert st["cols"] == cols  # (no restart behind the end)
    elif branch == "breakdown":
        assert st["done"] and not st["converged"] and st["breakdown"] and st["cycles"] == 1 and st["rnorm"] > atol
    else:
        f = 0.75 if branch == "relax" else 0.125
        assert not st["done"] and st["factor"] == f and st["ptol"] == s["small"]["presid"] * min(f, atol / st["rnorm"]) and st["cols"] == 0
    if branch != "done":
        assert h.gmres_end_cycle(atol) == st  # (cols == 0, or done: nothing more to end)
    h.close()


def test_the_first_test_and_the_first_ptol():
    A = step_matrix("csr")
    n = A.shape[0]
    b = np.random.default_rng(4).standard_normal(n)
    bnorm = float(np.linalg.norm(b))
    h = _handle(A)
    h.gmres_begin(5, b)
    st = h.gmres_run(0, 1e-3 * bnorm)
    assert not st["done"] and abs(st["bnorm"] - bnorm) <= 4 * EPS * bnorm and st["rnorm"] == st["bnorm"]
    assert st["ptol"] == st["bnorm"] * min(1.0, 1e-3 * bnorm / st["bnorm"]) and st["factor"] == 1.0
    assert np.array_equal(h.gmres_get("rows")[0, :n], b / st["rnorm"])
    h.gmres_begin(5, b)
    st = h.gmres_run(3, 2.0 * bnorm)  # |r| < atol at once: no step runs
    assert st["done"] and st["converged"] and st["iterations"] == 0 and st["cycles"] == 0 and not np.any(h.gmres_get("x"))
    h.close()


# ---------------------------------------------------------------- d. end to end
@pytest.mark.parametrize("name,rtol,restart,seed", gr.CASES)
def test_end_to_end_on_the_admitted_cases(shared, name, rtol, restart, seed):
    A, b, adm = gr.case(name, rtol, restart, seed)
    host, dev = {}, {}
    xh, ch = gmres(A, b, rtol=rtol, restart=restart, info=host, _backend=NumpyGmresBackend(A))
    x, code = gmres(A, b, rtol=rtol, restart=restart, handle=shared, info=dev)
    assert code == ch == 0 and dev["exit"] == "converged"
    assert (dev["iterations"], dev["cycles"], dev["products"]) == (host["iterations"], host["cycles"], host["products"])
    assert [c["cols"] for c in dev["cycle_history"]] == [c["cols"] for c in host["cycle_history"]]
    assert dev["launches_per_step"] == 11
    op = Operator(A)
    true = float(np.linalg.norm(np.asarray(b.astype(LD) - op.matvec(x), dtype=np.float64)))
    slack = float(np.linalg.norm(product_bound(op, x)))  # what the device's own product may differ from the exact one by
    dist = float(np.linalg.norm(np.asarray(x.astype(LD) - adm["runs"]["longdouble"]["x"], dtype=np.float64)))
    print(f"{name} rtol {rtol:g} restart {restart} seed {seed}: |x - x_longdouble| {dist:.2e}, spread in x {adm['x_spread']:.2e}, "
          f"true residual / atol_eff {true / adm['atol_eff']:.3f}")
    assert dev["residual_norm"] <= adm["atol_eff"] and true <= adm["atol_eff"] + slack
    assert dist <= X_MARGIN * adm["x_spread"]


@pytest.mark.parametrize("name", ["csr", "convdiff", "dense"])
def test_single_steps_equal_one_chunk_across_cycle_ends(name):
    A = step_matrix(name)
    n = A.shape[0]
    b = np.random.default_rng(2).standard_normal(n)
    h = _handle(A)
    h.gmres_begin(5, b)
    for _ in range(13):
        st1 = h.gmres_run(1, 0.0)
    x1, small1, hist1 = h.gmres_get("x"), h.gmres_get("small"), h.gmres_history(13, 2)
    h.gmres_begin(5, b)
    st13 = h.gmres_run(13, 0.0)
    assert st1 == st13 and (st13["iterations"], st13["cycles"], st13["cols"]) == (13, 2, 3)
    assert np.array_equal(h.gmres_get("x"), x1) and np.array_equal(h.gmres_get("small")["R"], small1["R"])
    hist13 = h.gmres_history(13, 2)
    assert np.array_equal(hist1[0], hist13[0]) and np.array_equal(hist1[1], hist13[1]) and np.all(hist1[0] > 0.0)
    ref = NumpyGmresBackend(A)
    ref.begin(5, b, None)
    ref.run(13, 0.0)
    assert np.linalg.norm(x1 - ref.x) <= 1e-12 * np.linalg.norm(ref.x)
    h.close()


@pytest.mark.parametrize("name,rtol,restart,seed", [("convdiff24x20", 1e-10, 20, 0), ("random401", 1e-6, 5, 0), ("skew64", 1e-6, 20, 0),
                                                    ("dense130", 1e-10, 40, 0)])
def test_x_does_not_depend_on_check_every(shared, name, rtol, restart, seed):
    A, b, adm = gr.case(name, rtol, restart, seed)
    runs = []
    for ce in (1, 3, 8, restart, 256):
        info = {}
        x, code = gmres(A, b, rtol=rtol, restart=restart, check_every=ce, handle=shared, info=info)
        runs.append((x, code, info))
    for x, code, info in runs[1:]:
        assert code == runs[0][1] == 0 and np.array_equal(x, runs[0][0])
        assert np.array_equal(info["history"], runs[0][2]["history"]) and info["cycle_history"] == runs[0][2]["cycle_history"]
    assert runs[-1][2]["chunks"] == 1 and np.array_equal(shared.gmres_get("x"), runs[0][0])


def test_breakdown_case_on_the_device(shared):
    A, b = gr.breakdown_case()
    host, dev = {}, {}
    xh, ch = gmres(A, b, rtol=1e-14, restart=10, info=host, _backend=NumpyGmresBackend(A))
    x, code = gmres(A, b, rtol=1e-14, restart=10, handle=shared, info=dev)
    assert code == ch == 0 and (dev["iterations"], dev["cycles"]) == (3, 1) and dev["cycle_history"][0]["cols"] == 3
    assert np.linalg.norm(x - xh) <= 1e-13 * np.linalg.norm(xh)
    x, code = gmres(A, b, rtol=1e-18, restart=10, maxiter=50, handle=shared, info=dev)  # the outer test cannot pass: SciPy bails out
    assert code == 50 and dev["exit"] == "breakdown" and dev["cycles"] == 1 and np.all(np.isfinite(x))


def test_callbacks_x0_and_maxiter_on_the_device(shared):
    A, b, _ = gr.case("convdiff24x20", 1e-10, 5, 0)
    x0 = np.random.default_rng(3).standard_normal(len(b))
    for kw in (dict(callback_type="pr_norm"), dict(callback_type="legacy", maxiter=13), dict(callback_type="x", maxiter=4), dict(maxiter=3)):
        got_h, got_d, host, dev = [], [], {}, {}
        cb_h = {"callback": lambda v: got_h.append(np.copy(v))} if "callback_type" in kw else {}
        cb_d = {"callback": lambda v: got_d.append(np.copy(v))} if "callback_type" in kw else {}
        xh, ch = gmres(A, b, x0, rtol=1e-9, restart=5, info=host, _backend=NumpyGmresBackend(A), **cb_h, **kw)
        x, code = gmres(A, b, x0, rtol=1e-9, restart=5, handle=shared, info=dev, **cb_d, **kw)
        assert code == ch and (dev["iterations"], dev["cycles"], dev["exit"]) == (host["iterations"], host["cycles"], host["exit"])
        assert len(got_d) == len(got_h) and np.linalg.norm(x - xh) <= 1e-12 * np.linalg.norm(xh)
        for a, c in zip(got_d, got_h):
            assert np.allclose(a, c, rtol=1e-6, atol=1e-12)


def test_one_handle_serves_eigs_gmres_bicgstab_with_the_thick_restart_basis_intact():
    A, b, _ = gr.case("convdiff24x20", 1e-6, 5, 0)
    fresh_w = eigs(A, k=4, which="LM", return_eigenvectors=False)
    fresh_x, _ = gmres(A, b, rtol=1e-8)
    fresh_y, _ = bicgstab(A, b, rtol=1e-8)
    h = _capi.Handle(0)
    assert np.array_equal(eigs(A, k=4, which="LM", return_eigenvectors=False, handle=h), fresh_w)
    assert np.array_equal(gmres(A, b, rtol=1e-8, handle=h)[0], fresh_x)
    assert np.array_equal(bicgstab(A, b, rtol=1e-8, handle=h)[0], fresh_y)
    assert np.array_equal(gmres(A, b, rtol=1e-8, handle=h)[0], fresh_x)
    # a thick-restart basis under way and a GMRES solve on the same matrix: neither touches the other
    upload_matrix(h, A)
    h.trl_begin(6, b)
    h.trl_extend(0, 6)
    rows = h.trl_get_rows(0, 7)
    h.gmres_begin(5, b)
    assert h.gmres_run(12, 0.0)["iterations"] == 12
    assert np.array_equal(h.trl_get_rows(0, 7), rows)
    grow = h.gmres_get("rows")
    h.trl_begin(6, b[::-1].copy())
    h.trl_extend(0, 6)
    assert np.array_equal(h.gmres_get("rows"), grow) and h.gmres_run(1, 0.0)["iterations"] == 13
    h.close()


def _begin_without_matrix(h):
    b = np.ones(8)
    h.check(h.lib.lz_gmres_begin(h._h, 4, _capi.dptr(b), None))


def test_state_and_argument_errors():
    A, b, _ = gr.case("random401", 1e-6, 5, 0)
    h = _capi.Handle(0)
    assert status_of(_begin_without_matrix, h) == ERR_STATE  # no matrix
    upload_matrix(h, A)
    assert not h.gmres_info()["live"]
    h._gmres_m = 5
    assert status_of(h.gmres_run, 1, 0.0) == ERR_STATE
    assert status_of(h.gmres_get, "x") == ERR_STATE
    assert status_of(h.gmres_history, 1, 0) == ERR_STATE
    for restart in (0, 129, 402):  # restart out of range (n = 401)
        assert status_of(h.gmres_begin, restart, b) == ERR_ARG
    h.gmres_begin(5, b)
    assert h.gmres_info() == {"launches_per_step": 11, "launches_per_cycle_end": 6, "live": True, "restart": 5}
    assert status_of(h.gmres_step_time, 2) == ERR_STATE  # (nothing has run yet)
    assert h.gmres_run(7, 0.0)["iterations"] == 7
    assert all(t > 0.0 for t in h.gmres_step_time(2))  # (the probe's timer spends the state)
    assert status_of(h.gmres_run, 1, 0.0) == ERR_STATE
    h.gmres_begin(5, b)
    assert status_of(h.gmres_run, -1, 0.0) == ERR_ARG
    assert status_of(h.gmres_run, 1, -1.0) == ERR_ARG
    assert status_of(h.gmres_end_cycle, float("nan")) == ERR_ARG
    upload_matrix(h, A)  # matrix changed: a new matrix drops the state
    assert not h.gmres_info()["live"]
    assert status_of(h.gmres_run, 1, 0.0) == ERR_STATE
    assert status_of(h.gmres_get, "x") == ERR_STATE
    h.set_options(_capi.FLAG_REORTH_PARTIAL)
    assert status_of(h.gmres_begin, 5, b) == ERR_STATE
    h.set_options(0)
    h.set_dense_cplx(np.eye(4, dtype=np.complex128))
    assert status_of(h.gmres_begin, 2, np.ones(4)) == ERR_STATE
    h.close()
    # a handle with a communicator: multi-GPU is refused
    hc = _capi.Handle(0)
    hc.comm_init_host(1, 0, lambda a: None)  # (host callbacks: a communicator without RCCL's start-up)
    csr = sp.csr_matrix(A)
    hc.set_csr(401, 0, csr.indptr.astype(np.int32), csr.indices.astype(np.int32), csr.data)
    assert status_of(hc.gmres_begin, 5, b) == ERR_STATE
    hc.close()
