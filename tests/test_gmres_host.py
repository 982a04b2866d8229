"""``lanczos_amd.gmres`` on the host: ``solve`` driven by ``NumpyGmresBackend`` against SciPy's ``gmres`` and the longdouble loop on
admitted cases (tests/gmres_reference.py), the rules at the edges, the callbacks and every argument error.  No GPU."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla
from scipy.linalg import get_lapack_funcs

import gmres_reference as gr
from lanczos_amd import gmres
from lanczos_amd.gmres import NumpyGmresBackend, lartg

X_MARGIN = 16  # the project's figure (test_bicgstab_host.py): x within this many x_spread of the longdouble x
LD = np.longdouble


def host(A, b, x0=None, **kw):
    info = {}
    x, code = gmres(A, b, x0, _backend=NumpyGmresBackend(A), info=info, **kw)
    return x, code, info


def test_lartg_is_scipys_bit_for_bit():
    ref = get_lapack_funcs("lartg", dtype=np.float64)
    rng = np.random.default_rng(0)
    pairs = [(rng.standard_normal() * 10.0 ** rng.integers(-30, 30), abs(rng.standard_normal()) * 10.0 ** rng.integers(-30, 30)) for _ in range(4000)]
    pairs += [(0.0, 0.0), (0.0, 2.0), (-3.0, 0.0), (1e-200, 1e-210), (-1e-300, 1e-300), (1e200, 3e180), (-1e-170, 1e160)]
    for f, g in pairs:
        assert tuple(float(v) for v in ref(f, g)) == lartg(f, g), (f, g)


@pytest.mark.parametrize("name,rtol,restart,seed", gr.CASES)
def test_every_case_is_admitted(name, rtol, restart, seed):
    _, _, adm = gr.case(name, rtol, restart, seed)
    assert adm["same_stop"] and adm["admitted"], (adm["margin"], adm["spread"])


def test_the_cases_cover_what_the_issue_lists():
    assert len(gr.CASES) == 5 * 2 * 3 * 2
    for name in ("convdiff24x20", "convdiff33x31", "random401", "dense130"):
        for rtol in gr.RTOLS:
            runs = [gr.case(n, t, r, s)[2]["scipy"] for n, t, r, s in gr.CASES if n == name and t == rtol]
            assert all(r["code"] == 0 and r["iterations"] > 20 for r in runs)  # every restart value yields several cycles ...
            assert any(r["cycles"] >= 3 for r in runs)
    assert all(gr.case(n, t, r, s)[2]["scipy"]["iterations"] == 2 for n, t, r, s in gr.CASES if n == "skew64")  # a mid-cycle exit


@pytest.mark.parametrize("name,rtol,restart,seed", gr.CASES)
def test_admitted_case_against_scipy_and_longdouble(name, rtol, restart, seed):
    A, b, adm = gr.case(name, rtol, restart, seed)
    x, code, info = host(A, b, rtol=rtol, restart=restart)
    sc, ld = adm["scipy"], adm["runs"]["longdouble"]
    assert (code, info["iterations"], info["cycles"]) == (sc["code"], sc["iterations"], sc["cycles"])
    assert [c["cols"] for c in info["cycle_history"]] == ld["cols"]
    dist = float(np.linalg.norm(np.asarray(np.asarray(x, dtype=LD) - ld["x"], dtype=np.float64)))
    print(f"|x - x_longdouble| = {dist:.3e}, x_spread = {adm['x_spread']:.3e}")
    assert dist <= X_MARGIN * adm["x_spread"]
    assert info["residual_norm"] <= adm["atol_eff"] == info["atol_effective"]
    assert np.linalg.norm(b - A @ x) <= adm["atol_eff"] * (1 + 1e-6)  # (recomputed in another summation order)
    assert info["exit"] == "converged" and info["products"] == info["iterations"] + info["cycles"]
    np.testing.assert_allclose(info["history"] / np.linalg.norm(b), sc["pr_norm"], rtol=1e-6, atol=1e-3 * rtol)


def test_nonzero_and_all_zero_x0():
    A, b, _ = gr.case("convdiff24x20", 1e-10, 20, 0)
    x0 = np.random.default_rng(9).standard_normal(len(b))
    x, code, info = host(A, b, x0, rtol=1e-10, restart=20)
    sc = gr.scipy_run(A, b, 1e-10, 20, x0=x0)
    assert (code, info["iterations"], info["cycles"]) == (0, sc["iterations"], sc["cycles"])
    assert info["products"] == info["iterations"] + info["cycles"] + 1
    assert np.linalg.norm(x - sc["x"]) <= 1e-12 * np.linalg.norm(sc["x"])
    xz, cz, iz = host(A, b, np.zeros(len(b)), rtol=1e-10, restart=20)
    xn, cn, inn = host(A, b, rtol=1e-10, restart=20)
    assert np.array_equal(xz, xn) and iz["products"] == inn["products"]
    # a guess that already meets the first test: no cycle at all
    xe, ce, ie = host(A, b, x, rtol=1e-6, restart=20)
    assert ce == 0 and ie["iterations"] == 0 and ie["cycles"] == 0 and np.array_equal(xe, x)


def test_restart_edges():
    A, b, _ = gr.case("skew64", 1e-6, 5, 0)
    x, code, info = host(A, b, rtol=1e-8, restart=1000)  # clipped to n = 64
    assert code == 0 and info["iterations"] == 2
    B, c, _ = gr.case("dense130", 1e-6, 5, 0)
    x, code, info = host(B, c, rtol=1e-6, restart=1)
    sc = gr.scipy_run(B, c, 1e-6, 1)
    assert (code, info["iterations"], info["cycles"]) == (sc["code"], sc["iterations"], sc["cycles"])
    assert all(h["cols"] == 1 for h in info["cycle_history"])
    assert np.linalg.norm(x - sc["x"]) <= 1e-10 * np.linalg.norm(sc["x"])
    with pytest.raises(ValueError, match="restart"):
        host(B, c, restart=129)
    with pytest.raises(ValueError, match="restart"):
        host(B, c, restart=0)
    host(B, c, restart=128, maxiter=1)


def test_maxiter_exhausted():
    A, b, adm = gr.case("convdiff33x31", 1e-10, 5, 1)
    x, code, info = host(A, b, rtol=1e-10, restart=5, maxiter=4)
    xs, cs = sla.gmres(A, b, rtol=1e-10, restart=5, maxiter=4)
    assert code == cs == 4 and info["cycles"] == 4 and info["iterations"] == 20 and info["exit"] == "maxiter"
    assert np.linalg.norm(x - xs) <= 1e-12 * np.linalg.norm(xs)
    assert info["residual_norm"] > adm["atol_eff"]


@pytest.mark.parametrize("check_every", [1, 3, 8])
def test_pr_norm_callbacks(check_every):
    A, b, adm = gr.case("random401", 1e-10, 5, 0)
    got = []
    x, code, info = host(A, b, rtol=1e-10, restart=5, callback=got.append, callback_type="pr_norm", check_every=check_every)
    sc = adm["scipy"]
    assert len(got) == sc["iterations"] == info["iterations"]
    np.testing.assert_allclose(got, sc["pr_norm"], rtol=1e-6, atol=1e-13)
    assert np.array_equal(got, info["history"] / np.linalg.norm(b))


def test_x_callbacks():
    A, b, adm = gr.case("random401", 1e-10, 5, 0)
    got, ref = [], []
    x, code, info = host(A, b, rtol=1e-10, restart=5, callback=lambda v: got.append(v.copy()), callback_type="x")
    sla.gmres(A, b, rtol=1e-10, restart=5, callback=lambda v: ref.append(v.copy()), callback_type="x")
    assert len(got) == len(ref) == info["cycles"] == info["chunks"]
    for g, r in zip(got, ref):
        assert np.linalg.norm(g - r) <= 1e-12 * np.linalg.norm(r)
    assert np.array_equal(got[-1], x)


@pytest.mark.parametrize("maxiter", [7, 10, 13, 400])
def test_legacy_callbacks_and_the_mid_cycle_exit(maxiter):
    A, b, adm = gr.case("random401", 1e-10, 5, 0)
    got, ref = [], []
    x, code, info = host(A, b, rtol=1e-10, restart=5, maxiter=maxiter, callback=got.append, callback_type="legacy", check_every=4)
    xs, cs = sla.gmres(A, b, rtol=1e-10, restart=5, maxiter=maxiter, callback=ref.append, callback_type="legacy")
    assert code == cs and len(got) == len(ref) == info["iterations"]
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-13)
    assert np.linalg.norm(x - xs) <= 1e-12 * np.linalg.norm(xs)
    if maxiter < 400:
        assert code == maxiter and info["iterations"] == maxiter
        assert info["cycle_history"][-1]["cols"] == (maxiter % 5 or 5)  # the cycle ended where the count ran out


def test_callback_without_a_type_warns_and_means_legacy():
    A, b, _ = gr.case("random401", 1e-10, 5, 0)
    got = []
    with pytest.warns(DeprecationWarning, match="callback_type"):
        x, code, info = host(A, b, rtol=1e-10, restart=5, maxiter=7, callback=got.append)
    assert code == 7 and len(got) == 7
    with pytest.raises(ValueError, match="Unknown callback_type"):
        host(A, b, callback=got.append, callback_type="residual")
    with pytest.raises(ValueError, match="Unknown callback_type"):
        host(A, b, callback_type="residual")


def test_breakdown():
    A, b = gr.breakdown_case()
    backend, info = NumpyGmresBackend(A), {}
    x, code = gmres(A, b, rtol=1e-14, restart=10, _backend=backend, info=info)
    xs, cs = sla.gmres(A, b, rtol=1e-14, restart=10)
    assert backend.breakdown  # the exit was the breakdown indicator's
    assert code == cs == 0 and info["cycles"] == 1 and info["iterations"] == 3
    assert info["cycle_history"][0]["cols"] == 3 < 10
    assert np.linalg.norm(x - xs) <= 1e-13 * np.linalg.norm(xs)
    # the same breakdown with a tolerance the true residual cannot meet: SciPy bails out with maxiter
    x, code, info = host(A, b, rtol=1e-18, restart=10, maxiter=50)
    xs, cs = sla.gmres(A, b, rtol=1e-18, restart=10, maxiter=50)
    assert code == cs == 50 and info["exit"] == "breakdown" and info["cycles"] == 1


def test_inner_passed_outer_failed_tightens():
    A, b, rtol, restart, maxiter = gr.tighten_case()
    atol_eff = rtol * float(np.linalg.norm(b))
    refs = [gr.loop(A, b, atol_eff, restart, maxiter, order) for order in ("dot", "reversed", "fsum")]
    sc = gr.scipy_run(A, b, rtol, restart, maxiter)
    assert all(r["branches"].count("tighten") >= 2 and (r["cols"], r["branches"]) == (refs[0]["cols"], refs[0]["branches"]) for r in refs)
    x, code, info = host(A, b, rtol=rtol, restart=restart, maxiter=maxiter)
    assert (code, info["iterations"], info["cycles"]) == (sc["code"], sc["iterations"], sc["cycles"]) == (maxiter, refs[0]["iterations"], maxiter)
    ch = info["cycle_history"]
    assert [c["cols"] for c in ch] == refs[0]["cols"]
    # the factor's path, recomputed from what info holds, gives every cycle's ptol exactly
    eps, f, at = float(np.finfo(float).eps), 1.0, 0
    for c, nxt, branch in zip(ch, ch[1:], refs[0]["branches"]):
        at += c["cols"]
        presid = info["history"][at - 1]
        passed = presid <= c["ptol"]
        assert passed == (branch == "tighten")
        f = max(eps, 0.25 * f) if passed else min(1.0, 1.5 * f)
        assert nxt["ptol"] == presid * min(f, atol_eff / c["rnorm"])


@pytest.mark.parametrize("name,rtol,restart,seed", [("convdiff24x20", 1e-10, 20, 0), ("dense130", 1e-6, 5, 0), ("skew64", 1e-6, 20, 0)])
def test_x_does_not_depend_on_check_every(name, rtol, restart, seed):
    A, b, _ = gr.case(name, rtol, restart, seed)
    runs = [host(A, b, rtol=rtol, restart=restart, check_every=ce) for ce in (1, 3, 8, restart)]
    for x, code, info in runs[1:]:
        assert np.array_equal(x, runs[0][0]) and code == runs[0][1]
        assert (info["iterations"], info["cycles"]) == (runs[0][2]["iterations"], runs[0][2]["cycles"])
    assert runs[0][2]["chunks"] > runs[2][2]["chunks"]


def test_zero_b_and_n_equal_one():
    A, b, _ = gr.case("dense130", 1e-6, 5, 0)
    x, code, info = host(A, np.zeros(130))
    assert code == 0 and not x.any() and info["iterations"] == 0
    x, code = gmres(np.array([[4.0]]), np.array([2.0]))  # answered on the host: no device is asked for
    assert code == 0 and x.tolist() == [0.5]


def test_argument_errors():
    A, b, _ = gr.case("dense130", 1e-6, 5, 0)
    with pytest.raises(NotImplementedError, match="gmres"):
        gmres(A, b, M=np.eye(130))
    with pytest.raises(NotImplementedError):
        gmres(A.astype(complex), b)
    with pytest.raises(NotImplementedError):
        gmres(A, b.astype(complex))
    with pytest.raises(NotImplementedError):
        gmres(A, b, x0=b.astype(complex))
    with pytest.raises(NotImplementedError):
        gmres(sla.aslinearoperator(A), b)
    for bad in (dict(A=np.ones((3, 4)), b=np.ones(3)), dict(A=A, b=np.ones(129)), dict(A=A, b=b, x0=np.ones(131)), dict(A=A, b=b, maxiter=-1),
                dict(A=A, b=b, check_every=0), dict(A=A, b=b, rtol=-1.0), dict(A=A, b=b, atol=-1.0), dict(A=np.ones(4), b=np.ones(4)),
                dict(A=sp.csr_matrix((0, 0)), b=np.ones(0))):
        with pytest.raises(ValueError):
            gmres(bad.pop("A"), bad.pop("b"), **bad)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x, code = gmres(A, b.reshape(130, 1), rtol=1e-6, _backend=NumpyGmresBackend(A))  # (n, 1) is accepted, and no warning without a callback
    assert code == 0 and x.shape == (130,)
