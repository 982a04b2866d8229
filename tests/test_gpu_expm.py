"""``expm_multiply`` on the device: the product of a real matrix with a planar complex vector in both of its forms against clongdouble
(tests/hermitian_reference.py), ``lz_expm_extend`` / ``lz_expm_combine`` step by step against ``NumpyExpmBackend`` on the device's own
rows, the function end to end on every route at the host tests' bars (tests/test_expm_host.py: ``|out - exact| <= tol |exact|``), and
the life of a handle that serves ``eigsh`` and ``expm_multiply`` in turn."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from expm_reference import exact, matrix, rel_errors, vector
from hermitian_reference import matvec, product_bound, worst
from test_gpu_eigsh_complex import product_matrix

from lanczos_amd import StencilOperator, _capi, eigsh, expm_multiply, synthetic
from lanczos_amd.eigsh import upload_complex_matrix, upload_matrix
from lanczos_amd.expm import NumpyExpmBackend

pytestmark = pytest.mark.gpu

FORMS = {1: "two-launch", 2: "two-plane"}


def _handle(A, knob=0):
    h = _capi.Handle(0)
    h.expm_set_product(knob)
    (upload_complex_matrix if np.iscomplexobj(A) else upload_matrix)(h, A)
    return h


def status_of(call, *args):
    with pytest.raises(_capi.LanczosHipError) as e:
        call(*args)
    return e.value.status


# ---------------------------------------------------------------- a. the mixed product alone
def _check_product(h, A, label, form):
    n = A.shape[0]
    rng = np.random.default_rng(n)
    for trial in range(2):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        y = h.zspmv_real(x)
        ref = matvec(A, x)
        err = np.abs(np.asarray(y - ref, dtype=np.complex128))
        bound = product_bound(A, x)
        print(f"{label:24s} {form:10s} trial {trial}: worst error / bound {worst(err, bound):.2e}")
        assert np.all(np.isfinite(y.view(np.float64)))
        assert worst(err, bound) <= 1.0
    assert h.expm_info()["product"] == form


@functools.lru_cache(maxsize=None)
def real_part(name):
    A = sp.csr_matrix(product_matrix(name).real)
    A.sort_indices()
    return A


@pytest.mark.parametrize("knob", [1, 2], ids=["two_launch", "two_plane"])
@pytest.mark.parametrize("name", ["hofstadter", "ragged1000", "band70001", "n5"])
def test_csr_product_against_clongdouble(name, knob):
    A = real_part(name)
    h = _handle(A, knob)
    _check_product(h, A, name, FORMS[knob])
    if name == "ragged1000":  # an empty row gives an exact zero in both planes
        y = h.zspmv_real(np.ones(1000) + 1j)
        assert np.all(y[[0, 123, 500, 501, 999]] == 0.0)
        assert np.diff(A.indptr).max() >= 300
    h.close()


@functools.lru_cache(maxsize=None)
def symmetric333(per_row):
    """a random symmetric pattern on n = 333 with ``2 (per_row n // 2 + 10)`` entries, none on the diagonal"""
    n = 333
    rng = np.random.default_rng(per_row)
    iu = np.triu_indices(n, 1)
    pick = rng.choice(len(iu[0]), per_row * n // 2 + 10, replace=False)
    U = sp.csr_matrix((rng.standard_normal(len(pick)), (iu[0][pick], iu[1][pick])), shape=(n, n))
    A = sp.csr_matrix(U + U.T)
    A.sort_indices()
    return A


@pytest.mark.parametrize("knob", [0, 1, 2], ids=["auto", "two_launch", "two_plane"])
@pytest.mark.parametrize("per_row,group", [(1, 1), (2, 2), (4, 4), (9, 8), (17, 16), (33, 32), (70, 64)])
def test_csr_product_at_every_group_width(per_row, group, knob):
    """the widest power of two that the mean row still fills, as ``lz_set_csr_cplx`` chooses it: every instance of the kernel.  Left
    to itself the library takes the two-plane kernel up to groups of 8 lanes and two launches from 16 on"""
    A = symmetric333(per_row)
    assert group <= A.nnz / 333 < 2 * group or group == 64
    h = _handle(A, knob)
    assert h.expm_info()["group"] == group
    _check_product(h, A, f"n333 {per_row}/row G={group}", FORMS[knob or (2 if group <= 8 else 1)])
    h.close()


@pytest.mark.parametrize("knob", [0, 1], ids=["auto", "two_launch"])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 320, 511, 512, 513, 640])
def test_dense_product_against_clongdouble(n, knob):
    """the edges of the unrolled loop (four 16-byte loads of 64 lanes: 512 columns), of its tail (128 columns) and the odd last column;
    a dense matrix takes the two-plane kernel unless the knob says otherwise"""
    rng = np.random.default_rng(n + 11)
    G = rng.standard_normal((n, n))
    A = np.ascontiguousarray(G + G.T)
    h = _handle(A, knob)
    _check_product(h, A, f"dense {n}", FORMS[knob or 2])
    h.close()


# ---------------------------------------------------------------- b. extend and combine against NumpyExpmBackend
@functools.lru_cache(maxsize=None)
def hof(route):
    H = synthetic.hofstadter(24, 17, 1 / 8)
    if route == "complex":
        return H
    A = sp.csr_matrix(H.real)
    A.sort_indices()
    return A


@pytest.mark.parametrize("m", [2, 12, 64])
@pytest.mark.parametrize("route", ["real", "mixed", "complex"])
def test_extend_and_combine_against_numpy(route, m):
    A = hof(route)
    n = A.shape[0]
    cplx = route != "real"
    anorm = abs(A).sum(axis=1).max()
    v0 = vector(n, cplx, seed=m)
    for ncols in sorted({1, 3, m - 1} & set(range(1, m))):
        h = _handle(A)
        h.expm_begin(m, v0, cplx)
        assert h.expm_info()["route"] == route
        if m > 5:
            first, _ = h.expm_extend(0, 5)
            proj, beta = h.expm_extend(5, m)
            assert np.array_equal(proj[:5], first[:5]) and not np.any(first[5:])
        else:
            proj, beta = h.expm_extend(0, m)
        rows = h.expm_get_rows(0, m + 1)
        # every step again in NumPy from the device's own rows: no step inherits another's rounding
        ref = NumpyExpmBackend(A, cplx)
        ref.begin(m, v0)
        assert np.abs(rows[0] - ref.V[0]).max() <= 2e-14  # (n + 2) eps |v_i|: the norm in another summation order
        worst_proj = worst_beta = worst_row = 0.0
        for j in range(m):
            ref.V[: j + 1] = rows[: j + 1]
            p, b = ref.extend(j, j + 1)
            worst_proj = max(worst_proj, np.abs(p[j, : j + 1] - proj[j, : j + 1]).max())
            worst_beta = max(worst_beta, abs(b[j] - beta[j]))
            worst_row = max(worst_row, np.linalg.norm(ref.V[j + 1] - rows[j + 1]) * beta[j] / anorm)
        gram = np.abs(rows.conj() @ rows.T - np.eye(m + 1)).max()
        print(f"{route} m={m}: proj {worst_proj / anorm:.2e} beta {worst_beta / anorm:.2e} row {worst_row:.2e} (in |A|), |V V^H - I| {gram:.2e}")
        assert worst_proj <= 1e-12 * anorm and worst_beta <= 1e-12 * anorm and worst_row <= 1e-12
        assert gram <= 1e-12
        # combine: the same rotation in NumPy on the device's rows
        rng = np.random.default_rng(100 * m + ncols)
        C = rng.standard_normal((m, ncols)) + (1j * rng.standard_normal((m, ncols)) if cplx else 0.0)
        ref.V[:] = rows
        want = ref.combine(m, C)
        norm = h.expm_combine(m, C)
        got = h.expm_get_rows(0, ncols)
        assert abs(norm - ref.state_norm) <= 1e-13 * ref.state_norm
        assert abs(np.linalg.norm(got[0]) - 1.0) <= 1e-14
        assert np.linalg.norm(got[0] - ref.V[0]) <= 1e-12
        for c in range(1, ncols):
            assert np.linalg.norm(got[c] - want[c - 1]) <= 1e-12 * np.linalg.norm(want[c - 1])
        h.close()


def path_matrix(n=40):
    """nodes 0 - 1 - 2 form a path that nothing else touches: from e_0 the Krylov space is exactly three-dimensional, every number of
    its three Lanczos steps is exact in floating point and the fourth residual is an exact zero"""
    rng = np.random.default_rng(3)
    R = sp.random(n - 3, n - 3, density=0.2, random_state=rng, format="csr")
    A = sp.block_diag([sp.csr_matrix(np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0]])), R + R.T + sp.identity(n - 3)]).tocsr()
    A.sort_indices()
    return A


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "mixed"])
def test_combine_reads_no_row_behind_a_breakdown(cplx):
    A = path_matrix()
    n = A.shape[0]
    v0 = np.zeros(n, dtype=np.complex128 if cplx else np.float64)
    v0[0] = 1j if cplx else 1.0
    h = _handle(A)
    h.expm_begin(6, v0, cplx)
    proj, beta = h.expm_extend(0, 6)
    assert beta[0] == 1.0 and beta[1] == 1.0 and beta[2] == 0.0
    rows = h.expm_get_rows(0, 7)
    assert np.all(np.isfinite(rows[:3].view(np.float64))) and np.all(np.isnan(rows[3:, :n].view(np.float64)))  # 0 / 0 behind the vanished residual
    C = np.array([[0.5, 2.0], [-1.0, 0.25], [3.0, 1.0]]) * (1j if cplx else 1.0)
    norm = h.expm_combine(3, C)
    got = h.expm_get_rows(0, 2)
    want = C.T @ rows[:3]
    assert np.isfinite(norm) and np.all(np.isfinite(got.view(np.float64)))
    assert abs(norm - np.linalg.norm(want[0])) <= 1e-14 * norm
    assert np.abs(got[0] * norm - want[0]).max() <= 1e-14 * norm and np.abs(got[1] - want[1]).max() <= 1e-14 * np.abs(want[1]).max()
    # ... and the next extension starts from clean rows
    proj, beta = h.expm_extend(0, 3)
    assert np.all(np.isfinite(proj[:3].view(np.float64))) and np.all(np.isfinite(beta[:3]))
    h.close()
    # the function itself on that start vector: every substep is truncated to three rows and exact
    info = {}
    out = expm_multiply(A, v0, start=1.0, stop=7.0, num=4, a=-1.0 if not cplx else -1j, ncv=6, tol=1e-10, info=info)
    ref = exact(A, v0, -1.0 if not cplx else -1j, np.linspace(1.0, 7.0, 4))
    assert info["substeps"] == 2 and info["err_est"] == 0.0
    assert np.all(rel_errors(out, ref) <= 1e-12)


def test_one_row_is_scaled():
    """mm = 1: the start vector is an eigenvector"""
    A = sp.csr_matrix(sp.diags(np.arange(1.0, 41.0)))
    v0 = np.zeros(40, dtype=np.complex128)
    v0[4] = 2.0
    h = _handle(A)
    h.expm_begin(5, v0, True)
    proj, beta = h.expm_extend(0, 5)
    assert proj[0, 0] == 5.0 and beta[0] == 0.0
    norm = h.expm_combine(1, np.array([[3.0 - 4.0j]]))
    row = h.expm_get_rows(0, 1)[0]
    assert abs(norm - 5.0) <= 1e-15 and abs(row[4] - (0.6 - 0.8j)) <= 1e-15 and not np.any(np.delete(row, 4))
    assert status_of(h.expm_combine, 1, np.ones((1, 2), dtype=complex)) == -1
    h.close()
    out = expm_multiply(A, v0, start=0.5, stop=1.5, num=3, a=-1j, ncv=5)
    assert np.all(rel_errors(out, exact(A, v0, -1j, [0.5, 1.0, 1.5])) <= 1e-14)


# ---------------------------------------------------------------- c. end to end
def _stencil(dims):
    return StencilOperator(dims, 7)


E2E = {  # name: (matrix, a, complex b, route, product)
    "real_csr": (lambda: matrix("lap20"), -1.0, False, "real", None),
    "mixed_csr": (lambda: hof("mixed"), -1j, False, "mixed", "two-plane"),
    "mixed_dense": (lambda: matrix("dense96"), -1j, True, "mixed", "two-plane"),
    "mixed_coded_laplacian": (lambda: matrix("lap20"), -1j, False, "mixed", "two-launch"),
    "mixed_stencil_operator": (lambda: _stencil((9, 8, 7)), -1j, True, "mixed", "two-launch"),
    "complex_csr": (lambda: matrix("hof24x17"), -1j, True, "complex", None),
    "complex_heat": (lambda: matrix("hof24x17"), -1.0, False, "complex", None),
}


@pytest.mark.parametrize("tol", [1e-8, 1e-11])
@pytest.mark.parametrize("name", list(E2E))
def test_expm_multiply_end_to_end(name, tol):
    make, a, cplx_b, route, product = E2E[name]
    A = make()
    n = A.shape[0]
    b = vector(n, cplx_b)
    times = np.linspace(0.0, 3.0, 4)
    info = {}
    out = expm_multiply(A, b, start=0.0, stop=3.0, num=4, a=a, tol=tol, info=info)
    ref = exact(A, b, a, times)
    err = rel_errors(out, ref)
    print(f"{name} tol={tol:g}: worst error / tol {err.max() / tol:.3f}, substeps {info['substeps']}, product {info['product']}")
    assert out.shape == (4, n) and out.dtype == (np.float64 if route == "real" else np.complex128)
    assert np.all(err <= tol)
    assert info["route"] == route and info["product"] == product and info["ncv"] == 30 and info["matvecs"] == 30 * info["substeps"]
    if a == -1j:
        nb = np.linalg.norm(b)
        assert np.all(np.abs(np.linalg.norm(out, axis=1) - nb) <= tol * nb)


def test_the_chosen_form_changes_the_product_not_the_answer():
    A, b = hof("mixed"), vector(408, True)
    ref = exact(A, b, -1j, [2.0])
    for knob, form in FORMS.items():
        h = _capi.Handle(0)
        h.expm_set_product(knob)
        info = {}
        out = expm_multiply(A, b, start=2.0, stop=2.0, num=1, a=-1j, tol=1e-11, handle=h, info=info)
        assert info["product"] == form and rel_errors(out, ref)[0] <= 1e-11
        h.close()


# ---------------------------------------------------------------- d. the life of a handle
def test_a_handle_serves_eigsh_and_expm_in_turn():
    """(the complex matrix carries disorder: the clean lattice's band edge is a cluster of levels 1e-6 apart, on which ``eigsh`` at its
    default ``ncv`` and ``tol`` runs out of cycles on either backend - nothing this test is about)"""
    L, H = matrix("lap20"), synthetic.hofstadter(24, 17, 1 / 8, disorder=2.0, seed=1)
    lamL, lamH = np.linalg.eigvalsh(L.toarray()), np.linalg.eigvalsh(H.toarray())
    bL, bH = vector(400, False), vector(408, True)
    h = _capi.Handle(0)
    w = eigsh(L, k=3, which="LA", return_eigenvectors=False, handle=h)
    assert np.abs(w - lamL[-3:]).max() <= 1e-10 * 8
    info = {}
    out = expm_multiply(L, bL, start=0.5, stop=2.0, num=2, a=-1j, tol=1e-10, handle=h, info=info)
    assert info["route"] == "mixed" and np.all(rel_errors(out, exact(L, bL, -1j, [0.5, 2.0])) <= 1e-10)
    w = eigsh(H, k=3, which="SA", return_eigenvectors=False, handle=h)
    assert np.abs(w - lamH[:3]).max() <= 1e-10 * 6
    out = expm_multiply(H, bH, start=0.5, stop=2.0, num=2, a=-1j, tol=1e-10, handle=h, info=info)
    assert info["route"] == "complex" and np.all(rel_errors(out, exact(H, bH, -1j, [0.5, 2.0])) <= 1e-10)
    w = eigsh(L, k=3, which="LA", return_eigenvectors=False, handle=h)
    assert np.abs(w - lamL[-3:]).max() <= 1e-10 * 8
    out = expm_multiply(L, bL, a=-1.0, tol=1e-10, handle=h, info=info)
    assert info["route"] == "real" and rel_errors(out, exact(L, bL, -1.0, [1.0]))[0] <= 1e-10
    h.close()


def test_state_checks():
    L, H, D = matrix("lap20"), matrix("hof24x17"), matrix("dense96")
    h = _capi.Handle(0)
    h.expm_m, h.expm_cplx, h.rows = 12, True, 400
    assert status_of(h.expm_begin, 12, np.ones(400), True) == -4  # no matrix set
    upload_matrix(h, L)
    assert status_of(h.expm_extend, 0, 12) == -4  # before begin
    assert status_of(h.expm_combine, 12, np.ones((12, 1))) == -4
    assert status_of(h.expm_get_rows, 0, 1) == -4
    assert status_of(h.expm_begin, 65, np.ones(400), True) == -1
    assert status_of(h.expm_begin, 1, np.ones(400), True) == -1
    h.expm_begin(12, np.ones(400), True)
    assert status_of(h.expm_extend, 0, 13) == -1 and status_of(h.expm_extend, 3, 3) == -1
    h.expm_extend(0, 12)
    assert status_of(h.expm_combine, 12, np.ones((12, 12))) == -1  # ncols < mm
    # the complex solver's state is its own: a real matrix and the propagator's planar basis do not open it
    assert status_of(h.ztrl_extend, 0, 12) == -4
    assert status_of(h.zspmv, np.ones(400)) == -4
    upload_matrix(h, D)  # another row length
    assert status_of(h.expm_extend, 0, 12) == -4
    upload_matrix(h, L)  # the old length again: the basis is still there
    h.expm_extend(0, 12)
    upload_complex_matrix(h, H)
    assert status_of(h.zspmv_real, np.ones(408)) == -4  # no real matrix
    assert status_of(h.expm_begin, 12, np.ones(408), False) == -1  # a complex matrix needs the planar basis
    h.expm_begin(12, np.ones(408), True)
    assert h.expm_info()["route"] == "complex"
    upload_matrix(h, L)
    h.expm_begin(12, np.ones(400), False)
    assert h.expm_info()["route"] == "real"
    assert status_of(h.expm_set_product, 3) == -1 and status_of(h.expm_set_product, -1) == -1
    h.set_options(_capi.FLAG_REORTH_PARTIAL)
    assert status_of(h.expm_begin, 12, np.ones(400), False) == -4
    h.close()
