"""Products on CSR as stored: rows that are unsorted, hold unsummed duplicates and explicit zeros (tests/noncanonical_reference.py) on
every kernel that walks a CSR row.  The real square product is held to SciPy's ``B @ x`` bit for bit wherever tests/test_gpu_kernels.py
holds canonical input to it, and to the longdouble sum of the STORED entries within its forward bound everywhere; every case asserts the
plan and the coding it ran on.  The other row walks (complex, planar, residuals, quality, rectangular), one solver iteration from an
uploaded state and the functions end to end run the same matrices against the references and bars their own tests use."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from bicgstab_reference import dot_bound, worst
from noncanonical_reference import (LD, T_CLS_GROUP, T_FIXED_LAYOUT, T_FIXED_ROWS, T_PB_ENTRIES, T_SPMV_PLAN, SCALAR, STREAM, class_count,
                                    diagonal_position, product_cases, as_stored, stored_abs, stored_product, stored_sum_float64, trimmed, untouched, arrays_of,
                                    x_of, _canonical)

from lanczos_amd import _capi

pytestmark = pytest.mark.gpu

CASES = product_cases()


def test_the_registry_names_the_library_s_knobs(hip):
    assert (SCALAR, STREAM) == (hip.FLAG_SPMV_SCALAR, hip.FLAG_SPMV_STREAM)
    assert (T_FIXED_ROWS, T_PB_ENTRIES, T_SPMV_PLAN, T_FIXED_LAYOUT, T_CLS_GROUP) == (hip.TUNE_FIXED_ROWS, hip.TUNE_PB_ENTRIES, hip.TUNE_SPMV_PLAN,
                                                                                      hip.TUNE_FIXED_LAYOUT, hip.TUNE_CLS_GROUP)


def _err(a, b):
    return np.abs(np.asarray(a - b, dtype=np.float64))


# ---------------------------------------------------------------- a. the real square product
@pytest.mark.parametrize("name", list(CASES))
def test_product_as_stored(hip, name):
    """``spmv_host`` and ``step_spmv`` (the product with its ``x . y`` epilogue): SciPy's bits where the plan is bit-exact - everywhere
    but, on the CSR-stream kernel, a row longer than its tile, which a whole block sums (test_spmv_bit_exact's rule) -, the longdouble sum
    of the stored entries within ``stored_product``'s bound everywhere, ``x . y`` within ``dot_bound``, a zero pad, the same bits twice"""
    case = CASES[name]
    B = case["build"]()
    before = arrays_of(B)
    n = B.shape[0]
    x = x_of(B)
    ref = B @ x
    assert np.array_equal(stored_sum_float64(B, x), ref)
    exact, bound = stored_product(B, x)
    h = hip.Handle(0)
    for index, value in case["tune"]:
        h.set_tuning(index, value)
    h.set_options(case["flags"])
    h.set_csr(n, 0, B.indptr, B.indices, B.data)  # the caller's arrays, as they are (``padded``: longer than indptr[-1])
    kind, ncls = h.spmv_coding()
    assert h.spmv_plan() == case["plan"] and kind in case["coding"], (h.spmv_plan(), kind, ncls)
    if case["classes"] is not None:
        assert ncls == class_count(B, *case["classes"]), ncls
        assert np.mean(diagonal_position(B) != diagonal_position(_canonical(B))) > 0.5  # the diagonal is not where sorting would put it
    else:
        assert ncls == 0 or name == "lap2d_37x29_k7_repeated_offset"
    if name == "lap3d_21x17x13_rows_shuffled_apart":
        assert class_count(B, False) > 256
    # a row beyond the CSR-stream tile (2048 entries when rows average >= 12 entries, else 4096) is summed by a whole block
    cap = 2048 if B.nnz / n >= 12 else 4096
    loose = (np.diff(B.indptr) > cap) if case["plan"] == "csr-stream" else np.zeros(n, dtype=bool)
    assert loose.sum() == (1 if name == "long_row_3000" else 0)
    got = []
    for _ in range(2):
        y = h.spmv_host(x)
        assert np.array_equal(y[~loose], ref[~loose]), (np.flatnonzero(y != ref)[:8], _err(y, ref).max())
        got.append(y)
    assert np.array_equal(got[0], got[1])
    h.basis_alloc(3)
    h.basis_set_row(1, x)
    alpha = h.step_spmv(1)
    r = h.r_get()
    assert np.array_equal(r[~loose], ref[~loose]) and np.array_equal(r, got[0])
    assert h.step_spmv(1) == alpha and np.array_equal(h.r_get(), r)
    alpha_exact = np.sum(x.astype(LD) * exact)
    figures = {"y": worst(_err(got[0], exact), bound), "r": worst(_err(r, exact), bound),
               "x.y": worst([abs(float(alpha - alpha_exact))], [dot_bound(x, exact, db=bound)])}
    # the pad: cg's first iteration forms q = A p with p = r = b = x into a padded vector
    h.cg_begin(x)
    h.cg_run(1, 0.0)
    q = h.cg_get("q", raw=True)
    assert np.array_equal(q[:n], got[0]) and not np.any(q[n:]) and len(q) == h.padded_rows(n)
    print(f"{name:44s} {case['plan']:10s} {kind} ({ncls})  error / bound: " + "  ".join(f"{key} {val:.2e}" for key, val in figures.items()))
    for key, val in figures.items():
        assert val <= 1.0, key
    rowptr, colidx, vals = h.get_csr()  # the three arrays exactly as uploaded
    T = trimmed(B)
    assert np.array_equal(rowptr, T.indptr) and np.array_equal(colidx, T.indices) and vals.tobytes() == T.data.tobytes()
    h.close()
    assert untouched(B, before)


# ---------------------------------------------------------------- b. the other CSR walks
import hermitian_reference as hr  # noqa: E402
import ritz_reference as rr  # noqa: E402
import test_gpu_eigs as t_eigs  # noqa: E402  (modules, not names: their tests are collected where they live)
import test_gpu_eigsh_complex as t_zeigsh  # noqa: E402
import test_gpu_expm as t_expm  # noqa: E402
import test_gpu_ritz_exact as t_ritz  # noqa: E402
from noncanonical_reference import noncanonical, noncanonical_hermitian, reshuffled, stencil, sym_random  # noqa: E402
from test_gpu_svds import EPS  # noqa: E402

SIZES = (257, 1000)


@pytest.fixture(autouse=True)
def shared_matrices_stay_as_built():
    """the matrices are built once and shared: no test, reference or library call may leave one sorted, summed or trimmed"""
    yield
    for cache in (real_matrix, hermitian_matrix, step_matrices):
        for B, before in _SNAPSHOTS.get(cache.__name__, []):
            assert untouched(B, before), cache.__name__


_SNAPSHOTS = {}


def _shared(name, B):
    _SNAPSHOTS.setdefault(name, []).append((B, arrays_of(B)))
    return B


@functools.lru_cache(maxsize=None)
def real_matrix(n, padded=False):
    return _shared("real_matrix", noncanonical(sym_random(n), seed=n, padded=padded))


@functools.lru_cache(maxsize=None)
def hermitian_matrix(n, padded=False):
    rng = np.random.default_rng(n)
    G = sp.random(n, n, density=3.0 / n, random_state=rng, data_rvs=rng.standard_normal) + 1j * sp.random(n, n, density=3.0 / n, random_state=rng,
                                                                                                          data_rvs=rng.standard_normal)
    return _shared("hermitian_matrix", noncanonical_hermitian((G + G.getH() + sp.diags(rng.standard_normal(n))).tocsr(), seed=n, padded=padded))


@pytest.mark.parametrize("padded", [False, True], ids=["exact_length", "padded"])
@pytest.mark.parametrize("n", SIZES)
def test_complex_product_as_stored(n, padded):
    """``k_zspmv_csr`` (``set_csr_cplx`` + ``zspmv``) against clongdouble at ``hermitian_reference.product_bound``"""
    Z = hermitian_matrix(n, padded)
    h = _capi.Handle(0)
    h.set_csr_cplx(n, Z.indptr, Z.indices, Z.data)
    t_zeigsh._check_product(h, trimmed(Z), f"hermitian {n}")
    h.close()


@pytest.mark.parametrize("knob", [1, 2], ids=["two_launch", "two_plane"])
@pytest.mark.parametrize("n", SIZES)
def test_planar_product_as_stored(n, knob):
    """``k_spmv_csr_z2`` (a real matrix times a planar complex vector, ``zspmv_real``) in both forms: the reference and bar of
    test_gpu_expm.py::test_csr_product_against_clongdouble"""
    B = real_matrix(n)
    h = t_expm._handle(B, knob)
    t_expm._check_product(h, B, f"real {n}", t_expm.FORMS[knob])
    h.close()


@pytest.mark.parametrize("n", SIZES)
def test_residual_kernels_as_stored(n):
    """``k_trl_resid_csr`` and ``k_trl_resid_cplx_csr``: test_gpu_eigs.py's patterns, reference and bound, fed the stored entries"""
    B = real_matrix(n)
    h = _capi.Handle(0)
    h.set_csr(n, 0, B.indptr, B.indices, B.data)
    assert h.spmv_plan() == "csr-stream"
    h.trl_begin(t_eigs.M_TRL, np.ones(n))
    t_eigs._check_patterns(h, B, n, n + 1)
    h.close()


@pytest.mark.parametrize("n", SIZES)
def test_complex_residuals_as_stored(n):
    """``lz_ztrl_residuals``: ``|A y_i - theta_i y_i|`` of rows set from the host, against clongdouble.  The bound: the product row errs
    by ``hermitian_reference.product_bound``; ``theta y`` and the difference by ``2 eps (|A y| + |theta y|)`` more; the norm of ``n``
    complex terms by ``gamma(2 n)`` of itself and one rounding of the root"""
    Z = trimmed(hermitian_matrix(n))
    h = _capi.Handle(0)
    h.set_csr_cplx(n, Z.indptr, Z.indices, Z.data)
    k = 4
    h.ztrl_begin(8, np.ones(n))
    rng = np.random.default_rng(n + 2)
    Y = rng.standard_normal((k, n)) + 1j * rng.standard_normal((k, n))
    theta = rng.uniform(-2.0, 2.0, k)
    h.ztrl_set_rows(0, Y)
    got = h.ztrl_residuals(k, theta)
    for i in range(k):
        t = hr.matvec(Z, Y[i]) - hr.LD(theta[i]) * Y[i].astype(hr.CLD)
        ref = float(np.sqrt(np.sum(np.abs(t) ** 2)))
        entry = hr.product_bound(Z, Y[i]) + 2.0 * EPS * (np.abs(np.asarray(hr.matvec(Z, Y[i]), dtype=np.complex128)) + abs(theta[i]) * np.abs(Y[i]))
        bound = float(np.linalg.norm(entry)) + (2.0 * n + 2.0) * EPS * ref
        print(f"hermitian {n} row {i}: residual {ref:.3e}, error / bound {abs(got[i] - ref) / bound:.2e}")
        assert abs(got[i] - ref) <= bound
    assert np.array_equal(h.ztrl_residuals(k, theta), got) and np.array_equal(h.ztrl_get_rows(0, k), Y)
    h.close()


@pytest.mark.parametrize("rows", SIZES)
def test_quality_kernel_as_stored(rows):
    """``k_ritz_quality`` on an integer matrix (tests/ritz_reference.py's ragged one) split, zero-filled and shuffled with integers:
    test_gpu_ritz_exact.py's exact case - the same bits as the integer sums of the stored entries"""
    B = noncanonical(rr.quality_matrix("ragged", rows), seed=rows, integer=True)
    assert np.array_equal(B.data, np.rint(B.data)) and not B.has_canonical_format
    h = _capi.Handle(0)
    h.set_csr(rows, 0, B.indptr, B.indices, B.data)
    for width in (1, 17):
        t_ritz.quality_case(h, as_stored(B), width, rows, [(0, 0), (0, 1)])  # (quality_exact calls SciPy's abs())
    h.close()


def test_filter_steps_fused_and_unfused_as_stored():
    """the Chebyshev filter's and the series' step as the coded kernel's epilogue and as SpMV + step kernel
    (``FLAG_TRL_FILTER_UNFUSED``) on the ``same_order`` stencil: the same bits, as
    test_gpu_kernels.py::test_filter_steps_fused_into_the_27_entry_class_table asks of sorted rows"""
    from lanczos_amd.eigsh import ChebFilter, SeriesFilter

    for name, coding in (("lap2d_37x29_same_order_g0", "offsets+values"), ("lap3d_21x17x13_potential_same_order_g0", "offsets+values, diagonal streamed")):
        B = CASES[name]["build"]()
        n = B.shape[0]
        nrm = float(stored_abs(B).sum(axis=1).max())
        f, s = ChebFilter(-nrm, 0.5 * nrm, 1.5 * nrm, 4), SeriesFilter(-nrm, nrm, 0.1 * nrm, 5)
        x = np.random.default_rng(2).uniform(-1, 1, n)
        out = []
        for flags in (0, _capi.FLAG_TRL_FILTER_UNFUSED):
            h = _capi.Handle(0)
            h.set_options(flags)
            h.set_csr(n, 0, B.indptr, B.indices, B.data)
            assert h.spmv_coding()[0] == coding
            h.trl_begin(8, x)
            h.trl_set_filter(f.coefficients(), f.c)
            yf = h.trl_filter_apply(x)
            h.trl_set_series(s.coefficients(), s.c, s.e)
            out.append((yf, h.trl_filter_apply(x)))
            h.close()
        for fused, unfused in zip(*out):
            assert np.isfinite(fused).all() and np.abs(fused).max() > 0
            assert np.array_equal(fused, unfused)


@pytest.mark.parametrize("transpose", [False, True])
def test_rectangular_product_as_stored(transpose):
    """``gk_set_csr(A, AT)`` + ``gk_spmv`` (``k_spmv_rect``, ``k_spmv_rect_fold``) with both matrices non-canonical - ``svds`` itself
    canonicalises, the raw call does not: test_gpu_svds.py::test_rectangular_product's bar, SciPy's bits included"""
    rng = np.random.default_rng(13)
    W = noncanonical(sp.random(1000, 4099, density=8.0 / 1000, random_state=rng, data_rvs=rng.standard_normal), seed=13)
    T = reshuffled(W.T.tocsr(), 14)  # the tall orientation, its rows in yet another order
    assert T.shape == (4099, 1000) and T.nnz == W.nnz and not T.has_sorted_indices and not W.has_sorted_indices
    h = _capi.Handle(0)
    h.gk_set_csr(T, W)
    B = W if transpose else T
    rows, cols = B.shape
    x = np.random.default_rng(rows).standard_normal(cols)
    y = h.gk_spmv(x, transpose=transpose)
    assert y.shape == (h.padded_rows(rows),) and not np.any(y[rows:])
    ref = B @ x
    bound = 2.0 * np.diff(B.indptr) * EPS * (stored_abs(B) @ np.abs(x))
    exact, stored_bound = stored_product(B, x)
    print(f"rectangular {B.shape}: error / bound {worst(_err(y[:rows], exact), stored_bound):.2e}")
    assert np.all(np.abs(y[:rows] - ref) <= bound) and worst(_err(y[:rows], exact), stored_bound) <= 1.0
    assert np.array_equal(h.gk_spmv(x, transpose=transpose), y)
    assert np.diff(B.indptr).max() <= 4096 and np.array_equal(y[:rows], ref)  # rows inside one tile are summed in csr_matvec's order
    h.close()


# ---------------------------------------------------------------- c. one solver iteration from an uploaded state
import bicgstab_reference as br  # noqa: E402
import cg_reference as cr  # noqa: E402
import test_gpu_bicgstab as t_bicgstab  # noqa: E402
import test_gpu_cg as t_cg  # noqa: E402
import test_gpu_gmres as t_gmres  # noqa: E402
import test_gpu_minres as t_minres  # noqa: E402


@functools.lru_cache(maxsize=None)
def step_matrices(kind):
    """``(non-canonical csr_257, same_order stencil)``: symmetric ones for cg and minres, non-symmetric ones for bicgstab and gmres"""
    if kind == "symmetric":
        return real_matrix(257), CASES["lap2d_37x29_potential_same_order_g0"]["build"]()
    return (_shared("step_matrices", noncanonical(br.random_csr(257, 3), seed=257)),
            _shared("step_matrices", noncanonical(br.convdiff(24, 20, 0.6, -0.3, 0.5), seed=0, dup=False, zeros=False, same_order=True)))


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "diagonal"])
@pytest.mark.parametrize("which", [0, 1], ids=["csr_257", "stencil"])
def test_cg_iteration_as_stored(monkeypatch, which, pre):
    """test_gpu_cg.py::test_one_iteration_against_longdouble, unchanged, on a new matrix"""
    B = step_matrices("symmetric")[which]
    monkeypatch.setattr(t_cg, "step_matrix", lambda name: B)
    monkeypatch.setattr(t_cg, "step_operator", lambda name: cr.Operator(B))
    t_cg.test_one_iteration_against_longdouble("noncanonical", pre)


@pytest.mark.parametrize("which", [0, 1], ids=["csr_257", "stencil"])
def test_minres_step_as_stored(monkeypatch, which):
    """test_gpu_minres.py::test_one_step_against_longdouble, unchanged, on a new matrix (the name it is given decides one expectation:
    a matrix with five entries in every row runs the ELL product, which scales on read - ``csr_5`` there, the stencil here)"""
    B = step_matrices("symmetric")[which]
    monkeypatch.setattr(t_minres, "step_matrix", lambda name: B)
    t_minres.test_one_step_against_longdouble("csr_5" if which else "csr_257")


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("which", [0, 1], ids=["csr_257", "stencil"])
def test_bicgstab_iteration_as_stored(monkeypatch, which, k):
    """test_gpu_bicgstab.py::test_one_iteration_against_longdouble, unchanged, on a new matrix (``convdiff``: it asserts the coded kernel)"""
    B = step_matrices("general")[which]
    monkeypatch.setattr(t_bicgstab, "step_matrix", lambda name: B)
    t_bicgstab.test_one_iteration_against_longdouble("convdiff_24x20" if which else "csr_257", k)


@pytest.mark.parametrize("k", [0, 4])
@pytest.mark.parametrize("which", [0, 1], ids=["csr_257", "stencil"])
def test_gmres_step_as_stored(monkeypatch, which, k):
    """test_gpu_gmres.py::test_one_inner_step_against_longdouble, unchanged, on a new matrix"""
    B = step_matrices("general")[which]
    monkeypatch.setattr(t_gmres, "step_matrix", lambda name: B)
    t_gmres.test_one_inner_step_against_longdouble("convdiff" if which else "csr", k)


# ---------------------------------------------------------------- d. end to end
import gmres_reference as gr  # noqa: E402
from test_trl_host import reference  # noqa: E402

import lanczos_amd  # noqa: E402
from lanczos_amd.bicgstab import NumpyBicgstabBackend  # noqa: E402
from lanczos_amd.cg import NumpyCgBackend  # noqa: E402
from lanczos_amd.eigs import NumpyCplxBackend, _eigs  # noqa: E402
from lanczos_amd.expm import NumpyExpmBackend  # noqa: E402
from lanczos_amd.gmres import NumpyGmresBackend  # noqa: E402


def test_eigsh_end_to_end_as_stored():
    """test_gpu_trl.py::test_eigsh_on_the_device's bars, against dense ``eigvalsh`` of the stored matrix"""
    B = real_matrix(1000, True)
    dense = B.toarray()
    ref, nrm = reference(dense, "LA", 3)
    info = {}
    theta, Y = lanczos_amd.eigsh(B, k=3, which="LA", v0=np.random.default_rng(3).standard_normal(1000), info=info)
    res = np.linalg.norm(dense @ Y - Y * theta, axis=0)
    assert np.all(np.diff(theta) >= 0) and np.abs(theta - ref).max() <= 1e-10 * nrm and res.max() <= 1e-9 * nrm
    assert np.abs(Y.T @ Y - np.eye(3)).max() <= 1e-12 and np.abs(info["residuals"] - res).max() <= 1e-12 * nrm


def test_complex_eigsh_end_to_end_as_stored():
    """test_eigsh_complex_host.py's bars (``check_pairs``) and test_gpu_eigsh_complex.py's on the residuals the device reports; the
    matrix is Hermitian as a matrix, not entry by entry, and its arrays are longer than ``indptr[-1]``"""
    Z = hermitian_matrix(1000, True)
    D = Z.toarray()
    assert abs(D - D.conj().T).max() == 0.0
    ev = np.linalg.eigvalsh(D)
    anorm = np.abs(ev).max()
    info = {}
    theta, Y = lanczos_amd.eigsh(Z, k=3, which="LA", info=info)
    err = np.abs(theta - ev[-3:]).max() / anorm
    host_res = np.linalg.norm(D @ Y - Y * theta, axis=0)
    orth = np.abs(Y.conj().T @ Y - np.eye(3)).max()
    print(f"complex eigsh: err/|A| {err:.1e}  res/|A| {host_res.max() / anorm:.1e}  |Y^H Y - I| {orth:.1e}")
    assert err <= 1e-10 and host_res.max() / anorm <= 1e-9 and orth <= 1e-12
    assert np.abs(info["residuals"] - host_res).max() <= 1e-12 * anorm


def test_eigs_end_to_end_as_stored():
    """tests/test_eigs_host.py's bars by its own rule: the true residual under ten times the larger of SciPy's own (ARPACK, ``tol=0``, the
    same stored matrix) and 1e-14, relative to ``max|lambda|``; every eigenvalue within the first-order bound ``2 bar max|lambda| / |y^H x|``
    of a dense one; the NumPy backend on the same matrix within the two bounds of it"""
    import scipy.linalg
    import scipy.sparse.linalg

    B = step_matrices("general")[0]
    D = B.toarray()
    lam, YL, XR = scipy.linalg.eig(D, left=True, right=True)
    yx = np.abs(np.einsum("ij,ij->j", YL.conj(), XR))
    amax = np.abs(lam).max()
    ws, Xs = scipy.sparse.linalg.eigs(B, k=3, which="LM", tol=0, v0=np.random.default_rng(1).standard_normal(257))
    bar = 10.0 * max(np.linalg.norm(D @ Xs - Xs * ws, axis=0).max() / amax, 1e-14)
    w, X = lanczos_amd.eigs(B, k=3, which="LM")
    wh, Xh = _eigs(NumpyCplxBackend(B), 257, 3, "LM", None, None, 0, None, True, None)
    res = np.linalg.norm(D @ X - X * w, axis=0)
    near = np.abs(w[:, None] - lam[None, :]).argmin(axis=1)
    bound = 2.0 * bar * amax / yx[near]
    print(f"eigs: true residual / max|lambda| {res.max() / amax:.2e} (bar {bar:.2e}), eigenvalue error / bound {(np.abs(w - lam[near]) / bound).max():.2e}")
    assert res.max() <= bar * amax and np.abs(np.linalg.norm(X, axis=0) - 1.0).max() <= 1e-13
    assert np.all(np.abs(w - lam[near]) <= bound) and len(set(near)) == 3
    assert np.all(np.abs(np.sort_complex(w) - np.sort_complex(wh)) <= 2.0 * bound.max())


def test_expm_multiply_end_to_end_as_stored():
    """tests/test_expm_host.py's bar, ``|out - exact| <= tol |exact|`` with the dense exponential of the stored matrix, and the NumPy
    backend under the same bar"""
    from expm_reference import exact, rel_errors

    B = real_matrix(257)
    b = np.random.default_rng(5).standard_normal(257)
    tol = 1e-10
    for a in (-0.5, -0.5j):
        ref = exact(B, b, a, [1.0])
        out = lanczos_amd.expm_multiply(B, b, a=a, tol=tol)
        host = lanczos_amd.expm_multiply(B, b, a=a, tol=tol, _backend=NumpyExpmBackend(B, a != -0.5))
        print(f"expm_multiply a = {a}: device {rel_errors(out[None, :], ref).max():.2e}, host {rel_errors(host[None, :], ref).max():.2e}")
        assert rel_errors(out[None, :], ref).max() <= tol and rel_errors(host[None, :], ref).max() <= tol


def _spd_257():
    S = sym_random(257)
    S = S - sp.diags(S.diagonal())
    return noncanonical((S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr(), seed=11)


def _admitted(adm_of):
    for seed in range(6):
        b = np.random.default_rng(seed).standard_normal(257)
        adm = adm_of(b)
        if adm["admitted"]:
            return b, adm
    raise AssertionError("no seed among 0 .. 5 is admitted")


def test_cg_jacobi_end_to_end_as_stored():
    """test_gpu_cg.py's ``_end_to_end`` on the first seed the reference's admission rule admits; ``M="jacobi"``: the summed diagonal"""
    B = _spd_257()
    d = 1.0 / B.diagonal()
    b, adm = _admitted(lambda b: cr.admission(B, b, 1e-8, d))
    h = _capi.Handle(0)
    t_cg._end_to_end(h, B, b, d, 1e-8, adm, B, "non-canonical spd 257")
    x, code = lanczos_amd.cg(B, b, rtol=1e-8, M="jacobi", handle=h)
    xd, _ = lanczos_amd.cg(B, b, rtol=1e-8, M=sp.diags(d), handle=h)
    assert code == 0 and np.array_equal(x, xd) and h.spmv_plan() == "csr-stream"
    h.close()


def test_bicgstab_end_to_end_as_stored():
    """test_gpu_bicgstab.py::test_end_to_end_on_the_admitted_cases' assertions on an admitted seed"""
    B = step_matrices("general")[0]
    b, adm = _admitted(lambda b: br.admission(B, b, 1e-8))
    host, dev = {}, {}
    xh, ch = lanczos_amd.bicgstab(B, b, rtol=1e-8, info=host, _backend=NumpyBicgstabBackend(B))
    x, code = lanczos_amd.bicgstab(B, b, rtol=1e-8, info=dev)
    assert code == ch == 0 and (dev["iterations"], dev["exit"], dev["code"]) == (host["iterations"], host["exit"], 0)
    assert dev["products"] == host["products"]
    true = np.asarray(br.Operator(B).matvec(x) - b.astype(LD), dtype=np.float64)
    dist = float(np.linalg.norm(x - xh))
    print(f"bicgstab: |x - x_host| {dist:.2e}, spread in x {adm['x_spread']:.2e}, true residual / atol_eff {np.linalg.norm(true) / adm['atol_eff']:.3f}")
    assert np.linalg.norm(true) <= 2.0 * adm["atol_eff"] and dist <= t_bicgstab.X_MARGIN * adm["x_spread"]


def test_gmres_end_to_end_as_stored():
    """test_gpu_gmres.py::test_end_to_end_on_the_admitted_cases' assertions on an admitted seed"""
    B = step_matrices("general")[0]
    b, adm = _admitted(lambda b: gr.admission(B, b, 1e-8, 20))
    host, dev = {}, {}
    xh, ch = lanczos_amd.gmres(B, b, rtol=1e-8, restart=20, info=host, _backend=NumpyGmresBackend(B))
    x, code = lanczos_amd.gmres(B, b, rtol=1e-8, restart=20, info=dev)
    assert code == ch == 0 and dev["exit"] == "converged"
    assert (dev["iterations"], dev["cycles"], dev["products"]) == (host["iterations"], host["cycles"], host["products"])
    op = br.Operator(B)
    true = float(np.linalg.norm(np.asarray(b.astype(LD) - op.matvec(x), dtype=np.float64)))
    slack = float(np.linalg.norm(br.product_bound(op, x)))
    dist = float(np.linalg.norm(np.asarray(x.astype(LD) - adm["runs"]["longdouble"]["x"], dtype=np.float64)))
    print(f"gmres: |x - x_longdouble| {dist:.2e}, spread in x {adm['x_spread']:.2e}, true residual / atol_eff {true / adm['atol_eff']:.3f}")
    assert dev["residual_norm"] <= adm["atol_eff"] and true <= adm["atol_eff"] + slack and dist <= t_gmres.X_MARGIN * adm["x_spread"]
