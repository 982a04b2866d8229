"""The Chebyshev filter of lanczos_amd.eigsh on the device: lz_trl_set_filter / lz_trl_filter_apply / lz_trl_rayleigh against NumPy,
the fused and the unfused filter step against each other, eigsh(filter_degree=...) against dense eigvalsh, footprint, state errors."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse
from test_trl_filter_host import CASES
from test_trl_host import _matrix, reference

import lanczos_amd
from lanczos_amd import Hamiltonian, Lanczos, _capi, synthetic
from lanczos_amd._pool import StencilOperator
from lanczos_amd.eigsh import ChebFilter, DeviceBackend, trl_filtered, upload_matrix

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DEGREES = (2, 3, 16)
W27 = np.array([-44 / 3, 1.0, 1.0 / 2, 1.0 / 3]) * 3.0 / 13


def stencil27(N):
    pot = np.random.default_rng(N).uniform(-1.0, 0.0, N**3)
    return StencilOperator((N, N, N), 27, 1.0, W27, True, potential=pot)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(what eigsh's upload takes, SciPy CSR or dense ndarray of the same matrix)"""
    if name == "dense512":
        _, dense = _matrix("c1_dense512_n20")
        return dense, dense
    if name == "stencil27_12":
        op = stencil27(12)
        return op, op.to_scipy()
    A = {"lap2d_8x8": lambda: synthetic.laplacian_2d_5pt(8, 8), "lap2d_61x67": lambda: synthetic.laplacian_2d_5pt(61, 67),
         "lap2d_1003x997": lambda: synthetic.laplacian_2d_5pt(1003, 997), "lap3d_20x21x23": lambda: synthetic.laplacian_3d_7pt(20, 21, 23),
         "graph2000": lambda: synthetic.random_graph_laplacian(2000, 7000)}[name]()
    return A, A.to_scipy().tocsr()


def make_filter(S, degree):
    """a filter for the lower end whose bounds hold the spectrum (eigvalsh up to 2000 rows, Gershgorin's discs beyond): |p| <= 1 on it"""
    if S.shape[0] <= 2000:
        ev = np.linalg.eigvalsh(S.toarray() if scipy.sparse.issparse(S) else S)
        emin, emax = ev[0], ev[-1]
    else:
        d = S.diagonal()
        r = np.asarray(abs(S).sum(axis=1)).ravel() - np.abs(d)
        emin, emax = (d - r).min(), (d + r).max()
    w = emax - emin
    return ChebFilter(emin + 0.3 * w, emax + 0.01 * w, emin - 0.01 * w, degree)


def restatement(S, f, x, dtype):
    """the recurrence as the device states it, z = a (A y - c y) - b x, in `dtype`"""
    S = S.astype(dtype) if not scipy.sparse.issparse(S) or dtype == np.float64 else S.toarray().astype(dtype)
    prev = cur = x.astype(dtype)
    c = dtype(f.c)
    for a, b in f.coefficients():
        prev, cur = cur, dtype(a) * (S @ cur - c * cur) - dtype(b) * prev
    return cur


def device_apply(name, degree, poison=True, flags=0, tuning=()):
    """p(A) x on the device -> (y, x, filter, the raw result row with its padding)"""
    A, S = matrix(name)
    h = _capi.Handle(0)
    h.set_options(flags)
    for knob, value in tuning:
        h.set_tuning(knob, value)
    n = upload_matrix(h, A)
    m = 4
    x = np.random.default_rng(n + degree).standard_normal(n)
    h.trl_begin(m, x)
    f = make_filter(S, degree)
    h.trl_set_filter(f.coefficients(), f.c)
    if poison:  # the staging row starts with a NaN padding: the result row's padding must still come out zero
        row = np.full((1, h.padded_rows(n)), np.nan)
        row[0, :n] = 1.0
        h.trl_set_rows(m, row)
    y = h.trl_filter_apply(x)
    raw = h.trl_get_rows(m, 1)[0]
    h.close()
    return y, x, f, raw


SMALL = ("lap2d_8x8", "graph2000", "dense512", "stencil27_12")
LARGE = ("lap2d_61x67", "lap2d_1003x997")


@functools.lru_cache(maxsize=None)
def small_case(name, degree):
    """device result, float64 restatement and long-double reference of one small case (n <= 2000), computed once"""
    y, x, f, raw = device_apply(name, degree)
    _, S = matrix(name)
    return y, restatement(S, f, x, np.float64), restatement(S, f, x, np.longdouble), raw


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("name", SMALL)
def test_filter_apply_matches_numpy(name, degree):
    y, y64, yld, raw = small_case(name, degree)
    n = y.size
    dev = np.abs(y - yld).max()
    host = np.abs(y64 - yld).max()
    print(f"{name} degree {degree}: device - longdouble {float(dev):.3e}, float64 - longdouble {float(host):.3e}, max|y| {np.abs(y).max():.3e}")
    # 4x the float64 restatement's own distance from the long-double recurrence (fma contraction, the SpMV's summation order) + 4 eps max|y|
    assert dev <= 4 * host + 4 * EPS * np.abs(y).max()
    assert np.array_equal(raw[:n], y) and np.all(raw[n:] == 0.0)


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("name", LARGE)
def test_filter_apply_matches_numpy_large(name, degree):
    # the bound is measured, not invented: 4x the largest relative distance between the device and the float64 restatement on the small cases
    bound = 4 * max(float(np.abs(small_case(s, d)[0] - small_case(s, d)[1]).max() / np.abs(small_case(s, d)[0]).max()) for s in SMALL for d in DEGREES)
    y, x, f, raw = device_apply(name, degree)
    _, S = matrix(name)
    y64 = restatement(S, f, x, np.float64)
    rel = np.abs(y - y64).max() / np.abs(y).max()
    print(f"{name} degree {degree}: device - float64 {rel:.3e} of max|y|, bound {bound:.3e}")
    assert rel <= bound
    assert np.array_equal(raw[: y.size], y) and np.all(raw[y.size:] == 0.0)


# tuning knobs that select another ELL kernel for the same matrix (lz_set_tuning): 17 = 2 / 3 the uncoded copy with one row per lane /
# two adjacent rows per lane, 4 offsets coded only; 23 = 1 / 3 the coded one-row-per-lane kernel with one / two units per workgroup
ELL_FORMS = [(), ((17, 2),), ((17, 3),), ((17, 4),), ((23, 1),), ((23, 3),)]


@pytest.mark.parametrize("tuning", ELL_FORMS, ids=lambda t: "default" if not t else "knob%d=%d" % t[0])
@pytest.mark.parametrize("name", ["lap2d_61x67", "lap3d_20x21x23", "stencil27_12"])
def test_fused_and_unfused_filter_steps_give_the_same_bits(name, tuning):
    for degree in DEGREES:
        fused = device_apply(name, degree, tuning=tuning)
        unfused = device_apply(name, degree, flags=_capi.FLAG_TRL_FILTER_UNFUSED, tuning=tuning)  # the same SpMV kernel + k_cheb_step
        stream = device_apply(name, degree, flags=_capi.FLAG_SPMV_STREAM, tuning=tuning)  # the CSR-stream SpMV + k_cheb_step
        assert np.array_equal(fused[3], unfused[3]) and np.array_equal(fused[3], stream[3])
        assert np.isfinite(fused[0]).all() and np.abs(fused[0]).max() > 0


@pytest.mark.parametrize("name,which,k", CASES)
def test_filtered_eigsh_on_the_device(name, which, k):
    A, dense = _matrix(name)
    ref, nrm = reference(dense, which, k)
    v0 = np.random.default_rng(3).standard_normal(dense.shape[0])
    h = _capi.Handle(0)
    plain, info = {}, {}
    theta0, Y0 = lanczos_amd.eigsh(A, k=k, which=which, v0=v0, handle=h, info=plain)
    theta, Y = lanczos_amd.eigsh(A, k=k, which=which, v0=v0, handle=h, info=info, filter_degree=16)
    assert np.all(np.diff(theta) >= 0)
    assert np.abs(theta - ref).max() <= 1e-10 * nrm
    res = np.linalg.norm(dense @ Y - Y * theta, axis=0)
    assert res.max() <= 1e-9 * nrm
    assert np.abs(Y.T @ Y - np.eye(k)).max() <= 1e-12
    assert np.abs(info["residuals"] - res).max() <= 1e-12 * nrm
    theta2, Y2 = lanczos_amd.eigsh(A, k=k, which=which, v0=v0, handle=h, filter_degree=16)
    assert np.array_equal(theta, theta2) and np.array_equal(Y, Y2)  # same v0, same bits
    print(f"{name} {which} {k}: plain steps {plain['matvecs']}, filtered steps {info['steps']}, A-products {info['matvecs']}, degree {info['filter']['degree']}")
    assert info["steps"] <= plain["matvecs"] / 2
    assert sorted(plain) == ["anorm", "breakdowns", "cycles", "matvecs", "probes", "residuals"]  # an unfiltered run's info is as it was
    theta3, Y3 = lanczos_amd.eigsh(A, k=k, which=which, v0=v0, handle=h, filter_degree=None)  # None: today's path, bit for bit
    assert np.array_equal(theta0, theta3) and np.array_equal(Y0, Y3)
    h.close()


@pytest.mark.parametrize("k", [1, 6, 20])
@pytest.mark.parametrize("rows", [37, 4087])
def test_rayleigh_matches_numpy(rows, k):
    if rows == 37:
        S = scipy.sparse.random(rows, rows, density=0.3, random_state=np.random.default_rng(5), format="csr")
        S = (S + S.T).tocsr()
        S.sort_indices()
        A = S
    else:
        A, S = matrix("lap2d_61x67")
    h = _capi.Handle(0)
    upload_matrix(h, A)
    m = 24
    h.trl_begin(m, np.ones(rows))
    V = np.zeros((m + 1, h.padded_rows(rows)))
    V[:, :rows] = np.random.default_rng(rows + k).standard_normal((m + 1, rows))
    h.trl_set_rows(0, V)
    f = make_filter(S, 5)
    h.trl_set_filter(f.coefficients(), f.c)  # the Rayleigh quotient is A's, filter or not
    G = h.trl_rayleigh(k)
    ref = V[:k, :rows] @ (S @ V[:k, :rows].T)
    assert np.abs(G - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.array_equal(h.trl_get_rows(0, m + 1), V)  # the basis is read only
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_ARG"):
        h.trl_rayleigh(m)
    h.close()


def test_filtered_deuteron_hamiltonian_footprint():
    Hamiltonian.verbose = Lanczos.verbose = False
    N = 40
    os.makedirs("T_matrices", exist_ok=True)
    ham = Hamiltonian(N, 25, synthetic.DeuteronPotential(), 197.327**2 / (2 * 469.4592) / (25.0 / N) ** 2)
    ham.device_potential = True
    op = ham.operator("27")
    h = _capi.Handle(0)
    n = upload_matrix(h, op)
    free0, _ = h.device_memory()
    theta, info = trl_filtered(DeviceBackend(h, n), n, 4, "SA", 16)
    free1, _ = h.device_memory()
    ncv = 20
    assert free0 - free1 <= (ncv + 3) * h.padded_rows(n) * 8 + (64 << 20)  # the basis, w and the filter's two work vectors
    res = h.trl_residuals(4, theta)
    h.close()
    s = Lanczos(op)
    s.execute_Lanczos(300, seed=1)
    lowest = np.min(s.H_eigvals)
    s.close()
    assert theta[0] <= lowest + 1e-10 * abs(lowest)
    assert res.max() <= 1e-9 * info["anorm"]


def test_filter_state_errors():
    A, S = matrix("lap2d_61x67")
    n = S.shape[0]
    f = make_filter(S, 8)
    x = np.random.default_rng(0).standard_normal(n)
    h = _capi.Handle(0)
    upload_matrix(h, A)
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):  # no basis yet
        h.trl_set_filter(f.coefficients(), f.c)
    m = 8
    h.trl_begin(m, x)
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):  # no filter yet
        h.trl_filter_apply(x)
    h.trl_set_filter(f.coefficients(), f.c)
    y = h.trl_filter_apply(x)
    h.trl_begin(m, x)  # the same m keeps the filter (the driver sets it before the loop's own lz_trl_begin)
    assert np.array_equal(h.trl_filter_apply(x), y)
    pf, bf = h.trl_extend(0, m)
    h.trl_set_filter(None)  # switched off: the extension is the one of a handle that never had a filter
    h.trl_begin(m, x)
    p0, b0 = h.trl_extend(0, m)
    rows0 = h.trl_get_rows(0, m + 1)
    g = _capi.Handle(0)
    upload_matrix(g, A)
    g.trl_begin(m, x)
    p1, b1 = g.trl_extend(0, m)
    assert np.array_equal(p0, p1) and np.array_equal(b0, b1) and np.array_equal(rows0, g.trl_get_rows(0, m + 1))
    assert not np.array_equal(pf, p0)  # (and the filtered extension was a different one)
    g.close()
    h.trl_set_filter(f.coefficients(), f.c)
    upload_matrix(h, A)  # a new matrix of the same size: the basis stays usable, the filter is gone
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):
        h.trl_filter_apply(x)
    p2, b2 = h.trl_extend(0, m)
    assert np.array_equal(p2, p0) and np.array_equal(b2, b0)
    h.close()
