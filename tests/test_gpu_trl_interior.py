"""The interior mode of lanczos_amd.eigsh on the device: lz_trl_set_series / lz_trl_filter_apply against SeriesFilter in NumPy, the fused
and the unfused series step against each other, eigsh(sigma=..., filter_degree=...) against dense eigvalsh and against the NumPy backend,
state rules, the drop-in class's exact_eigs = "device-filtered"."""
import functools

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg
from test_trl_host import _matrix
from test_trl_interior_host import assert_nearest, solved, spectrum, start_vector

import lanczos_amd
from lanczos_amd import Lanczos, _capi
from lanczos_amd.eigsh import ChebFilter, SeriesFilter, upload_matrix

pytestmark = pytest.mark.gpu

DEGREES = (1, 2, 3, 4, 17)  # 1 - 4: the special first step and every rotation of the three work vectors; 17: the coefficient index
# dense: the GEMV and k_cheb_series_step; the graph: CSR without an ELL copy; ragged: a row count (700) that is no multiple of the padding;
# the three stencil fixtures have 5 / 7 / 27 entries in every row and take the coded ELL kernels (k_spmv_cls2, k_spmv_cls2, k_spmv_cls),
# the tuning knobs of ELL_FORMS put k_spmv_ell (uncoded, offsets coded) and k_spmv_cls (one / two units) under the same matrices
GENERAL = ("c1_dense512_n20", "graph_M2000_E7000_n40", "ragged_M700_n25")
ELL = ("lap2d_32x32_n30", "lap3d_8x8x8_n40", "deuteron3d_N12_27pt_n100")
# lz_set_tuning: 17 = 2 / 3 the uncoded ELL copy with one row per lane / two adjacent rows per lane, 4 offsets coded only; 23 = 1 / 3 the
# coded one-row-per-lane kernel with one / two units per workgroup
ELL_FORMS = [(), ((17, 2),), ((17, 3),), ((17, 4),), ((23, 1),), ((23, 3),)]


def make_series(name, degree):
    """a series over bounds that hold the spectrum, peaked a third of the way up"""
    ev, _ = spectrum(name)
    w = ev[-1] - ev[0]
    return SeriesFilter(ev[0] - 0.01 * w, ev[-1] + 0.01 * w, ev[0] + 0.31 * w, degree)


def device_apply(name, degree, flags=0, tuning=(), poison=True):
    """p(A) x on the device -> (y, x, series, the raw result row with its padding)"""
    A, _ = _matrix(name)
    h = _capi.Handle(0)
    h.set_options(flags)
    for knob, value in tuning:
        h.set_tuning(knob, value)
    n = upload_matrix(h, A)
    m = 4
    x = np.random.default_rng(n + degree).standard_normal(n)
    h.trl_begin(m, x)
    f = make_series(name, degree)
    h.trl_set_series(f.coefficients(), f.c, f.e)
    if poison:  # the staging row starts with a NaN padding: the result row's padding must still come out zero
        row = np.full((1, h.padded_rows(n)), np.nan)
        row[0, :n] = 1.0
        h.trl_set_rows(m, row)
    y = h.trl_filter_apply(x)
    raw = h.trl_get_rows(m, 1)[0]
    h.close()
    return y, x, f, raw


@functools.lru_cache(maxsize=None)
def host_apply(name, degree):
    A, _ = _matrix(name)
    n = A.shape[0]
    x = np.random.default_rng(n + degree).standard_normal(n)
    return make_series(name, degree).apply(lambda v: A @ v, x)


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("name", GENERAL + ELL)
def test_series_apply_matches_numpy(name, degree):
    y, x, f, raw = device_apply(name, degree)
    ref = host_apply(name, degree)
    rel = np.abs(y - ref).max() / np.abs(ref).max()
    print(f"{name} degree {degree}: device - numpy {rel:.3e} of max|y|, bound {1e-13 * (degree + 1):.1e}")
    assert rel <= 1e-13 * (degree + 1)
    n = y.size
    assert np.array_equal(raw[:n], y) and np.all(raw[n:] == 0.0)


@pytest.mark.parametrize("tuning", ELL_FORMS, ids=lambda t: "default" if not t else "knob%d=%d" % t[0])
@pytest.mark.parametrize("name", ELL)
def test_fused_and_unfused_series_steps_give_the_same_bits(name, tuning):
    """the result row is the running sum after the last step; degree 1 is the first-step form of it, degrees 2 - 4 every rotation of the
    update form, and its padding (rows .. rows_pad) reads back as zero on either path although the staging row's was NaN"""
    for degree in DEGREES:
        fused = device_apply(name, degree, tuning=tuning)
        unfused = device_apply(name, degree, flags=_capi.FLAG_TRL_FILTER_UNFUSED, tuning=tuning)  # the same SpMV kernel + k_cheb_series_step
        stream = device_apply(name, degree, flags=_capi.FLAG_SPMV_STREAM, tuning=tuning)  # the CSR-stream SpMV + k_cheb_series_step
        n = fused[0].size
        assert np.array_equal(fused[3], unfused[3]) and np.array_equal(fused[3], stream[3])
        assert np.all(fused[3][n:] == 0.0) and np.all(unfused[3][n:] == 0.0)
        assert np.isfinite(fused[0]).all() and np.abs(fused[0]).max() > 0
        ref = host_apply(name, degree)
        assert np.abs(fused[0] - ref).max() <= 1e-13 * (degree + 1) * np.abs(ref).max()


def test_series_and_filter_clear_each_other():
    name = "lap2d_32x32_n30"
    A, _ = _matrix(name)
    ev, _ = spectrum(name)
    n = A.shape[0]
    x = np.random.default_rng(0).standard_normal(n)
    s = make_series(name, 6)
    f = ChebFilter(ev[0] + 0.3 * (ev[-1] - ev[0]), ev[-1] + 0.01, ev[0] - 0.01, 6)
    h = _capi.Handle(0)
    upload_matrix(h, A)
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):  # no basis yet
        h.trl_set_series(s.coefficients(), s.c, s.e)
    m = 8
    h.trl_begin(m, x)
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):  # neither set
        h.trl_filter_apply(x)
    free0, _ = h.device_memory()
    h.trl_set_filter(f.coefficients(), f.c)
    yf = h.trl_filter_apply(x)
    h.trl_set_series(s.coefficients(), s.c, s.e)  # clears the filter
    ys = h.trl_filter_apply(x)
    assert not np.array_equal(ys, yf)
    assert np.abs(ys - s.apply(lambda v: A @ v, x)).max() <= 7e-13 * np.abs(ys).max()
    h.trl_set_series(None)  # degree 0 clears the series and does not bring the filter back
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):
        h.trl_filter_apply(x)
    h.trl_set_series(s.coefficients(), s.c, s.e)
    h.trl_set_filter(f.coefficients(), f.c)  # clears the series
    assert np.array_equal(h.trl_filter_apply(x), yf)
    h.trl_set_filter(None)  # and clearing the filter does not bring the series back
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):
        h.trl_filter_apply(x)
    h.trl_set_series(s.coefficients(), s.c, s.e)
    h.trl_begin(m, x)  # the same m keeps the series (the driver sets it before the loop's own lz_trl_begin)
    assert np.array_equal(h.trl_filter_apply(x), ys)
    ps, _ = h.trl_extend(0, m)
    h.trl_set_series(None)  # switched off: the extension is that of a handle that never had one
    h.trl_begin(m, x)
    p0, b0 = h.trl_extend(0, m)
    g = _capi.Handle(0)
    upload_matrix(g, A)
    g.trl_begin(m, x)
    p1, b1 = g.trl_extend(0, m)
    g.close()
    assert np.array_equal(p0, p1) and np.array_equal(b0, b1) and not np.array_equal(ps, p0)
    free1, _ = h.device_memory()
    assert free0 - free1 <= 3 * h.padded_rows(n) * 8 + (64 << 20)  # two work vectors and the running sum
    for bad in ((s.coefficients(), s.c, 0.0), (s.coefficients(), np.nan, s.e)):
        with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_ARG"):
            h.trl_set_series(*bad)
    h.trl_set_series(s.coefficients(), s.c, s.e)
    upload_matrix(h, A)  # a new matrix of the same size: the basis stays usable, the series is gone
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):
        h.trl_filter_apply(x)
    h.close()


def set_operator(h, name, kind, degree):
    """the series of make_series, or the filter of test_series_and_filter_clear_each_other, at this degree"""
    if kind == "series":
        s = make_series(name, degree)
        h.trl_set_series(s.coefficients(), s.c, s.e)
    else:
        ev, _ = spectrum(name)
        f = ChebFilter(ev[0] + 0.3 * (ev[-1] - ev[0]), ev[-1] + 0.01, ev[0] - 0.01, degree)
        h.trl_set_filter(f.coefficients(), f.c)


# the fused ELL epilogue; the GEMV and the two streaming kernels; 700 rows, no multiple of the padding
@pytest.mark.parametrize("name", ["lap2d_32x32_n30", "c1_dense512_n20", "ragged_M700_n25"])
def test_one_operator_state_survives_changes_of_kind_and_degree(name):
    """The filter and the series share one state in the handle (kind, degree, one coefficient array, the work vectors): after every
    change of kind or degree - a longer array, a shorter one, a running sum that an earlier series left behind - the operator is
    bit for bit that of a fresh handle which only ever set this one, and the padding of the result row is zero."""
    A, _ = _matrix(name)
    m = 8
    h = _capi.Handle(0)
    n = upload_matrix(h, A)
    x = np.random.default_rng(11).standard_normal(n)
    h.trl_begin(m, x)
    fresh = {}
    for kind, degree in (("series", 3), ("filter", 24), ("series", 40), ("filter", 2), ("series", 3)):
        set_operator(h, name, kind, degree)
        y = h.trl_filter_apply(x)
        raw = h.trl_get_rows(m, 1)[0]
        if (kind, degree) not in fresh:
            g = _capi.Handle(0)
            upload_matrix(g, A)
            g.trl_begin(m, x)
            set_operator(g, name, kind, degree)
            fresh[(kind, degree)] = g.trl_filter_apply(x)
            g.close()
        assert np.isfinite(y).all() and np.abs(y).max() > 0
        assert np.array_equal(y, fresh[(kind, degree)]), (kind, degree)
        assert np.array_equal(raw[:n], y) and np.all(raw[n:] == 0.0), (kind, degree)
    h.trl_begin(12, x)  # a basis of another size leaves no operator set
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):
        h.trl_filter_apply(x)
    h.trl_begin(m, x)  # and the old size does not bring it back
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):
        h.trl_filter_apply(x)
    h.close()


@pytest.mark.parametrize("name,k,sigma", [("graph_M2000_E7000_n40", 10, 5.0), ("lap2d_32x32_n30", 10, 3.0), ("deuteron3d_N12_27pt_n100", 20, 0.0)])
def test_interior_eigsh_on_the_device(name, k, sigma):
    A, dense = _matrix(name)
    n = dense.shape[0]
    _, nrm = spectrum(name)
    v0 = start_vector(n)
    info = {}
    theta, Y = lanczos_amd.eigsh(A, k=k, sigma=sigma, which="LM", v0=v0, filter_degree=16, info=info)
    # eigsh asserts to 1e-10 |A| here; the shared helper checks 1e-12 |A| and the tie rule, which the device meets as well
    assert_nearest(name, k, sigma, theta)
    res = np.linalg.norm(dense @ Y - Y * theta, axis=0)
    f = info["filter"]
    print(f"{name} k {k} sigma {sigma}: degree {f['degree']}, steps {info['steps']}, products {info['matvecs']}, residual {res.max() / nrm:.1e} |A|, "
          f"attempts {[(a['degree'], a['pairs'], a['steps'], a['certified']) for a in f['attempts']]}")
    assert res.max() <= 1e-9 * nrm
    assert np.abs(Y.T @ Y - np.eye(k)).max() <= 1e-12
    assert np.abs(info["residuals"] - res).max() <= 1e-12 * nrm
    assert f["requested"] == 16 and f["attempts"][-1]["certified"]
    host = solved(name, k, sigma, 16)[0]  # the NumPy backend's run from the same start vector (shared with the host tests)
    assert np.abs(theta - host).max() <= 1e-10 * nrm


def test_exact_eigs_device_filtered():
    Lanczos.verbose = False
    H, dense = _matrix("deuteron3d_N12_27pt_n100")
    _, nrm = spectrum("deuteron3d_N12_27pt_n100")
    ref = np.sort(scipy.sparse.linalg.eigsh(H, k=20, which="SM")[0])
    s = Lanczos(H)
    assert s.exact_eigs_filter_degree == 32
    s.exact_eigs = "device-filtered"
    s.find_exact_eigs(20)
    assert np.abs(np.sort(s._H_eigvals_actual) - ref).max() <= 1e-10 * nrm
    Y = s._H_eigvecs_actual
    assert Y.shape == (dense.shape[0], 20)
    assert np.linalg.norm(dense @ Y - Y * s._H_eigvals_actual, axis=0).max() <= 1e-9 * nrm
    s.close()
