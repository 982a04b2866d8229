"""``expm_multiply`` on the host: the propagator's loop (``lanczos_amd.expm.propagate``) over ``NumpyExpmBackend`` against the
``eigh``-exact reference (tests/expm_reference.py), SciPy's calling conventions against ``scipy.sparse.linalg.expm_multiply`` itself,
and the argument errors, which are raised before a device is asked for.

The accuracy bar is the function's own contract: ``|out - exact| <= tol |exact|`` at every output time."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from expm_reference import exact, matrix, rel_errors, vector

from lanczos_amd import expm_multiply, synthetic
from lanczos_amd.expm import NumpyExpmBackend, route_of


def run(A, b, a, tol, ncv, info=None, **grid):
    backend = NumpyExpmBackend(A, route_of(A, b, a) != "real")
    return expm_multiply(A, b, a=a, tol=tol, ncv=ncv, info=info, _backend=backend, **grid)


def stop_time(name, a):
    """t = 3, but t = 0.5 where the solution would grow too far: a = +1, and the dense matrix (|A| = 14) with a real a"""
    return 0.5 if a == 1.0 or (name == "dense96" and not np.iscomplexobj(a)) else 3.0


@pytest.mark.parametrize("tol", [1e-8, 1e-11])
@pytest.mark.parametrize("ncv", [12, 30])
@pytest.mark.parametrize("cplx_b", [False, True], ids=["real_b", "complex_b"])
@pytest.mark.parametrize("a", [-1j, -1.0, 1.0], ids=["schroedinger", "heat", "plus"])
@pytest.mark.parametrize("name", ["lap20", "hof24x17", "dense96"])
def test_accuracy_against_eigh(name, a, cplx_b, ncv, tol):
    A = matrix(name)
    n = A.shape[0]
    b = vector(n, cplx_b)
    times = np.linspace(0.0, stop_time(name, a), 4)
    info = {}
    out = run(A, b, a, tol, ncv, info, start=times[0], stop=times[-1], num=4)
    ref = exact(A, b, a, times)
    err = rel_errors(out, ref)
    print(f"{name} a={a} ncv={ncv} tol={tol:g}: worst error / tol {err.max() / tol:.3f}, substeps {info['substeps']}, est {info['err_est']:.2e}")
    assert out.shape == (4, n)
    assert out.dtype == (np.float64 if route_of(A, b, a) == "real" else np.complex128)
    assert np.all(err <= tol)
    assert np.array_equal(out[0], b)  # t = 0 is B itself
    assert info["route"] == route_of(A, b, a) and info["ncv"] == ncv and info["matvecs"] == ncv * info["substeps"]
    if a == -1j:  # unitarity
        nb = np.linalg.norm(b)
        assert np.all(np.abs(np.linalg.norm(out, axis=1) - nb) <= tol * nb)


def test_routes_from_the_dtypes_alone():
    L, H, D = matrix("lap20"), matrix("hof24x17"), matrix("dense96")
    x, z = vector(400, False), vector(400, True)
    assert route_of(L, x, 1.0) == "real" and route_of(L, x, -1) == "real" and route_of(L.astype(np.float32), x.astype(np.float32), np.float32(2)) == "real"
    assert route_of(L, z, 1.0) == "mixed" and route_of(L, x, -1j) == "mixed" and route_of(L, x, 1 + 0j) == "mixed" and route_of(D, z[:96], 1.0) == "mixed"
    assert route_of(H, x, 1.0) == "complex" and route_of(H.astype(np.complex64), z, -1j) == "complex"
    assert route_of(synthetic.laplacian_2d_5pt(6, 5), x[:30], -1.0) == "real"  # synthetic.CSR has no dtype: real


# ---------------------------------------------------------------- breakdown
def test_an_invariant_subspace_truncates_the_substep():
    A = matrix("dense96")
    lam, U = np.linalg.eigh(A)
    b = U[:, 3] + 2.0 * U[:, 40] - 0.5 * U[:, 90]
    nb = np.linalg.norm(b)
    for a, t in ((-1j, 25.0), (-1.0, 0.5)):
        info = {}
        out = run(A, b, a, 1e-10, 12, info, start=t, stop=t, num=1)
        assert info["substeps"] == 1 and info["err_est"] == 0.0  # mm = 3: exact for any tau
        assert np.linalg.norm(out[0] - exact(A, b, a, [t])[0]) <= 1e-12 * nb
    # a step on mm = 3 rows serves mm - 1 = 2 output times: four times take two substeps, each truncated and exact
    info = {}
    times = np.linspace(2.0, 20.0, 4)
    out = run(A, b, -1j, 1e-10, 12, info, start=2.0, stop=20.0, num=4)
    assert info["substeps"] == 2 and info["err_est"] == 0.0
    assert np.all(np.linalg.norm(out - exact(A, b, -1j, times), axis=1) <= 1e-12 * nb)


def test_an_eigenvector_is_a_space_of_one():
    A = matrix("dense96")
    lam, U = np.linalg.eigh(A)
    info = {}
    out = run(A, 3.0 * U[:, 17], -1j, 1e-10, 8, info, start=1.0, stop=9.0, num=3)
    assert info["substeps"] == 3 and info["err_est"] == 0.0  # mm = 1: one output per substep
    ref = exact(A, 3.0 * U[:, 17], -1j, [1.0, 5.0, 9.0])
    assert np.all(np.linalg.norm(out - ref, axis=1) <= 1e-12 * 3.0)


def test_a_basis_that_fills_the_space_is_exact_in_one_substep():
    G = np.random.default_rng(12).standard_normal((12, 12))
    A = (G + G.T) / 2
    b = vector(12, False)
    for a, t in ((-1j, 40.0), (-1.0, 1.0)):
        info = {}
        out = run(A, b, a, 1e-10, 12, info, start=t, stop=t, num=1)
        ref = exact(A, b, a, [t])
        assert info["substeps"] == 1 and info["err_est"] == 0.0
        assert np.linalg.norm(out - ref) <= 1e-12 * np.linalg.norm(ref)


# ---------------------------------------------------------------- SciPy's calling conventions
A_SMALL = 0.1 * matrix("dense96")  # |A| = 1.4: SciPy's own result is good to a few eps for |t| <= 1


def against_scipy(B, scipy_values=True, **grid):
    """the same call to both: shape, dtype and values within 1e-10 relative - and within the same of the exact reference.
    ``scipy_values=False``: SciPy's values are not compared (see ``test_a_descending_grid``)"""
    out = run(A_SMALL, B, 1.0, 1e-13, 30, None, **grid)
    with np.errstate(all="ignore"):
        ref = spla.expm_multiply(A_SMALL, B, traceA=np.trace(A_SMALL), **grid)
    assert out.shape == ref.shape and out.dtype == ref.dtype
    if scipy_values:
        assert np.linalg.norm(out - ref) <= 1e-10 * np.linalg.norm(ref)
    times = np.linspace(**grid) if grid else [1.0]
    ex = exact(A_SMALL, B, 1.0, times).real
    assert np.linalg.norm(out.reshape(ex.shape) - ex) <= 1e-10 * np.linalg.norm(ex)
    return out


def test_a_single_time_is_t_equal_one():
    b = vector(96, False)
    assert against_scipy(b).shape == (96,)
    assert np.linalg.norm(expm_multiply(A_SMALL, b, traceA=0.0, _backend=NumpyExpmBackend(A_SMALL, False)) - exact(A_SMALL, b, 1.0, [1.0])[0].real) <= 1e-11


@pytest.mark.parametrize("grid", [dict(start=0.1, stop=1.0, num=5), dict(start=0.1, stop=1.0, num=5, endpoint=False),
                                  dict(start=-0.5, stop=0.5, num=4), dict(start=-0.5, stop=0.5, num=5),
                                  dict(start=0.0, stop=0.0, num=3), dict(start=0.25, stop=1.0)],
                         ids=["start_stop_num", "endpoint_false", "across_zero", "through_zero", "all_zero", "default_num"])
def test_time_grids_as_scipy(grid):
    out = against_scipy(vector(96, False), **grid)
    assert out.shape == (grid.get("num", 50), 96)


def test_a_descending_grid():
    """SciPy's own values are no reference here: on ``start=1.0, stop=0.2, num=4`` SciPy 1.15.3 returns a first row that is off by 0.59
    relative and ``inf`` behind it (its interval code assumes an ascending grid).  Shape and dtype are SciPy's; the values are held to
    the same 1e-10 against the exact reference, which is what SciPy approximates on the grids it handles."""
    out = against_scipy(vector(96, False), scipy_values=False, start=1.0, stop=0.2, num=4)
    assert out.shape == (4, 96)


def test_one_time_point_is_a_grid_of_one():
    """``num=1``: SciPy 1.15.3 raises ("at least two time points are required"); here the grid rule holds as for any ``num`` - the
    times are ``np.linspace(start, stop, 1)`` and the result is ``(1,) + B.shape`` - and the values are held to the exact reference"""
    b = vector(96, False)
    with pytest.raises(ValueError):
        spla.expm_multiply(A_SMALL, b, start=0.3, stop=0.9, num=1)
    out = run(A_SMALL, b, 1.0, 1e-13, 30, start=0.3, stop=0.9, num=1)
    ex = exact(A_SMALL, b, 1.0, [0.3]).real
    assert out.shape == (1, 96) and out.dtype == np.float64
    assert np.linalg.norm(out - ex) <= 1e-10 * np.linalg.norm(ex)


def test_a_column_vector_keeps_its_shape():
    B = vector(96, False).reshape(96, 1)
    assert against_scipy(B).shape == (96, 1)
    assert against_scipy(B, start=0.2, stop=1.0, num=3).shape == (3, 96, 1)


def test_shapes_and_dtypes_of_the_three_routes():
    L, H = matrix("lap20"), matrix("hof24x17")
    for A, b, a, dt in ((L, vector(400, False), -1.0, np.float64), (L, vector(400, False), -1j, np.complex128),
                        (L, vector(400, True), -1.0, np.complex128), (H, vector(408, False), -1.0, np.complex128),
                        (L.astype(np.float32), vector(400, False).astype(np.float32), -1.0, np.float64)):
        one = run(A, b, a, 1e-8, 20)
        many = run(A, b.reshape(-1, 1), a, 1e-8, 20, start=0.1, stop=0.3, num=2)
        assert one.shape == b.shape and one.dtype == dt
        assert many.shape == (2, len(b), 1) and many.dtype == dt


# ---------------------------------------------------------------- argument errors: before any device is asked for
def test_argument_errors_need_no_device():
    A = matrix("dense96")
    b = vector(96, False)
    for ncv in (0, 1, 65, 97):
        with pytest.raises(ValueError, match="ncv"):
            expm_multiply(A, b, ncv=ncv)
    with pytest.raises(ValueError, match="ncv"):
        expm_multiply(A[:10, :10], b[:10], ncv=11)  # ncv <= n
    with pytest.raises(ValueError):
        expm_multiply(A, b[:95])
    with pytest.raises(ValueError):
        expm_multiply(A[:, :95], b)
    with pytest.raises(NotImplementedError):
        expm_multiply(A, np.ones((96, 2)))
    with pytest.raises(TypeError):
        expm_multiply(A, b, 0.1, 1.0, 3, True, None, -1j)  # a is keyword-only


def test_n_equal_one_in_closed_form():
    for A in (np.array([[0.5]]), sp.csr_matrix(np.array([[0.5]]))):
        info = {}
        out = expm_multiply(A, np.array([2.0]), start=0.0, stop=2.0, num=3, a=-1.0, info=info)
        assert out.dtype == np.float64 and np.allclose(out[:, 0], 2.0 * np.exp(-0.5 * np.array([0.0, 1.0, 2.0])), rtol=1e-15)
        assert info["route"] == "real" and info["substeps"] == 0
    out = expm_multiply(np.array([[0.5]]), np.array([[2.0]]), a=-1j)
    assert out.shape == (1, 1) and out.dtype == np.complex128 and abs(out[0, 0] - 2.0 * np.exp(-0.5j)) <= 1e-15
