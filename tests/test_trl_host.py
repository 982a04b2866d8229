"""The thick-restart outer loop of lanczos_amd.eigsh, driven by its NumPy backend (no GPU)."""
import numpy as np
import pytest
import scipy.sparse
from conftest import load_golden

from lanczos_amd.eigsh import NumpyBackend, _order, check_args, trl

# (fixture, which, k): the cases of the triage prototype
CASES = [
    ("deuteron1d_N1001_n1001", "SM", 20),
    ("box1d_N500_n50", "SM", 20),
    ("deuteron3d_N12_27pt_n100", "SA", 6),
    ("deuteron3d_N12_27pt_n100", "SA", 10),
    ("graph_M2000_E7000_n40", "LA", 6),
    ("lap3d_8x8x8_n40", "LA", 8),
    ("lap2d_32x32_n30", "SA", 10),
    ("c1_dense512_n20", "LM", 6),
]


def _matrix(name):
    _, H = load_golden(name)
    dense = H.toarray() if scipy.sparse.issparse(H) else np.asarray(H)
    return (H.tocsr() if scipy.sparse.issparse(H) else dense), dense


def reference(dense, which, k):
    ev = np.linalg.eigvalsh(dense)
    return np.sort(ev[_order(ev, which)[:k]]), np.abs(ev).max()


@pytest.mark.parametrize("name,which,k", CASES)
def test_outer_loop_finds_the_wanted_eigenvalues(name, which, k):
    A, dense = _matrix(name)
    ref, nrm = reference(dense, which, k)
    be = NumpyBackend(A)
    theta, info = trl(be, dense.shape[0], k, which)
    assert np.all(np.diff(theta) >= 0)
    assert np.abs(theta - ref).max() <= 1e-12 * nrm
    res = be.residuals(k, theta)
    assert res.max() <= 1e-9 * nrm
    assert info["probes"] >= 1 and info["matvecs"] > 0


def test_without_the_probe_a_degenerate_copy_is_missed():
    A, dense = _matrix("deuteron3d_N12_27pt_n100")
    ref, nrm = reference(dense, "SA", 6)
    wrong = 0
    for seed in range(20):
        v0 = np.random.default_rng(seed).standard_normal(dense.shape[0])
        theta, _ = trl(NumpyBackend(A), dense.shape[0], 6, "SA", v0=v0, probe=False)
        wrong += np.abs(theta - ref).max() > 1e-12 * nrm
        theta, _ = trl(NumpyBackend(A), dense.shape[0], 6, "SA", v0=v0)
        assert np.abs(theta - ref).max() <= 1e-12 * nrm, seed
    assert wrong >= 1


def test_breakdown_ncv_equal_to_n():
    A, dense = _matrix("lap2d_8x8_n2")
    ref, nrm = reference(dense, "SA", 6)
    theta, info = trl(NumpyBackend(A), 64, 6, "SA", ncv=64)
    assert info["breakdowns"] >= 1
    assert np.abs(theta - ref).max() <= 1e-12 * nrm


def test_breakdown_on_three_distinct_values():
    D = scipy.sparse.diags(np.repeat([1.0, 2.0, 3.0], 10)).tocsr()
    theta, info = trl(NumpyBackend(D), 30, 3, "SA")
    assert info["breakdowns"] >= 1
    assert np.abs(theta - 1.0).max() <= 1e-12 * 3


def test_argument_errors_match_scipy():
    import scipy.sparse.linalg as sla

    A, dense = _matrix("lap2d_8x8_n2")
    for kw, exc in [({"k": 64}, TypeError), ({"k": 0}, ValueError), ({"k": 6, "which": "XX"}, ValueError), ({"k": 6, "ncv": 6}, ValueError)]:
        with pytest.raises(exc):
            sla.eigsh(A, **kw)
        with pytest.raises(exc):
            check_args(64, kw["k"], kw.get("which", "LM"), kw.get("ncv"))
    with pytest.raises(ValueError, match="k\\+3<=ncv"):  # stricter than SciPy: two spare rows and one for the probe
        check_args(64, 6, "LM", 8)
    with pytest.raises(ValueError, match="ncv"):  # the restart holds S in LDS: at most 128 basis vectors
        check_args(1000, 6, "LM", 129)
    assert check_args(64, 6, "LM", 65) == 64  # SciPy clamps ncv to n as well
    with pytest.raises(NotImplementedError):
        check_args(64, 6, "BE", None)
    with pytest.raises(NotImplementedError):
        check_args(64, 6, "LM", None, sigma=1.0)
    assert check_args(1000, 6, "LM", None) == 20 and check_args(1000, 15, "LM", None) == 31 and check_args(10, 3, "LM", None) == 10


def test_max_iterations_raise_arpack_no_convergence():
    from scipy.sparse.linalg import ArpackNoConvergence

    A, dense = _matrix("deuteron1d_N1001_n1001")
    with pytest.raises(ArpackNoConvergence) as e:
        trl(NumpyBackend(A), dense.shape[0], 20, "SM", maxiter=1)
    assert len(e.value.eigenvalues) == e.value.eigenvectors.shape[1] < 20


def test_a_run_that_gives_up_hands_on_its_counts():
    """err.info of the ArpackNoConvergence that trl raises: its counts, the steps being those of the extend calls"""
    from scipy.sparse.linalg import ArpackNoConvergence

    class Counting(NumpyBackend):
        steps = 0

        def extend(self, k, m):
            self.steps += m - k
            return super().extend(k, m)

    A, dense = _matrix("deuteron1d_N1001_n1001")
    be = Counting(A)
    with pytest.raises(ArpackNoConvergence) as e:
        trl(be, dense.shape[0], 20, "SM", maxiter=1)
    info = e.value.info
    assert {"matvecs", "cycles", "probes", "breakdowns"} <= set(info)
    assert info["matvecs"] == be.steps > 0 and info["cycles"] == 1


def test_global_rng_is_untouched():
    A, dense = _matrix("lap2d_32x32_n30")
    np.random.seed(7)
    before = np.random.get_state()
    a, _ = trl(NumpyBackend(A), dense.shape[0], 4, "SA")
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    b, _ = trl(NumpyBackend(A), dense.shape[0], 4, "SA")
    assert np.array_equal(a, b)  # the private generator is seeded per call
