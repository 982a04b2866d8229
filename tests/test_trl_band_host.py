"""The band (block) thick-restart loop of lanczos_amd.eigsh, ``trl_band``, driven by the NumPy band backend (no GPU).

``ncv`` of the accuracy cases is ``2 max(2k + 1, 20)``: with ``b`` residual rows and ``b + 1`` free rows taken off the basis, the
default of the single-vector loop leaves a band of width 4 one or two block steps per cycle."""
import numpy as np
import pytest
import scipy.sparse
from test_trl_host import CASES, _matrix, reference

from lanczos_amd.eigsh import NumpyBackend, check_band_args, trl, trl_band, trl_filtered

DIAG = scipy.sparse.diags(np.repeat([1.0, 2.0, 3.0], 10)).tocsr()


@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("name,which,k", CASES[2:])
def test_band_loop_finds_the_wanted_eigenvalues(name, which, k, b):
    A, dense = _matrix(name)
    ref, nrm = reference(dense, which, k)
    be = NumpyBackend(A, block_size=b)
    theta, info = trl_band(be, dense.shape[0], k, which, b, ncv=2 * max(2 * k + 1, 20))
    assert np.all(np.diff(theta) >= 0)
    assert np.abs(theta - ref).max() <= 1e-12 * nrm
    assert be.residuals(k, theta).max() <= 1e-9 * nrm
    assert info["block_size"] == b and info["probes"] >= 1 and info["matvecs"] > 0


def _deuteron_wrong(b, probe):
    A, dense = _matrix("deuteron3d_N12_27pt_n100")
    ref, nrm = reference(dense, "SA", 6)
    n = dense.shape[0]
    wrong = 0
    for seed in range(20):
        v0 = np.random.default_rng(seed).standard_normal(n)
        theta, _ = trl_band(NumpyBackend(A, block_size=b), n, 6, "SA", b, ncv=20, v0=v0, probe=probe)
        wrong += bool(np.abs(theta - ref).max() > 1e-12 * nrm)
    return wrong


def test_a_band_as_wide_as_the_multiplicity_needs_no_probe():
    """the 6th lowest value of deuteron3d_N12 is one of three copies: a band of 3 finds them from any start, a band of 2 only with the probe"""
    assert _deuteron_wrong(3, probe=False) == 0
    assert _deuteron_wrong(2, probe=False) >= 1
    assert _deuteron_wrong(2, probe=True) == 0


@pytest.mark.parametrize("b,ncv", [(4, 60), (3, 61), (3, 40)])
def test_breakdowns_on_the_periodic_grid(b, ncv):
    A, dense = _matrix("lap2d_8x8_n2")
    ref, nrm = reference(dense, "SA", 6)
    theta, info = trl_band(NumpyBackend(A, block_size=b), 64, 6, "SA", b, ncv=ncv)
    assert np.abs(theta - ref).max() <= 1e-12 * nrm
    if ncv == 64 - b:  # the basis spans everything: the Krylov space must run out
        assert info["breakdowns"] >= 1


@pytest.mark.parametrize("b", [2, 4])
def test_breakdowns_on_three_distinct_values(b):
    theta, info = trl_band(NumpyBackend(DIAG, block_size=b), 30, 3, "SA", b)
    assert info["breakdowns"] >= 1
    assert np.abs(theta - 1.0).max() <= 1e-12 * 3


class _NoiseBehindBreakdown(NumpyBackend):
    """``extend_band`` as a device runs it: no synchronisation, so behind a vanished residual it goes on from whatever the division
    left - here a huge row that is orthogonal to nothing, or NaN"""

    def __init__(self, A, fill):
        super().__init__(A)
        self.fill = fill

    def extend_band(self, k, m):
        b = len(self.V) - m
        proj, beta = np.zeros((m, m + b)), np.zeros(m)
        for j in range(k, m):
            w = self._op(self.V[j])
            w, c = self._cgs(w, j + b - 1)
            w, c2 = self._cgs(w, j + b - 1)
            proj[j, : j + b] = c + c2
            beta[j] = np.linalg.norm(w)
            self.V[j + b] = w / beta[j] if beta[j] > 1e-14 else self.fill  # (a residual that vanished: they are below 6e-15 here)
        return proj, beta


@pytest.mark.parametrize("fill", [1e8, np.nan])
@pytest.mark.parametrize("b", [2, 4])
def test_what_lies_behind_a_breakdown_is_never_used(b, fill):
    theta, info = trl_band(_NoiseBehindBreakdown(DIAG, fill), 30, 3, "SA", b)
    assert info["breakdowns"] >= 1
    assert np.abs(theta - 1.0).max() <= 1e-12 * 3


@pytest.mark.parametrize("name,k", [("deuteron3d_N12_27pt_n100", 6), ("lap2d_32x32_n30", 10)])
def test_band_loop_on_the_chebyshev_filter(name, k):
    A, dense = _matrix(name)
    ref, nrm = reference(dense, "SA", k)
    theta, info = trl_filtered(NumpyBackend(A, block_size=2), dense.shape[0], k, "SA", 16, block_size=2)
    assert np.abs(theta - ref).max() <= 1e-12 * nrm
    assert info["block_size"] == 2 and info["filter"]["degree"] >= 2 and info["matvecs"] > info["steps"]


def test_argument_errors():
    for bad in (1, 9, 2.5, True):
        with pytest.raises(ValueError, match="block_size"):
            check_band_args(64, 6, "SA", None, bad)
        with pytest.raises(ValueError, match="block_size"):
            trl_band(NumpyBackend(DIAG), 30, 3, "SA", bad)
    assert check_band_args(64, 6, "SA", None, 3) == (20, 3)
    assert check_band_args(1000, 6, "SA", None, 8) == (23, 8)  # k + 2b + 1 above max(2k + 1, 20)
    assert check_band_args(24, 6, "SA", None, 4) == (20, 4)  # n - b
    assert check_band_args(64, 6, "SA", 13, 3) == (13, 3) and check_band_args(64, 6, "SA", 61, 3) == (61, 3)
    with pytest.raises(ValueError, match="k\\+2b\\+1<=ncv"):
        check_band_args(64, 6, "SA", 12, 3)
    with pytest.raises(ValueError, match="ncv"):
        check_band_args(64, 6, "SA", 62, 3)
    with pytest.raises(ValueError, match="ncv"):
        check_band_args(1000, 6, "SA", 129, 2)
    with pytest.raises(NotImplementedError, match="sigma"):
        check_band_args(64, 6, "LM", None, 2, sigma=0.5)
    with pytest.raises(TypeError):  # SciPy's own rules stay
        check_band_args(64, 64, "SA", None, 2)
    with pytest.raises(ValueError):
        check_band_args(64, 6, "XX", None, 2)


def test_eigsh_checks_block_size_before_it_touches_a_device():
    import lanczos_amd

    A, _ = _matrix("lap2d_8x8_n2")
    for bad in (1, 9, 2.5, True):
        with pytest.raises(ValueError, match="block_size"):
            lanczos_amd.eigsh(A, k=6, which="SA", block_size=bad)
    with pytest.raises(ValueError, match="ncv"):
        lanczos_amd.eigsh(A, k=6, which="SA", block_size=3, ncv=12)
    with pytest.raises(ValueError, match="ncv"):
        lanczos_amd.eigsh(A, k=6, which="SA", block_size=3, ncv=62)
    with pytest.raises(NotImplementedError, match="sigma"):
        lanczos_amd.eigsh(A, k=6, which="LM", sigma=1.0, filter_degree=16, block_size=2)
    with pytest.raises(NotImplementedError, match="sigma"):
        lanczos_amd.eigsh(A, k=6, which="LM", sigma=1.0, block_size=2)


def test_same_call_same_bits_and_the_global_rng_is_untouched():
    A, dense = _matrix("lap2d_32x32_n30")
    np.random.seed(7)
    before = np.random.get_state()
    a, ia = trl_band(NumpyBackend(A, block_size=2), dense.shape[0], 4, "SA", 2)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    b, ib = trl_band(NumpyBackend(A, block_size=2), dense.shape[0], 4, "SA", 2)
    assert np.array_equal(a, b) and ia == ib


def test_the_single_vector_loop_is_untouched_by_the_band_backend():
    """``block_size=None``: the NumPy backend's ``begin`` / ``extend`` / ``restart`` give ``trl`` what they gave before"""
    A, dense = _matrix("lap2d_32x32_n30")
    a, _ = trl(NumpyBackend(A), dense.shape[0], 4, "SA")
    b, _ = trl(NumpyBackend(A, block_size=None), dense.shape[0], 4, "SA")
    assert np.array_equal(a, b)
