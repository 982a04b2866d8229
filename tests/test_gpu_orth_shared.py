"""The thick-restart solver and the Golub-Kahan-Lanczos solver orthogonalise through one code path (lanczos_amd/csrc/lz_orth.hip):
the same rows and the same vector give the same bits in lz_trl_probe's basis and in lz_gk_probe's V side, padding included.

One handle holds a square symmetric matrix twice, as the square operator (lz_set_csr) and as the rectangular one with p = q
(lz_gk_set_csr), so both bases have the same row length, stride and plan.  No product runs: what is compared is orth_store alone -
k = 0 its norm-only branch, k = 8 the last row but one of an m = 9 basis - and the two row transfers.

What this guards: with both solvers on one helper the equality holds by construction, so the test fails when the helper is forked
again (or when one solver's plan, stride or small-array head drifts from the other's), not when the helper itself is wrong.  Whether
its numbers are right is the business of tests/test_gpu_trl*.py and tests/test_gpu_svds*.py, which compare with NumPy."""
import numpy as np
import pytest
import scipy.sparse

from lanczos_amd import _capi

pytestmark = pytest.mark.gpu
M_BASIS = 9


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()  # (NaN positions and signed zeros included)


@pytest.fixture(scope="module", params=[1000, 4099])
def both(request):
    """(handle, rows): the matrix set for both solvers, both bases begun from the same vector"""
    n = request.param
    rng = np.random.default_rng(n)
    R = scipy.sparse.random(n, n, density=4.0 / n, random_state=rng, format="csr")
    A = (R + R.T + scipy.sparse.identity(n)).tocsr()
    A.sort_indices()
    h = _capi.Handle(0)
    h.set_csr(n, 0, A.indptr, A.indices, A.data)
    h.gk_set_csr(A, A)
    v0 = rng.standard_normal(n)
    h.trl_begin(M_BASIS, v0)
    h.gk_begin(M_BASIS, v0)
    yield h, n
    h.close()


@pytest.mark.parametrize("k", [0, 1, 8])
def test_probe_gives_the_same_bits_in_both_solvers(both, k):
    h, n = both
    pad = h.padded_rows(n)
    rng = np.random.default_rng(100 * n + k)
    if k > 0:
        rows = np.zeros((k, pad))
        rows[:, :n] = rng.standard_normal((k, n)) / np.sqrt(n)  # (not orthonormal: the coefficients of both passes are of order one)
        h.trl_set_rows(0, rows)
        h.gk_set_rows(1, 0, rows)
    x = rng.standard_normal(n)
    h.trl_probe(k, x)
    h.gk_probe(1, k, x)
    t, g = h.trl_get_rows(0, k + 1), h.gk_get_rows(1, 0, k + 1)
    assert t.shape == (k + 1, pad)
    assert np.isfinite(t).all() and abs(np.linalg.norm(t[k]) - 1.0) < 1e-12  # a real row, not two empty buffers
    assert not t[k, n:].any()
    if k > 0:
        assert same_bits(t[:k], rows)
    assert same_bits(t, g)
    assert same_bits(h.trl_get_vectors(k + 1), h.gk_get_vectors(1, k + 1))
    assert same_bits(h.trl_get_vectors(k + 1), np.ascontiguousarray(t[:, :n].T))
