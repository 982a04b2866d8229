"""lz_trl_extend_band against longdouble: one call on rows set from the host under the reference's derived bounds
(tests/band_reference.py; the cases and what makes them decisive: tests/test_band_step_host.py) at every band width and both row
lengths of the update kernel, at the tile edges of the dots walk, with the dots kernel's LDS at and past 64 KiB, over several batches
with a short last one and on the second trip of the persistent slice loop; the rows the call is to write hold NaN before it, so a read
past ``r0`` shows.  Then a handle reused across a shrinking run, the bits of two fresh handles, and ``eigsh`` at the widths 5, 6, 7."""
import numpy as np
import pytest
from band_reference import extension
from test_band_step_host import BAND_CASES, Case, case_id, errors, inputs
from test_trl_host import _matrix, reference

import lanczos_amd
from lanczos_amd import _capi

pytestmark = pytest.mark.gpu


def band_handle(A, m, b):
    n = A.shape[0]
    h = _capi.Handle(0)
    h.set_csr(n, 0, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data)
    h.trl_begin_band(m, np.random.default_rng(b).standard_normal((b, n)))
    return h


def one_call(h, case, label, ref=None):
    """rows ``0 .. k + b - 1`` set from the host, NaN in the rows above, ``extend_band(k, m)``: everything it returns under the bounds of
    the reference evaluated on the basis it left (``ref``: that reference, where the caller knows the basis to be the same bits)"""
    n, k, m, b = case.n, case.k, case.m, case.b
    A, rows = inputs(case)
    pad = h.padded_rows(n)
    V = np.zeros((m + b, pad))
    V[: k + b, :n] = rows
    V[k + b:, :n] = np.nan
    h.trl_set_rows(0, V)
    proj, beta = h.trl_extend_band(k, m)
    out = h.trl_get_rows(0, m + b)
    assert proj.shape == (m, m + b)
    assert np.all(np.isfinite(proj[k:])) and np.all(np.isfinite(beta[k:])) and np.all(np.isfinite(out[k + b:]))
    if ref is None:
        ref = extension(A, out[:, :n], k, m, b)
    err = errors(case, ref, proj, beta, out)
    print(f"{label:44s} error / bound: " + " ".join(f"{key} {v:.2e}" for key, v in err.items()))
    assert all(v <= 1.0 for v in err.values()), err
    assert np.array_equal(out[: k + b], V[: k + b])  # the rows below are only read
    assert np.all(out[k + b:, n:] == 0.0)  # the padding of every row written
    assert all(not proj[j, j + b:].any() for j in range(k, m))
    return proj, beta, out, ref


@pytest.mark.parametrize("case", BAND_CASES, ids=case_id)
def test_one_call_within_the_reference_bounds(case):
    h = band_handle(inputs(case)[0], case.m, case.b)
    one_call(h, case, case_id(case))
    h.close()


def test_a_handle_reused_across_a_shrinking_run():
    """a run with the LDS attribute raised, then a small batch of another width on the same handle (a shorter run, the attribute
    still raised) and once more without a begin between (stale work vectors), then the first again: each within its bounds, the runs
    of the same case the same bits"""
    big, small = Case(1501, 121, 128, 8, "skew", 16), Case(1501, 6, 13, 7, "skew")
    assert big in BAND_CASES and small in BAND_CASES
    A = inputs(big)[0]
    h = band_handle(A, big.m, big.b)
    first = one_call(h, big, case_id(big) + " (first)")
    h.trl_begin_band(small.m, np.random.default_rng(7).standard_normal((small.b, small.n)))
    once = one_call(h, small, case_id(small) + " (same handle)")
    twice = one_call(h, small, case_id(small) + " (no begin between)", ref=once[3])  # the work vectors hold what the last call left
    assert all(np.array_equal(x, y) for x, y in zip(once[:3], twice[:3]))
    h.trl_begin_band(big.m, np.random.default_rng(8).standard_normal((big.b, big.n)))
    again = one_call(h, big, case_id(big) + " (again)", ref=first[3])
    h.close()
    assert all(np.array_equal(x, y) for x, y in zip(first[:3], again[:3]))


def test_two_fresh_handles_give_the_same_bits():
    """the summation order is fixed (wave order, then block order, no atomics): several batches, twice"""
    case = Case(1501, 3, 20, 6, "skew")
    assert case in BAND_CASES
    runs = []
    for _ in range(2):
        h = band_handle(inputs(case)[0], case.m, case.b)
        runs.append(one_call(h, case, case_id(case) + " (fresh handle)", ref=runs[0][3] if runs else None))
        h.close()
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][:3], runs[1][:3]))


@pytest.mark.parametrize("b", [5, 6, 7])
def test_band_eigsh_at_the_widths_five_to_seven(b):
    """under the bars of test_gpu_trl_band.py::test_band_eigsh_on_the_device"""
    name, which, k = "lap2d_32x32_n30", "SA", 6
    A, dense = _matrix(name)
    ref, nrm = reference(dense, which, k)
    v0 = np.random.default_rng(3).standard_normal(dense.shape[0])
    h = _capi.Handle(0)
    info = {}
    theta, Y = lanczos_amd.eigsh(A, k=k, which=which, v0=v0, ncv=40, handle=h, info=info, block_size=b)
    h.close()
    res = np.linalg.norm(dense @ Y - Y * theta, axis=0)
    print(f"{name} {which} k={k} b={b}: values {np.abs(theta - ref).max() / nrm:.2e} residuals {res.max() / nrm:.2e} |A|, "
          f"steps {info['matvecs']} cycles {info['cycles']}")
    assert info["block_size"] == b
    assert np.all(np.diff(theta) >= 0)
    assert np.abs(theta - ref).max() <= 1e-10 * nrm
    assert res.max() <= 1e-9 * nrm
    assert np.abs(Y.T @ Y - np.eye(k)).max() <= 1e-12
    assert np.abs(info["residuals"] - res).max() <= 1e-12 * nrm
