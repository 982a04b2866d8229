"""Band (block) thick-restart Lanczos on the device: one batch of lz_trl_extend_band against the NumPy band backend, the band restart,
eigsh(block_size=...) against dense eigvalsh, the copies of a 3-fold eigenvalue, breakdowns, the Chebyshev filter under the band loop."""
import numpy as np
import pytest
import scipy.sparse
from test_trl_host import CASES, _matrix, reference

import lanczos_amd
from lanczos_amd import _capi
from lanczos_amd.eigsh import DeviceBackend, NumpyBackend, trl, trl_band, upload_matrix

pytestmark = pytest.mark.gpu


def stencil1d(rows):
    """a 1-D three-point stencil with a varying diagonal; its infinity norm bounds |A|"""
    d = 2.0 + 0.25 * np.cos(np.arange(rows))
    A = scipy.sparse.diags([-np.ones(rows - 1), d, -np.ones(rows - 1)], [-1, 0, 1]).tocsr()
    return A, float(abs(A).sum(axis=1).max())


def orthonormal_rows(rows, count, pad):
    """``count`` orthonormal random rows of length ``rows`` (host QR) at the top of a zero ``(count, pad)`` array"""
    V = np.zeros((count, pad))
    V[:, :rows] = np.linalg.qr(np.random.default_rng(rows + count).standard_normal((rows, count)))[0].T
    return V


def band_handle(A, m, b):
    rows = A.shape[0]
    h = _capi.Handle(0)
    h.set_csr(rows, 0, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data)
    h.trl_begin_band(m, np.random.default_rng(b).standard_normal((b, rows)))
    return h


def run_batches(rows, k, m, b):
    """rows 0 .. k + b of a band basis set from the host, ``extend_band(k, m)`` on the device and in NumPy from the same rows"""
    A, nrm = stencil1d(rows)
    h = band_handle(A, m, b)
    pad = h.padded_rows(rows)
    V = orthonormal_rows(rows, k + b, pad)
    h.trl_set_rows(0, V)
    proj, beta = h.trl_extend_band(k, m)
    out = h.trl_get_rows(0, m + b)
    h.close()
    be = NumpyBackend(A, block_size=b)
    be.V = np.zeros((m + b, rows))
    be.V[: k + b] = V[:, :rows]
    pr, bt = be.extend_band(k, m)
    print(f"rows={rows} k={k} m={m} b={b}: proj {np.abs(proj[k:] - pr[k:]).max() / nrm:.2e} beta {np.abs(beta[k:] - bt[k:]).max() / nrm:.2e} |A|, "
          f"rows {max(np.abs(out[r, :rows] - be.V[r]).max() / np.abs(be.V[r]).max() for r in range(k + b, m + b)):.2e}")
    assert proj.shape == (m, m + b)
    assert np.abs(proj[k:] - pr[k:]).max() <= 1e-12 * nrm
    assert np.abs(beta[k:] - bt[k:]).max() <= 1e-12 * nrm
    for r in range(k + b, m + b):
        assert np.abs(out[r, :rows] - be.V[r]).max() <= 1e-10 * np.abs(be.V[r]).max(), r
    assert np.all(out[k + b:, rows:] == 0.0)  # the padding of every row written
    assert np.array_equal(out[: k + b], V)  # the rows below are only read


@pytest.mark.parametrize("r0,b", [(2, 2), (5, 3), (17, 4), (33, 8), (120, 8)])
@pytest.mark.parametrize("rows", [40, 1000, 4099, 1_000_003])
def test_one_batch_matches_numpy(rows, r0, b):
    run_batches(max(rows, r0 + b), r0 - b, r0, b)  # m = r0: steps r0 - b .. r0 - 1 are exactly one batch


@pytest.mark.parametrize("rows,k,m,b", [(1000, 8, 12, 3), (4099, 0, 6, 5)])
def test_a_full_batch_and_a_batch_of_one(rows, k, m, b):
    assert m - k == b + 1
    run_batches(rows, k, m, b)


@pytest.mark.parametrize("m,kk,b", [(20, 10, 2), (41, 30, 4), (128, 100, 8)])
@pytest.mark.parametrize("rows", [1000, 4099])
def test_band_restart(m, kk, b, rows):
    h = band_handle(scipy.sparse.identity(rows, format="csr"), m, b)
    pad = h.padded_rows(rows)
    rng = np.random.default_rng(rows + m)
    V = np.zeros((m + b, pad))
    V[:, :rows] = rng.standard_normal((m + b, rows))
    h.trl_set_rows(0, V)
    S = rng.standard_normal((m, kk))
    h.trl_restart(m, kk, S)
    out = h.trl_get_rows(0, m + b)
    h.close()
    ref = S.T @ V[:m, :rows]
    assert np.abs(out[:kk, :rows] - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.array_equal(out[kk: kk + b], V[m: m + b])  # all b residual rows moved down, bit for bit
    assert np.array_equal(out[kk + b: m], V[kk + b: m])  # the rows between are untouched
    assert np.all(out[:, rows:] == 0.0)


@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("name,which,k", CASES)
def test_band_eigsh_on_the_device(name, which, k, b):
    A, dense = _matrix(name)
    ref, nrm = reference(dense, which, k)
    v0 = np.random.default_rng(3).standard_normal(dense.shape[0])
    ncv = 2 * max(2 * k + 1, 20)  # (as the host tests: the default leaves a band of 4 a step or two per cycle)
    h = _capi.Handle(0)
    info = {}
    theta, Y = lanczos_amd.eigsh(A, k=k, which=which, v0=v0, ncv=ncv, handle=h, info=info, block_size=b)
    res = np.linalg.norm(dense @ Y - Y * theta, axis=0)
    print(f"{name} {which} k={k} b={b}: values {np.abs(theta - ref).max() / nrm:.2e} residuals {res.max() / nrm:.2e} |A|, "
          f"steps {info['matvecs']} cycles {info['cycles']}")
    assert info["block_size"] == b
    assert np.all(np.diff(theta) >= 0)
    assert np.abs(theta - ref).max() <= 1e-10 * nrm
    assert res.max() <= 1e-9 * nrm
    assert np.abs(Y.T @ Y - np.eye(k)).max() <= 1e-12
    assert np.abs(info["residuals"] - res).max() <= 1e-12 * nrm
    theta2, Y2 = lanczos_amd.eigsh(A, k=k, which=which, v0=v0, ncv=ncv, handle=h, block_size=b)
    assert np.array_equal(theta, theta2) and np.array_equal(Y, Y2)  # same v0, same bits
    h.close()


def test_a_band_of_three_finds_the_three_copies_without_the_probe():
    A, dense = _matrix("deuteron3d_N12_27pt_n100")
    ref, nrm = reference(dense, "SA", 6)
    h = _capi.Handle(0)
    n = upload_matrix(h, A)
    wrong = 0
    for seed in range(20):
        v0 = np.random.default_rng(seed).standard_normal(n)
        if seed < 5:
            theta, info = trl_band(DeviceBackend(h, n, block_size=3), n, 6, "SA", 3, ncv=20, v0=v0, probe=False)
            assert info["probes"] == 0
            assert np.abs(theta - ref).max() <= 1e-10 * nrm, seed
        elif wrong:  # (seeds 5 .. 19 only when rounding rescued the single-vector loop on all of 0 .. 4)
            break
        theta, _ = trl(DeviceBackend(h, n), n, 6, "SA", ncv=20, v0=v0, probe=False)
        wrong += bool(np.abs(theta - ref).max() > 1e-10 * nrm)
    h.close()
    assert wrong >= 1  # one Krylov vector sees one copy


def test_band_breakdowns_on_the_device():
    """both Krylov spaces run out before the basis is full: 4 start vectors reach at most 4 x (distinct eigenvalues) dimensions"""
    A, dense = _matrix("lap2d_8x8_n2")
    ref, nrm = reference(dense, "SA", 6)
    info = {}
    theta = lanczos_amd.eigsh(A, k=6, which="SA", ncv=60, block_size=4, return_eigenvectors=False, info=info)
    print("lap2d_8x8:", info["breakdowns"], "breakdowns,", np.abs(theta - ref).max() / nrm)
    assert np.abs(theta - ref).max() <= 1e-10 * nrm
    assert info["breakdowns"] >= 1
    D = scipy.sparse.diags(np.repeat([1.0, 2.0, 3.0], 10)).tocsr()
    for b in (2, 4):
        info = {}
        theta = lanczos_amd.eigsh(D, k=3, which="SA", block_size=b, return_eigenvectors=False, info=info)
        assert np.abs(theta - 1.0).max() <= 1e-10 * 3
        assert info["breakdowns"] >= 1


@pytest.mark.parametrize("name,k", [("deuteron3d_N12_27pt_n100", 6), ("lap2d_32x32_n30", 10)])
def test_band_loop_on_the_filter_fused_and_unfused(name, k):
    A, dense = _matrix(name)
    ref, nrm = reference(dense, "SA", k)
    out = []
    for flags in (0, _capi.FLAG_TRL_FILTER_UNFUSED):
        h = _capi.Handle(0)
        h.set_options(flags)
        info = {}
        theta, Y = lanczos_amd.eigsh(A, k=k, which="SA", handle=h, info=info, filter_degree=16, block_size=2)
        h.close()
        assert info["block_size"] == 2 and info["filter"]["degree"] >= 2
        assert np.abs(theta - ref).max() <= 1e-10 * nrm
        assert np.linalg.norm(dense @ Y - Y * theta, axis=0).max() <= 1e-9 * nrm
        out.append((theta, Y))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_band_state_errors():
    A, _ = stencil1d(100)
    h = band_handle(A, 10, 2)
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):
        h.trl_extend(0, 10)  # a band basis
    h.trl_begin(10, np.ones(100))
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):
        h.trl_extend_band(0, 10)  # begun without a band
    for m, b in [(10, 1), (10, 9), (99, 2), (1, 2)]:
        with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_ARG"):
            h.trl_begin_band(m, np.ones((b, 100)))
    h.trl_begin_band(10, np.random.default_rng(0).standard_normal((2, 100)))
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_ARG"):
        h.trl_probe(12, np.ones(100))  # rows 0 .. m + b - 1
    h.trl_probe(11, np.random.default_rng(1).standard_normal(100))
    assert h.trl_get_rows(0, 12).shape[0] == 12
    h.close()
