"""lanczos_amd.eigsh on the device: thick-restart Lanczos (lz_trl_* in include/lanczos_hip.h) against dense eigvalsh, the restart
kernel against NumPy, the DGKS gate against the forced second pass, breakdowns, the drop-in's exact_eigs = "device"."""
import os

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg
from conftest import load_golden
from test_trl_host import CASES, _matrix, reference

import lanczos_amd
from lanczos_amd import Hamiltonian, Lanczos, _capi, synthetic
from lanczos_amd.eigsh import DeviceBackend, trl, upload_matrix

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,which,k", CASES)
def test_eigsh_on_the_device(name, which, k):
    A, dense = _matrix(name)
    ref, nrm = reference(dense, which, k)
    v0 = np.random.default_rng(3).standard_normal(dense.shape[0])
    h = _capi.Handle(0)
    info = {}
    theta, Y = lanczos_amd.eigsh(A, k=k, which=which, v0=v0, handle=h, info=info)
    assert np.all(np.diff(theta) >= 0)
    assert np.abs(theta - ref).max() <= 1e-10 * nrm
    res = np.linalg.norm(dense @ Y - Y * theta, axis=0)
    assert res.max() <= 1e-9 * nrm
    assert np.abs(Y.T @ Y - np.eye(k)).max() <= 1e-12
    assert np.abs(info["residuals"] - res).max() <= 1e-12 * nrm
    theta2, Y2 = lanczos_amd.eigsh(A, k=k, which=which, v0=v0, handle=h)
    assert np.array_equal(theta, theta2) and np.array_equal(Y, Y2)  # same v0, same bits
    h.close()


@pytest.mark.parametrize("m,kk", [(20, 10), (41, 30), (64, 63), (128, 100)])
@pytest.mark.parametrize("rows", [1, 17, 1000, 4099, 1_000_003])
def test_restart_kernel_matches_numpy(m, kk, rows):
    if rows < m:  # the basis needs m rows at least (lz_trl_begin): the kernel is the same, test it on a matrix of m rows
        rows = m + rows
    h = _capi.Handle(0)
    D = scipy.sparse.identity(rows, format="csr")
    h.set_csr(rows, 0, D.indptr.astype(np.int32), D.indices.astype(np.int32), D.data)
    h.trl_begin(m, np.ones(rows))
    pad = h.padded_rows(rows)
    rng = np.random.default_rng(rows + m)
    V = np.full((m + 1, pad), np.nan)
    V[:, :rows] = rng.standard_normal((m + 1, rows))
    h.trl_set_rows(0, V)
    S = rng.standard_normal((m, kk))
    h.trl_restart(m, kk, S)
    out = h.trl_get_rows(0, m + 1)
    ref = S.T @ V[:m, :rows]
    scale = np.abs(ref).max()
    assert np.abs(out[:kk, :rows] - ref).max() <= 1e-13 * scale
    assert np.array_equal(out[kk, :rows], V[m, :rows])  # V[m] moved to V[kk]
    assert np.array_equal(out[kk + 1:, :rows], V[kk + 1:, :rows])  # the other rows >= kk untouched
    assert np.isnan(out[:, rows:]).all()  # padding untouched
    h.close()


def test_gated_and_forced_second_pass_agree():
    A, dense = _matrix("deuteron3d_N12_27pt_n100")
    ref, nrm = reference(dense, "SA", 10)
    out = []
    for force in (False, True):
        h = _capi.Handle(0)
        n = upload_matrix(h, A)
        theta, _ = trl(DeviceBackend(h, n, force_second_pass=force), n, 10, "SA")
        out.append(theta)
        h.close()
    assert np.abs(out[0] - out[1]).max() <= 1e-12 * nrm
    assert np.abs(out[0] - ref).max() <= 1e-10 * nrm


def test_breakdowns_on_the_device():
    A, dense = _matrix("lap2d_8x8_n2")
    ref, nrm = reference(dense, "SA", 6)
    theta = lanczos_amd.eigsh(A, k=6, which="SA", ncv=64, return_eigenvectors=False)
    assert np.abs(theta - ref).max() <= 1e-10 * nrm
    D = scipy.sparse.diags(np.repeat([1.0, 2.0, 3.0], 10)).tocsr()
    theta = lanczos_amd.eigsh(D, k=3, which="SA", return_eigenvectors=False)
    assert np.abs(theta - 1.0).max() <= 1e-10 * 3


def test_exact_eigs_on_the_device(monkeypatch):
    _, H = load_golden("deuteron1d_N1001_n1001")
    Lanczos.verbose = False
    ref = np.sort(scipy.sparse.linalg.eigsh(H, k=20, which="SM")[0])
    nrm = scipy.sparse.linalg.eigsh(H, k=1, which="LM", return_eigenvectors=False)[0]
    s = Lanczos(H)
    s.exact_eigs = "device"
    got = np.sort(s.H_eigvals_actual)
    assert np.abs(got - ref).max() <= 1e-10 * abs(nrm)
    assert s.H_eigvecs_actual.shape == (1001, 20)
    s.close()
    calls = []
    real = scipy.sparse.linalg.eigsh

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(scipy.sparse.linalg, "eigsh", spy)
    d = Lanczos(H)  # default: SciPy still runs
    d.find_exact_eigs(4)
    assert len(calls) == 1
    multi = Lanczos(H)
    multi.devices = [0, 0]
    multi.exact_eigs = "device"
    with pytest.raises(ValueError, match="one GPU"):
        multi.find_exact_eigs(4)


def test_deuteron_hamiltonian_on_the_device():
    Hamiltonian.verbose = Lanczos.verbose = False
    N = 100
    os.makedirs("T_matrices", exist_ok=True)
    ham = Hamiltonian(N, 25, synthetic.DeuteronPotential(), 197.327**2 / (2 * 469.4592) / (25.0 / N) ** 2)
    ham.device_potential = True
    op = ham.operator("27")
    h = _capi.Handle(0)
    n = upload_matrix(h, op)
    free0, _ = h.device_memory()
    be = DeviceBackend(h, n)
    theta, info = trl(be, n, 4, "SA")
    free1, _ = h.device_memory()
    ncv = 20
    assert free0 - free1 <= (ncv + 1) * h.padded_rows(n) * 8 + (64 << 20)
    nrm = info["anorm"]
    res = h.trl_residuals(4, theta)
    h.close()
    s = Lanczos(op)
    s.execute_Lanczos(300, seed=1)
    lowest = np.min(s.H_eigvals)
    s.close()
    assert theta[0] <= lowest + 1e-10 * abs(lowest)
    assert res.max() <= 1e-9 * nrm


def test_max_iterations_and_state_errors():
    A, dense = _matrix("deuteron1d_N1001_n1001")
    with pytest.raises(scipy.sparse.linalg.ArpackNoConvergence) as e:
        lanczos_amd.eigsh(A, k=20, which="SM", maxiter=1)
    assert len(e.value.eigenvalues) < 20 and e.value.eigenvectors.shape == (1001, len(e.value.eigenvalues))
    h = _capi.Handle(0)
    upload_matrix(h, A)
    h.set_options(_capi.FLAG_REORTH_PARTIAL)
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):
        h.trl_begin(20, np.ones(1001))
    h.close()
