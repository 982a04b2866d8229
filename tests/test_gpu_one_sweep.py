"""The one-sweep loop (lz_last_engine 9, run_loop_one_sweep): one walk over the basis per step, the coefficients predicted
from V^T V and checked in the same walk.  Forced at small sizes (TUNE_LOOP = 6) and compared with the six-launch loop
(TUNE_LOOP = 1): equal to rounding on the coefficients and vectors the reference arithmetic itself determines, an
orthogonal basis, bit-identical reruns, and the correcting sweep on a case whose prediction cannot hold."""
import numpy as np
import pytest
import scipy.sparse

from conftest import load_golden
from lanczos_amd import _capi, synthetic
from oracle import lanczos_ref as oracle

pytestmark = pytest.mark.gpu

ONE_SWEEP = 6


def _run(hip, H, n, knob):
    A = H.tocsr()
    h = hip.Handle(0)
    h.set_options(hip.FLAG_FUSED_NORM)
    h.set_tuning(_capi.TUNE_LOOP, knob)
    h.set_csr(A.shape[0], 0, A.indptr, A.indices, A.data)
    v0 = synthetic.reference_start_vector(A.shape[0])
    v0 /= np.linalg.norm(v0)
    a, b = h.run(n, v0)
    out = (np.array(a), np.array(b), h.get_basis(), h.last_engine(), h.last_gate_trips())
    h.close()
    return out


def _cases():
    return {
        "lap2d_64x48_n60": (synthetic.laplacian_2d_5pt(64, 48).to_scipy(), 60),
        "lap3d_10x9x8_n40": (synthetic.laplacian_3d_7pt(10, 9, 8).to_scipy(), 40),
        "ragged_M700_n25": (load_golden("ragged_M700_n25")[1], 25),
        "graph_M2000_E7000_n40": (load_golden("graph_M2000_E7000_n40")[1], 40),
        "deuteron3d_N12_27pt_n100": (load_golden("deuteron3d_N12_27pt_n100")[1], 100),
    }


@pytest.mark.parametrize("name", list(_cases()))
def test_one_sweep_equals_two_pass_to_rounding(hip, name):
    H, n = _cases()[name]
    a1, b1, V1, eng1, _ = _run(hip, H, n, 1)
    a2, b2, V2, eng2, trips = _run(hip, H, n, ONE_SWEEP)
    assert eng1 == "kernels" and eng2 == "one-sweep"
    scale = np.abs(np.linalg.eigvalsh(oracle.build_h_eff(a1, b1))).max()
    # compare what the reference arithmetic determines: the prefix a reordered evaluation reproduces to 1e-13 of the scale
    prefix, _ = oracle.stable_masks(H, n, a1, b1, tol=1e-13)
    rows = oracle.stable_basis_rows(H, n, V1, tol=1e-13)
    assert prefix >= min(n, 20) and rows >= min(n, 20), (prefix, rows)
    assert np.abs(a2 - a1)[:prefix].max() <= 1e-12 * scale
    assert np.abs(b2 - b1)[: prefix - 1].max() <= 1e-12 * scale
    assert np.abs(V2 - V1)[:rows].max() <= 1e-12 * scale
    k = min(prefix, rows)
    assert np.abs(V2[:k] @ V2[:k].T - np.eye(k)).max() < 1e-13
    print(f"\n[{name}] prefix {prefix}, rows {rows}, gate trips {trips}, max |dalpha| {np.abs(a2 - a1)[:prefix].max():.1e}")


def test_one_sweep_rerun_is_bit_identical_and_orthogonal(hip):
    H, n = _cases()["lap2d_64x48_n60"]
    a1, b1, V1, eng, trips = _run(hip, H, n, ONE_SWEEP)
    a2, b2, V2, _, trips2 = _run(hip, H, n, ONE_SWEEP)
    assert eng == "one-sweep" and trips == 0 and trips2 == 0
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2) and np.array_equal(V1, V2)
    assert np.abs(V1 @ V1.T - np.eye(n)).max() < 1e-13


def test_gate_trips_and_correction_keeps_the_basis_orthogonal(hip):
    # A slightly non-symmetric operator: the prediction uses A = A^T and misses by ~1e-9 at every step, so every step
    # after the first runs the correcting sweep.  The basis must still come out orthogonal, and the coefficients stay
    # those of the two-pass loop (which measures every dot) to the size of the asymmetry.
    L = synthetic.laplacian_2d_5pt(40, 30).to_scipy().tocsr()
    rng = np.random.default_rng(5)
    S = scipy.sparse.random(L.shape[0], L.shape[0], density=4.0 / L.shape[0], random_state=rng, format="csr")
    H = (L + 1e-9 * (S - S.T)).tocsr()
    n = 30
    a1, b1, V1, _, _ = _run(hip, H, n, 1)
    a2, b2, V2, eng, trips = _run(hip, H, n, ONE_SWEEP)
    assert eng == "one-sweep"
    assert trips >= n // 2, trips
    assert np.abs(V2 @ V2.T - np.eye(n)).max() < 1e-13
    assert np.abs(a2 - a1).max() < 1e-7 and np.abs(b2 - b1).max() < 1e-7
