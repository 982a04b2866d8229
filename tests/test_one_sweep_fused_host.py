"""The arithmetic of the fused one-sweep loop (run_loop_one_sweep_fused), checked without a GPU on its NumPy prototype
(tools/one_sweep_prototype.py, one_sweep_fused_lanczos): working in the units of w with the self term 1 and normalising the
measured and the predicted dots afterwards gives the two-pass recurrence's coefficients and basis to rounding, the prediction's
leftover stays under the gate, and the correcting sweep on u~ keeps the basis orthogonal when the prediction cannot hold."""
import os
import sys

import numpy as np
import pytest

from lanczos_amd import synthetic

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import one_sweep_prototype as proto  # noqa: E402


def _asym_5pt():
    L = synthetic.laplacian_2d_5pt(40, 30).to_scipy().tocsr()
    off = L.copy()
    off.setdiag(0.0)
    off.eliminate_zeros()
    P = off.copy()
    P.data = np.random.default_rng(5).uniform(-1.0, 1.0, size=P.nnz)
    return (L + 1e-9 * (P - P.T)).tocsr()


@pytest.mark.parametrize("name,n", [("lap2d_64x48", 60), ("lap2d_33x31", 40), ("lap3d_10x9x8", 40), ("lap2d_64x48", 2), ("lap2d_64x48", 3)])
def test_fused_prototype_equals_two_pass_to_rounding(name, n):
    dims = tuple(int(x) for x in name.split("_")[1].split("x"))
    H = (synthetic.laplacian_2d_5pt(*dims) if len(dims) == 2 else synthetic.laplacian_3d_7pt(*dims)).to_scipy()
    v0 = synthetic.reference_start_vector(H.shape[0])
    a, b, V, st = proto.one_sweep_fused_lanczos(H, n, v0=v0)
    a0, b0, V0 = proto.two_pass_lanczos(H, n, v0=v0)
    scale = np.abs(proto.tridiag_eigs(a0, b0)).max()
    k = min(n, 25)  # (well inside the prefix a reordered two-pass evaluation reproduces)
    assert st["trips"] == [] and st["emax"].max() < 1e-14
    assert np.abs(a - a0)[:k].max() <= 1e-12 * scale and np.abs(b - b0)[: k - 1].max() <= 1e-12 * scale
    assert np.abs(V - V0)[:k].max() <= 1e-12 * scale
    assert np.abs(V[:k] @ V[:k].T - np.eye(k)).max() < 1e-13


def test_fused_prototype_corrects_a_prediction_that_cannot_hold():
    H, n = _asym_5pt(), 30
    v0 = synthetic.reference_start_vector(H.shape[0])
    a, b, V, st = proto.one_sweep_fused_lanczos(H, n, v0=v0)
    a0, b0, _ = proto.two_pass_lanczos(H, n, v0=v0)
    assert len(st["trips"]) >= n // 2
    assert np.abs(V @ V.T - np.eye(n)).max() < 1e-13
    assert np.abs(a - a0).max() < 1e-7 and np.abs(b - b0).max() < 1e-7
