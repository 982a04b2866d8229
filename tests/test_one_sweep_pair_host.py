"""The arithmetic of the pair form of the one-sweep loop (run_loop_one_sweep_pair), checked without a GPU on its NumPy prototype
(tools/one_sweep_prototype.py, one_sweep_pair_lanczos): one walk over the basis finishes v_j and forms u~_{j+1}, the correction
step j owes to w_{j+1} being applied as a combination of basis rows.  The pair form gives the two-pass recurrence's coefficients
and basis to rounding (the bars of tests/test_one_sweep_fused_host.py), both leftovers of every pair stay under the gate, the
bookkept Gram matrix is honest, and a matrix whose predictions cannot hold marks the run as abandoned."""
import os
import sys

import numpy as np
import pytest

from lanczos_amd import synthetic

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import one_sweep_prototype as proto  # noqa: E402

TAU = 1e-14


def _asym_5pt():
    L = synthetic.laplacian_2d_5pt(40, 30).to_scipy().tocsr()
    off = L.copy()
    off.setdiag(0.0)
    off.eliminate_zeros()
    P = off.copy()
    P.data = np.random.default_rng(5).uniform(-1.0, 1.0, size=P.nnz)
    return (L + 1e-9 * (P - P.T)).tocsr()


def _check(H, n, v0, exhausted_at=None):
    a, b, V, st = proto.one_sweep_pair_lanczos(H, n, v0=v0, tau=TAU)
    a0, b0, V0 = proto.two_pass_lanczos(H, n, v0=v0)
    scale = np.abs(proto.tridiag_eigs(a0, b0)).max()
    k = min(n, 25)  # (well inside the prefix a reordered two-pass evaluation reproduces)
    m = n if exhausted_at is None else exhausted_at  # the steps before the Krylov space is exhausted
    assert st["pairs"] == max(n - 2, 0) // 2
    assert max(st["e1"][:m].max(), st["e2"][:m].max()) < TAU
    assert st["trips"] == []
    if exhausted_at is None:
        assert not st["abandoned"]
    else:
        assert st["abandoned"]
    assert np.abs(st["G"][:m, :m] - V[:m] @ V[:m].T).max() < 1e-14
    k = min(k, m)
    assert np.abs(a - a0)[:k].max() <= 1e-12 * scale and np.abs(b - b0)[: k - 1].max() <= 1e-12 * scale
    assert np.abs(V - V0)[:k].max() <= 1e-12 * scale
    assert np.abs(V[:k] @ V[:k].T - np.eye(k)).max() < 1e-13


@pytest.mark.parametrize("name,n", [("lap2d_64x48", 60), ("lap2d_64x48", 61), ("lap2d_33x31", 41), ("lap2d_33x31", 40),
                                    ("lap3d_10x9x8", 40), ("lap2d_64x48", 3), ("lap2d_64x48", 4), ("lap2d_64x48", 5)])
def test_pair_prototype_equals_two_pass_to_rounding(name, n):
    dims = tuple(int(x) for x in name.split("_")[1].split("x"))
    H = (synthetic.laplacian_2d_5pt(*dims) if len(dims) == 2 else synthetic.laplacian_3d_7pt(*dims)).to_scipy()
    _check(H, n, synthetic.reference_start_vector(H.shape[0]))


@pytest.mark.parametrize("fixture", ["lap2d_32x32_n30", "graph_M2000_E7000_n40", "deuteron3d_N12_27pt_n100", "ragged_M700_n25",
                                     "box1d_N500_n50", "c1_dense512_n20"])
def test_pair_prototype_on_the_golden_fixtures(fixture):
    (name, H, n, v0), = [c for c in proto.fixtures() if c[0] == fixture]
    _check(H, n, v0)


def test_pair_prototype_trips_where_the_krylov_space_is_exhausted():
    (name, H, n, v0), = [c for c in proto.fixtures() if c[0] == "lap3d_8x8x8_n40"]
    _check(H, n, v0, exhausted_at=24)  # the space is exhausted at step 25: every pair before it holds


def test_pair_prototype_abandons_a_prediction_that_cannot_hold():
    H, n = _asym_5pt(), 30
    _, _, _, st = proto.one_sweep_pair_lanczos(H, n, v0=synthetic.reference_start_vector(H.shape[0]), tau=TAU)
    assert st["abandoned"]
