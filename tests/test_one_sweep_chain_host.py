"""The group chain in the units of z (one_sweep_quad_iter's default), checked without a GPU on the NumPy prototype
(tools/one_sweep_group_prototype.py, one_sweep_group_lanczos with chain="unscaled"): the product runs on the unscaled z_t, b_t and a_t
come out of one pair of sums behind it, and x_t = z_t / b_t is formed by division wherever it is read.  On every fixture that holds the
gate, and on the 300 x 200 Laplacian at n = 200, both leftovers of every group stay under 5e-15 - half of the gate tau = 1e-14; the
largest measured is 3.4e-15 on ragged_M700_n25, the scaled chain's own - and alpha and beta are the two-pass recurrence's to 4e-15 of the
scale (measured: 1.7e-15 and 3.6e-16).  The two fixtures that abandon with the scaled chain still abandon."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import one_sweep_group_prototype as group  # noqa: E402
import one_sweep_prototype as proto  # noqa: E402

TAU = 1e-14
HOLDING = ["lap2d_32x32_n30", "graph_M2000_E7000_n40", "ragged_M700_n25", "box1d_N500_n50", "c1_dense512_n20"]
ABANDONING = ["deuteron3d_N12_27pt_n100", "lap3d_8x8x8_n40"]


@pytest.fixture(scope="module")
def cases():
    out = {name: (H, n, v0) for name, H, n, v0 in proto.fixtures()}
    assert sorted(out) == sorted(HOLDING + ABANDONING), "a fixture of proto.fixtures() is in neither list"
    out["lap2d_300x200"] = (proto.lap2d(300, 200), 200, None)
    return out


@pytest.mark.parametrize("name", HOLDING + ["lap2d_300x200"])
def test_unscaled_chain_holds_half_the_gate_and_the_two_pass_coefficients(cases, name):
    H, n, v0 = cases[name]
    a, b, V, st = group.one_sweep_group_lanczos(H, n, 4, v0=v0, tau=TAU, chain="unscaled")
    a0, b0, _ = proto.two_pass_lanczos(H, n, v0=v0)
    scale = np.abs(proto.tridiag_eigs(a0, b0)).max()
    da, db = np.abs(a - a0).max() / scale, np.abs(b - b0).max() / scale
    print(f"\n[{name} n = {n} unscaled chain] groups {st['groups']}, e_old {st['e_old'].max():.1e}, e_in {st['e_in'].max():.1e}, "
          f"|da| {da:.1e}, |db| {db:.1e} of the scale")
    assert st["groups"] == (n - 2) // 4 and st["trips"] == [] and not st["abandoned"]
    assert st["e_old"].max() <= 5e-15 and st["e_in"].max() <= 5e-15
    assert da <= 4e-15 and db <= 4e-15
    assert np.abs(V @ V.T - np.eye(n)).max() < 1e-13


@pytest.mark.parametrize("name", ABANDONING)
def test_unscaled_chain_still_abandons_where_the_scaled_chain_does(cases, name):
    H, n, v0 = cases[name]
    assert group.one_sweep_group_lanczos(H, n, 4, v0=v0, tau=TAU)[3]["abandoned"]
    assert group.one_sweep_group_lanczos(H, n, 4, v0=v0, tau=TAU, chain="unscaled")[3]["abandoned"]


def test_default_is_the_scaled_chain_and_an_unknown_chain_is_refused(cases):
    H, n, v0 = cases["lap2d_32x32_n30"]
    a, b, V, _ = group.one_sweep_group_lanczos(H, n, 4, v0=v0)
    a1, b1, V1, _ = group.one_sweep_group_lanczos(H, n, 4, v0=v0, chain="scaled")
    assert np.array_equal(a, a1) and np.array_equal(b, b1) and np.array_equal(V, V1)
    with pytest.raises(ValueError):
        group.one_sweep_group_lanczos(H, n, 4, v0=v0, chain="other")
