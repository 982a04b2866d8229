"""The arithmetic of the group form of the one-sweep loop (run_loop_one_sweep_quad), checked without a GPU on its NumPy prototype
(tools/one_sweep_group_prototype.py, one_sweep_group_lanczos): three speculative Lanczos steps with no walk, the omega-recurrence over
the extended set with the full matrix of applied coefficients, and ONE walk over the basis that finishes four vectors.  At m = 4 both
leftovers of every group stay under the gate, the coefficients are the two-pass recurrence's to 1e-12 of the scale (the bar of
tests/test_gpu_one_sweep.py) and the basis is orthogonal to 1e-13; the deuteron fixture trips the gate (the run then belongs to the pair
form, which holds it), the exhausted Krylov space of lap3d_8x8x8 trips it as well; m = 2 is the pair form to the same bars."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import one_sweep_group_prototype as group  # noqa: E402
import one_sweep_prototype as proto  # noqa: E402

TAU = 1e-14
HOLDING = ["lap2d_32x32_n30", "graph_M2000_E7000_n40", "ragged_M700_n25", "box1d_N500_n50", "c1_dense512_n20"]


@pytest.fixture(scope="module")
def cases():
    out = {name: (H, n, v0) for name, H, n, v0 in proto.fixtures()}
    out["lap2d_300x200"] = (proto.lap2d(300, 200), 200, None)
    return out


@pytest.fixture(scope="module")
def two_pass(cases):
    memo = {}

    def get(name):
        if name not in memo:
            H, n, v0 = cases[name]
            a0, b0, V0 = proto.two_pass_lanczos(H, n, v0=v0)
            memo[name] = (a0, b0, np.abs(proto.tridiag_eigs(a0, b0)).max())
        return memo[name]

    return get


def _assert_holds(name, H, n, v0, m, ref):
    a, b, V, st = group.one_sweep_group_lanczos(H, n, m, v0=v0, tau=TAU)
    a0, b0, scale = ref
    orth = np.abs(V @ V.T - np.eye(n)).max()
    da, db = np.abs(a - a0).max() / scale, np.abs(b - b0).max() / scale
    print(f"\n[{name} n = {n} m = {m}] groups {st['groups']}, e_old {st['e_old'].max():.1e}, e_in {st['e_in'].max():.1e}, orth {orth:.1e}, "
          f"|da| {da:.1e}, |db| {db:.1e} of the scale")
    assert st["groups"] == (n - 2) // m and st["trips"] == [] and not st["abandoned"]
    assert st["e_old"].max() <= TAU and st["e_in"].max() <= TAU
    assert da <= 1e-12 and db <= 1e-12
    assert orth < 1e-13
    assert np.abs(st["G"] - V @ V.T).max() < 1e-14  # the bookkept Gram matrix is honest
    return a, b, V


@pytest.mark.parametrize("name", HOLDING + ["lap2d_300x200"])
def test_group_prototype_holds_the_bars_at_m4(cases, two_pass, name):
    H, n, v0 = cases[name]
    _assert_holds(name, H, n, v0, 4, two_pass(name))


def test_group_prototype_trips_on_the_deuteron_fixture_and_the_pair_form_holds_it(cases):
    H, n, v0 = cases["deuteron3d_N12_27pt_n100"]
    _, _, _, st = group.one_sweep_group_lanczos(H, n, 4, v0=v0, tau=TAU)
    assert st["abandoned"]
    _, _, V, stp = proto.one_sweep_pair_lanczos(H, n, v0=v0, tau=TAU)  # the run the device repeats
    assert not stp["abandoned"]
    assert np.abs(V @ V.T - np.eye(n)).max() < 1e-13


def test_group_prototype_trips_where_the_krylov_space_is_exhausted(cases):
    H, n, v0 = cases["lap3d_8x8x8_n40"]
    _, _, _, st = group.one_sweep_group_lanczos(H, n, 4, v0=v0, tau=TAU)
    assert st["abandoned"]


@pytest.mark.parametrize("name", HOLDING + ["lap2d_300x200"])
def test_group_prototype_at_m2_is_the_pair_form(cases, two_pass, name):
    H, n, v0 = cases[name]
    a, b, V = _assert_holds(name, H, n, v0, 2, two_pass(name))
    ap, bp, Vp, stp = proto.one_sweep_pair_lanczos(H, n, v0=v0, tau=TAU)
    scale = two_pass(name)[2]
    assert not stp["abandoned"] and stp["pairs"] == (n - 2) // 2
    assert np.abs(a - ap).max() <= 1e-12 * scale and np.abs(b - bp).max() <= 1e-12 * scale
    assert np.abs(V @ Vp.T - np.eye(n)).max() < 1e-13  # (one basis to the bar of either's orthogonality)
