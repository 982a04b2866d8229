"""Long runs of the pair form's NumPy prototype (tools/one_sweep_prototype.py, one_sweep_pair_lanczos) held to the invariants of
tests/lanczos_invariants.py - the conditions tests/test_gpu_one_sweep_long.py asks of the device loops, checked here without a GPU -
and the checker itself shown to fail, at the right step, on a run that is wrong by 1e-10.

The relation residual has no bar of the project's own: it is measured against the two-pass recurrence (the reference arithmetic,
two_pass_lanczos's) on the same input and n and must stay within 4x of it, as the device loops must of the six-launch loop."""
import os
import sys

import numpy as np
import pytest

import lanczos_invariants as inv
from lanczos_amd import synthetic

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import one_sweep_prototype as proto  # noqa: E402

TAU = 1e-14

_runs = {}


def _residual(A, a, b, V):
    """r entering step n: the closing three-term step"""
    return (A @ V[-1] - a[-1] * V[-1]) - b[-1] * V[-2]


def _two_pass(A, n, v0):
    """proto.two_pass_lanczos (the reference recurrence: c = V w, v_j = 2 w - sum c_i V_i) with its sums as matrix products, which is
    what makes n = 1023 affordable here"""
    V = np.zeros((n, A.shape[0]))
    V[0] = proto.start_vector(A.shape[0], v0=v0)
    a, b = np.zeros(n), np.zeros(n - 1)
    r = A @ V[0]
    a[0] = r @ V[0]
    r = r - a[0] * V[0]
    for j in range(n):
        b[j - 1] = np.sqrt(r @ r)
        V[j] = r / b[j - 1]
        c = V[: j + 1] @ V[j]
        V[j] = 2 * V[j] - c @ V[: j + 1]
        r = A @ V[j]
        a[j] = V[j] @ r
        r = r - V[j] * a[j] - V[j - 1] * b[j - 1]
    return a, b, V


def _pair_run(name, n):
    """one prototype run per case, shared by the tests and left unchanged"""
    if (name, n) not in _runs:
        A = inv.long_matrix(name)
        v0 = synthetic.reference_start_vector(A.shape[0])
        a, b, V, st = proto.one_sweep_pair_lanczos(A, n, v0=v0, tau=TAU)
        a0, b0, V0 = _two_pass(A, n, v0)
        ref = inv.invariants(A, a0, b0, V0, _residual(A, a0, b0, V0), inv.dense_spectrum(name))
        _runs[(name, n)] = (A, a, b, V, st, ref)
    return _runs[(name, n)]


@pytest.mark.parametrize("name,n", [("values_48x40", 258), ("values7_13x12x11", 1023)])
def test_long_pair_prototype_keeps_the_invariants(name, n):
    A, a, b, V, st, ref = _pair_run(name, n)
    got = inv.invariants(A, a, b, V, _residual(A, a, b, V), inv.dense_spectrum(name))
    left = max(st["e1"].max(), st["e2"].max())
    print(f"\n[{name} n = {n}] pairs {st['pairs']}, largest leftover {left:.1e}, smallest beta {b.min():.2f}; {inv.describe(got)}; two-pass: {inv.describe(ref)}")
    assert not st["abandoned"] and st["trips"] == [] and st["pairs"] == (n - 2) // 2
    assert left <= TAU
    assert ref["rel"] <= 1e-13 * ref["scale"]  # (the yardstick is itself a hundred times under this)
    inv.assert_invariants(got, ref["rel"], f"{name} n = {n}")
    assert got["ritz"] is not None and got["orth_row"] is None and got["rel_col"] is None


def test_the_checker_names_a_wrong_coefficient():
    name, n, k = "values_48x40", 258, 100
    A, a, b, V, st, ref = _pair_run(name, n)
    bad = a.copy()
    bad[k] *= 1.0 + 1e-10
    got = inv.invariants(A, bad, b, V, _residual(A, a, b, V), inv.dense_spectrum(name))
    assert got["rel_col"] == k and got["rel"] > 1e-12
    assert got["orth_row"] is None
    with pytest.raises(AssertionError, match=f"first at column {k}"):
        inv.assert_invariants(got, ref["rel"], "alpha scaled")


def test_the_checker_names_a_row_that_is_not_orthogonal():
    name, n = "values_48x40", 258
    A, a, b, V, st, ref = _pair_run(name, n)
    bad = V.copy()
    bad[200] += 1e-10 * V[3]
    got = inv.invariants(A, a, b, bad, _residual(A, a, b, V), inv.dense_spectrum(name))
    assert got["orth_row"] == 200 and 0.9e-10 < got["orth"] < 1.1e-10
    with pytest.raises(AssertionError, match="first at row 200"):
        inv.assert_invariants(got, ref["rel"], "row 200 moved")


def test_the_checker_does_not_pass_a_nan():
    name, n = "values_48x40", 258
    A, a, b, V, st, ref = _pair_run(name, n)
    bad = V.copy()
    bad[17, 5] = np.nan
    got = inv.invariants(A, a, b, bad, _residual(A, a, b, V), inv.dense_spectrum(name))
    assert got["orth_row"] == 17 and got["rel_col"] == 16
    with pytest.raises(AssertionError):
        inv.assert_invariants(got, ref["rel"], "a NaN in row 17")
    bad = a.copy()
    bad[40] = np.nan
    got = inv.invariants(A, bad, b, V, _residual(A, a, b, V), inv.dense_spectrum(name))
    assert got["rel_col"] == 40 and np.isnan(got["ritz"]) and got["orth_row"] is None
    with pytest.raises(AssertionError):
        inv.assert_invariants(dict(got, rel=0.0, per_col=np.zeros(n)), ref["rel"], "a NaN coefficient, seen by the Ritz values alone")
