"""The three forms of the one-sweep loop (unfused, fused, pair) at the Krylov lengths where their one-block kernels and their walks take
the paths n <= 61 never reaches, and at their size limits:

* os_wave_dots (k_os_post, k_os_sum_predict, k_os_pair_predict, k_os_pair_post): above j = 64 both its loops take further trips, with
  the clamped-duplicate tail and the len(i) = i + 2 / min(i + 2, j) bounds in them;
* the mu sum of k_os_pair_predict: nchunk = 1024 / Lp chunks, Lp = (j + 1 + 63) & ~63 - the pair runs below end inside nchunk = 8
  (n = 66, 129), 3 (258), 1 (515 .. 1023) and pass through 5, 4 and 2 and the lengths (Lp = 192, 320, 384 ...) at which threads past
  nchunk * Lp stay idle;
* the LDS limits: the pair walk's 64 KiB (j >= 1007: n = 1022, 1023), the single walk's 48 KiB (fused n = 1520, unfused n = 1536), and the
  handovers one step past each (1024: pair -> single fused, 1521: fused -> unfused, 1537: one-sweep -> six launches).

Beyond the stable prefix the coefficients of a long run are not determined by the arithmetic, so each run is held to what every
correct run satisfies (tests/lanczos_invariants.py): max |V V^T - I| < 1e-13, the extreme Ritz values within 1e-12 of the spectral
scale (n >= 258), and the relation residual max |A V^T - V^T T - r e^T| within 4x of the six-launch loop's (TUNE_LOOP = 1) on the same
input and n.  A wrong sum in the pair path need not show in the numbers - a leftover above tau abandons the pairs and the run is
repeated on the single form - so every test also asserts which path ran.  CPU prototype (tools/one_sweep_prototype.py) on these inputs:
no gate trip and no abandon in any case below except the seven-point single form, which comes within 1.5x of tau (its trip count is
not asserted)."""
import numpy as np
import pytest

import lanczos_invariants as inv
from lanczos_amd import _capi, synthetic

pytestmark = pytest.mark.gpu

SIX, FUSED, UNFUSED, PAIR = 1, 6, 7, 8
V5, V7 = "values_48x40", "values7_13x12x11"


def _handle(hip, H, knob):
    A = H.tocsr()
    h = hip.Handle(0)
    h.set_options(hip.FLAG_FUSED_NORM)
    h.set_tuning(_capi.TUNE_LOOP, knob)
    h.set_csr(A.shape[0], 0, A.indptr, A.indices, A.data)
    v0 = synthetic.reference_start_vector(A.shape[0])
    return h, v0 / np.linalg.norm(v0)


def _collect(h, a, b):
    return dict(a=np.array(a), b=np.array(b), V=h.get_basis(), engine=h.last_engine(), trips=h.last_gate_trips(),
                fused=h.last_one_sweep_fused(), pairs=h.last_one_sweep_pairs(), abandoned=h.last_pair_abandoned(), r=h.get_residual())


def _run_fresh(hip, name, n, knob):
    h, v0 = _handle(hip, inv.long_matrix(name), knob)
    a, b = h.run(n, v0)
    out = _collect(h, a, b)
    h.close()
    return out


_checked = {}


def _checked_run(hip, name, n, knob):
    """one run per (input, n, loop) with its invariants, shared by the tests and left unchanged"""
    key = (name, n, knob)
    if key not in _checked:
        got = _run_fresh(hip, name, n, knob)
        got["inv"] = inv.invariants(inv.long_matrix(name), got["a"], got["b"], got["V"], got["r"], inv.dense_spectrum(name))
        got["V"] = got["r"] = None  # (up to 24 MB a run: only what was measured on them is kept)
        _checked[key] = got
    return _checked[key]


def _reference(hip, name, n):
    """the six-launch loop on the same input and n: the yardstick of the relation residual"""
    ref = _checked_run(hip, name, n, SIX)
    assert ref["engine"] == "kernels" and ref["fused"] == 0 and ref["pairs"] == 0
    return ref


def _check(hip, name, n, knob):
    ref, got = _reference(hip, name, n), _checked_run(hip, name, n, knob)
    print(f"\n[{name} n = {n} loop {knob}] engine {got['engine']} fused {got['fused']} pairs {got['pairs']} trips {got['trips']} "
          f"abandoned {got['abandoned']}; {inv.describe(got['inv'])}; six-launch rel {ref['inv']['rel']:.1e}")
    inv.assert_invariants(got["inv"], ref["inv"]["rel"], f"{name} n = {n} loop {knob}")
    return got


REFERENCE_CASES = [(V5, n) for n in (66, 129, 258, 515, 1022, 1023, 1024, 1520, 1521, 1536, 1537)] + [(V7, 1023), (V7, 1520)]


@pytest.mark.parametrize("name,n", REFERENCE_CASES)
def test_six_launch_reference_keeps_the_invariants(hip, name, n):
    ref = _reference(hip, name, n)
    print(f"\n[{name} n = {n} loop {SIX}] engine {ref['engine']}; {inv.describe(ref['inv'])}")
    # the yardstick of the relation residual has to be sound itself: 1e-13 of the scale is a hundred times what a correct run leaves
    assert ref["inv"]["rel"] <= 1e-13 * ref["inv"]["scale"], f"first at column {ref['inv']['rel_col']}"
    inv.assert_invariants(ref["inv"], ref["inv"]["rel"], f"{name} n = {n} six-launch")


@pytest.mark.parametrize("name,n", [(V5, 66), (V5, 129), (V5, 258), (V5, 515), (V5, 1022), (V5, 1023), (V7, 1023)])
def test_pair_form_at_length(hip, name, n):
    got = _check(hip, name, n, PAIR)
    assert got["engine"] == "one-sweep" and got["fused"] == 1
    assert got["pairs"] == (n - 2) // 2 and got["abandoned"] == 0 and got["trips"] == 0


@pytest.mark.parametrize("name,n", [(V5, 129), (V5, 515), (V5, 1520), (V7, 1520)])
def test_single_fused_form_at_length(hip, name, n):
    got = _check(hip, name, n, FUSED)
    assert got["engine"] == "one-sweep" and got["fused"] == 1 and got["pairs"] == 0 and got["abandoned"] == 0
    if name == V5:
        assert got["trips"] == 0


@pytest.mark.parametrize("n", [515, 1536])
def test_unfused_form_at_length(hip, n):
    got = _check(hip, V5, n, UNFUSED)
    assert got["engine"] == "one-sweep" and got["fused"] == 0 and got["pairs"] == 0 and got["trips"] == 0


def test_handover_pair_to_single_fused(hip):
    got = _check(hip, V5, 1024, PAIR)
    assert got["engine"] == "one-sweep" and got["fused"] == 1 and got["pairs"] == 0 and got["abandoned"] == 0


def test_handover_fused_to_unfused(hip):
    got = _check(hip, V5, 1521, FUSED)
    assert got["engine"] == "one-sweep" and got["fused"] == 0 and got["pairs"] == 0


def test_handover_one_sweep_to_six_launch(hip):
    got = _check(hip, V5, 1537, FUSED)
    assert got["engine"] == "kernels" and got["fused"] == 0 and got["pairs"] == 0


def test_long_pair_rerun_is_bit_identical(hip):
    # the mu chunk sums and the multi-trip dots have a fixed order
    n = 1023
    r1, r2 = _run_fresh(hip, V5, n, PAIR), _run_fresh(hip, V5, n, PAIR)
    assert r2["engine"] == "one-sweep" and r2["fused"] == 1 and r2["pairs"] == (n - 2) // 2 and r2["abandoned"] == 0 and r2["trips"] == 0
    assert np.array_equal(r1["a"], r2["a"]) and np.array_equal(r1["b"], r2["b"]) and np.array_equal(r1["V"], r2["V"])


def test_a_prediction_that_cannot_hold_abandons_the_pairs_at_length(hip):
    # every pair's leftover is ~1e-9 (amplitude 1e-9): the run is given up and repeated on the single fused form, whose result it must be
    name, n = "asym_48x40", 130
    one, got, six = _run_fresh(hip, name, n, FUSED), _run_fresh(hip, name, n, PAIR), _run_fresh(hip, name, n, SIX)
    orth, row = inv.orthogonality(got["V"])
    print(f"\n[{name} n = {n} loop {PAIR}] engine {got['engine']} fused {got['fused']} pairs {got['pairs']} trips {got['trips']} "
          f"abandoned {got['abandoned']}; orth {orth:.1e}; single fused: trips {one['trips']}; six-launch orth {inv.orthogonality(six['V'])[0]:.1e}")
    assert one["engine"] == "one-sweep" and one["fused"] == 1 and one["pairs"] == 0 and one["abandoned"] == 0
    assert got["engine"] == "one-sweep" and got["fused"] == 1
    assert got["abandoned"] == 1 and got["pairs"] == 0
    assert np.array_equal(got["a"], one["a"]) and np.array_equal(got["b"], one["b"]) and np.array_equal(got["V"], one["V"])
    assert orth < 1e-13, f"first at row {row}"
