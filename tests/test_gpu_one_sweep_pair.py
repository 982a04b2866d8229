"""The pair form of the one-sweep loop (lz_last_engine 9, lz_last_one_sweep_pairs > 0; run_loop_one_sweep_pair): from step 2 on ONE
walk over the basis finishes v_j and forms the un-normalised v_{j+1} - the SpMV of step j runs on the uncorrected w_j / beta_j, and
what the correction owes to w_{j+1} is applied as a combination of basis rows.  Forced at small sizes (TUNE_LOOP = 8; 9: the walk with
16 positions per lane) and compared with the six-launch loop (TUNE_LOOP = 1) and with the single fused form (TUNE_LOOP = 6).  The bars
are those of tests/test_gpu_one_sweep_fused.py: 1e-12 of the spectral scale on the coefficients and vectors the reference arithmetic
itself determines (the prefix a reordered evaluation reproduces to 1e-13), max |V V^T - I| < 1e-13 there."""
import functools

import numpy as np
import pytest

from conftest import load_golden
from lanczos_amd import _capi, synthetic
from oracle import lanczos_ref as oracle

pytestmark = pytest.mark.gpu

SIX, SINGLE, PAIR, PAIR16 = 1, 6, 8, 9


def _perturbed_5pt(kind):
    """The 40 x 30 periodic 5-point Laplacian with its off-diagonal entries changed on their own pattern (five entries per row stay):
    "values" - symmetric perturbations of size 1e-3; "asym" - 1e-9 (P - P^T): the prediction assumes A = A^T and misses by ~1e-9 at
    every step."""
    L = synthetic.laplacian_2d_5pt(40, 30).to_scipy().tocsr()
    off = L.copy()
    off.setdiag(0.0)
    off.eliminate_zeros()
    P = off.copy()
    P.data = np.random.default_rng(5).uniform(-1.0, 1.0, size=P.nnz)
    H = (L + 1e-3 * (P + P.T)) if kind == "values" else (L + 1e-9 * (P - P.T))
    H = H.tocsr()
    H.sort_indices()
    assert np.all(np.diff(H.indptr) == 5)
    return H


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name == "lap3d_10x9x8":
        return synthetic.laplacian_3d_7pt(10, 9, 8).to_scipy()
    if name == "values_40x30":
        return _perturbed_5pt("values")
    if name == "asym_40x30":
        return _perturbed_5pt("asym")
    if name.startswith("lap2d_"):
        nx, ny = name[len("lap2d_"):].split("x")
        return synthetic.laplacian_2d_5pt(int(nx), int(ny)).to_scipy()
    return load_golden(name)[1]


CASES = [("lap2d_64x48", 60), ("lap2d_64x48", 61), ("lap2d_33x31", 40), ("lap3d_10x9x8", 40), ("values_40x30", 40)]


def _handle(hip, H, knob, poison=False):
    A = H.tocsr()
    h = hip.Handle(0)
    h.set_options(hip.FLAG_FUSED_NORM)
    h.set_tuning(_capi.TUNE_LOOP, knob)
    if poison:
        h.set_tuning(_capi.TUNE_POISON_BASIS, 1)
    h.set_csr(A.shape[0], 0, A.indptr, A.indices, A.data)
    v0 = synthetic.reference_start_vector(A.shape[0])
    return h, v0 / np.linalg.norm(v0)


def _collect(h, a, b, basis=True):
    return dict(a=np.array(a), b=np.array(b), V=h.get_basis() if basis else None, engine=h.last_engine(), trips=h.last_gate_trips(),
                fused=h.last_one_sweep_fused(), pairs=h.last_one_sweep_pairs(), abandoned=h.last_pair_abandoned(), r=h.get_residual())


def _run_fresh(hip, name, n, knob, poison=False, basis=True):
    h, v0 = _handle(hip, _matrix(name), knob, poison)
    a, b = h.run(n, v0)
    out = _collect(h, a, b, basis)
    h.close()
    return out


_runs = {}


def _run(hip, name, n, knob):
    """one run per (case, n, loop), shared by the tests and left unchanged"""
    key = (name, n, knob)
    if key not in _runs:
        _runs[key] = _run_fresh(hip, name, n, knob)
    return _runs[key]


_stable_cache = {}


def _stable_of(hip, name, n):
    if (name, n) not in _stable_cache:
        ref = _run(hip, name, n, SIX)
        H = _matrix(name)
        scale = np.abs(np.linalg.eigvalsh(oracle.build_h_eff(ref["a"], ref["b"]))).max()
        prefix, _ = oracle.stable_masks(H, n, ref["a"], ref["b"], tol=1e-13)
        rows = oracle.stable_basis_rows(H, n, ref["V"], tol=1e-13)
        _stable_cache[(name, n)] = (scale, prefix, rows)
    return _stable_cache[(name, n)]


def _assert_equal_to_rounding(got, ref, scale, prefix, rows, what):
    da = np.abs(got["a"] - ref["a"])[:prefix].max()
    db = np.abs(got["b"] - ref["b"])[: prefix - 1].max() if prefix > 1 else 0.0
    dV = np.abs(got["V"] - ref["V"])[:rows].max()
    print(f"\n[{what}] prefix {prefix}, rows {rows}, pairs {got['pairs']}, max |dalpha| {da:.1e}, |dbeta| {db:.1e}, |dV| {dV:.1e} (scale {scale:.2f})")
    assert da <= 1e-12 * scale and db <= 1e-12 * scale and dV <= 1e-12 * scale


def _assert_ran_pairs(got, n):
    assert got["engine"] == "one-sweep" and got["fused"] == 1
    assert got["pairs"] == (n - 2) // 2 and got["abandoned"] == 0 and got["trips"] == 0


@pytest.mark.parametrize("name,n", CASES)
def test_pair_equals_two_pass_to_rounding(hip, name, n):
    ref, got = _run(hip, name, n, SIX), _run(hip, name, n, PAIR)
    assert ref["engine"] == "kernels" and ref["pairs"] == 0
    _assert_ran_pairs(got, n)
    scale, prefix, rows = _stable_of(hip, name, n)
    assert prefix >= min(n, 20) and rows >= min(n, 20), (prefix, rows)
    _assert_equal_to_rounding(got, ref, scale, prefix, rows, f"{name} n = {n}")
    k = min(prefix, rows)
    assert np.abs(got["V"][:k] @ got["V"][:k].T - np.eye(k)).max() < 1e-13


@pytest.mark.parametrize("name,n", CASES)
def test_pair_equals_single_fused_form(hip, name, n):
    one, got = _run(hip, name, n, SINGLE), _run(hip, name, n, PAIR)
    assert one["engine"] == "one-sweep" and one["fused"] == 1 and one["pairs"] == 0 and one["trips"] == 0
    _assert_ran_pairs(got, n)
    scale, prefix, rows = _stable_of(hip, name, n)
    _assert_equal_to_rounding(got, one, scale, prefix, rows, f"{name} n = {n} vs single")


@pytest.mark.parametrize("n", [3, 4, 5])
def test_first_pairs(hip, n):
    # n = 3: no pair at all (steps 0, 1 and an odd last step); n = 4: exactly one pair; n = 5: one pair and a single step behind it
    ref, got = _run(hip, "lap2d_64x48", n, SIX), _run(hip, "lap2d_64x48", n, PAIR)
    assert got["engine"] == "one-sweep" and got["fused"] == 1 and got["abandoned"] == 0
    assert got["pairs"] == (0 if n == 3 else 1)
    scale, prefix, rows = _stable_of(hip, "lap2d_64x48", n)
    assert prefix == n and rows == n
    _assert_equal_to_rounding(got, ref, scale, prefix, rows, f"n = {n}")


# every positions-per-lane instantiation of the pair walk (2, 4, 8 by the block count's balance over the CUs - the cases above all run
# one position per lane -, and 16 under knob 9), a few steps each
@pytest.mark.parametrize("name,knob", [("lap2d_500x500", PAIR), ("lap2d_1000x500", PAIR), ("lap2d_1000x1000", PAIR), ("lap2d_2000x1000", PAIR),
                                       ("lap2d_2000x1000", PAIR16)])
def test_pair_equals_single_at_every_walk_width(hip, name, knob):
    n = 6
    one, got = _run_fresh(hip, name, n, SINGLE, basis=False), _run_fresh(hip, name, n, knob, basis=False)
    assert one["pairs"] == 0 and one["trips"] == 0
    _assert_ran_pairs(got, n)
    scale = np.abs(np.linalg.eigvalsh(oracle.build_h_eff(one["a"], one["b"]))).max()
    da, db, dr = np.abs(got["a"] - one["a"]).max(), np.abs(got["b"] - one["b"]).max(), np.abs(got["r"] - one["r"]).max()
    print(f"\n[{name}, knob {knob}] max |dalpha| {da:.1e}, |dbeta| {db:.1e}, |dr| {dr:.1e} (scale {scale:.2f})")
    assert da <= 1e-12 * scale and db <= 1e-12 * scale and dr <= 1e-12 * scale


# the same shapes with the walks' row loops run through: at n = 21 the last pair walks 19 rows, so k_os_pair_sweep<2, 4> and <4, 2> see
# several full groups of rows and a tail (n = 6: at most one group), and the single steps' k_os_sweep likewise.  21 steps on 250 000 rows
# and more are far from breakdown on the periodic Laplacian
@pytest.mark.parametrize("name,knob", [("lap2d_500x500", PAIR), ("lap2d_1000x500", PAIR), ("lap2d_1000x1000", PAIR), ("lap2d_2000x1000", PAIR),
                                       ("lap2d_2000x1000", PAIR16)])
def test_pair_equals_single_at_every_walk_width_over_full_row_groups(hip, name, knob):
    n = 21
    one, got = _run_fresh(hip, name, n, SINGLE, basis=False), _run_fresh(hip, name, n, knob, basis=False)
    assert one["engine"] == "one-sweep" and one["fused"] == 1 and one["pairs"] == 0 and one["trips"] == 0
    _assert_ran_pairs(got, n)
    scale = np.abs(np.linalg.eigvalsh(oracle.build_h_eff(one["a"], one["b"]))).max()
    da, db, dr = np.abs(got["a"] - one["a"]).max(), np.abs(got["b"] - one["b"]).max(), np.abs(got["r"] - one["r"]).max()
    print(f"\n[{name}, knob {knob}, n = {n}] max |dalpha| {da:.1e}, |dbeta| {db:.1e}, |dr| {dr:.1e} (scale {scale:.2f})")
    assert da <= 1e-12 * scale and db <= 1e-12 * scale and dr <= 1e-12 * scale


def test_pair_rerun_is_bit_identical(hip):
    r1 = _run(hip, "lap2d_64x48", 60, PAIR)
    r2 = _run_fresh(hip, "lap2d_64x48", 60, PAIR)
    _assert_ran_pairs(r2, 60)
    assert np.array_equal(r1["a"], r2["a"]) and np.array_equal(r1["b"], r2["b"]) and np.array_equal(r1["V"], r2["V"])


def test_a_prediction_that_cannot_hold_abandons_the_pairs(hip):
    # (tools/one_sweep_prototype.py on this operator: every pair's leftover is ~1e-9.)  The run is repeated on the single fused form, whose
    # gate corrects every step; the handle remembers it, so a second run does not try pairs again
    n = 30
    one = _run(hip, "asym_40x30", n, SINGLE)
    h, v0 = _handle(hip, _matrix("asym_40x30"), PAIR)
    a, b = h.run(n, v0)
    got = _collect(h, a, b)
    a2, b2 = h.run(n, v0)
    again = _collect(h, a2, b2)
    h.close()
    assert got["engine"] == "one-sweep" and got["fused"] == 1
    assert got["abandoned"] == 1 and got["pairs"] == 0 and got["trips"] == one["trips"] >= n // 2
    assert np.array_equal(got["a"], one["a"]) and np.array_equal(got["b"], one["b"]) and np.array_equal(got["V"], one["V"])
    assert again["abandoned"] == 0 and again["pairs"] == 0 and again["trips"] == one["trips"]
    assert np.array_equal(again["a"], one["a"]) and np.array_equal(again["b"], one["b"]) and np.array_equal(again["V"], one["V"])


@pytest.mark.parametrize("j0", [30, 31])
def test_pair_residual_and_resume(hip, j0):
    # j0 = 30: the run ends with a pair; 31: with a single step behind the last pair
    name, n = "lap2d_64x48", 40
    one, got, full = _run(hip, name, j0, SINGLE), _run(hip, name, j0, PAIR), _run(hip, name, n, PAIR)
    _assert_ran_pairs(got, j0)
    _assert_ran_pairs(full, n)
    scale, prefix, rows = _stable_of(hip, name, n)
    assert prefix == n and rows == n
    dr = np.abs(got["r"] - one["r"]).max()
    h, _ = _handle(hip, _matrix(name), PAIR)
    a, b = h.run_resume(n, got["V"], got["r"], got["a"], got["b"])
    V = h.get_basis()
    h.close()
    da, db, dV = np.abs(np.array(a) - full["a"]).max(), np.abs(np.array(b) - full["b"]).max(), np.abs(V - full["V"]).max()
    print(f"\n[j0 = {j0}] |dr| {dr:.1e}; resumed: |dalpha| {da:.1e}, |dbeta| {db:.1e}, |dV| {dV:.1e} (scale {scale:.2f})")
    assert dr <= 1e-12 * scale
    assert da <= 1e-12 * scale and db <= 1e-12 * scale and dV <= 1e-12 * scale


@pytest.mark.parametrize("name,n", [("deuteron3d_N12_27pt_n100", 100), ("graph_M2000_E7000_n40", 40)])
def test_fallback_to_the_unfused_single_form(hip, name, n):
    got = _run_fresh(hip, name, n, PAIR, basis=False)
    assert got["engine"] == "one-sweep" and got["fused"] == 0 and got["pairs"] == 0 and got["abandoned"] == 0


def test_poisoned_padding(hip):
    clean = _run(hip, "lap2d_33x31", 40, PAIR)
    got = _run_fresh(hip, "lap2d_33x31", 40, PAIR, poison=True)
    _assert_ran_pairs(got, 40)
    assert np.isfinite(got["a"]).all() and np.isfinite(got["b"]).all()
    assert np.array_equal(got["a"], clean["a"]) and np.array_equal(got["b"], clean["b"])
