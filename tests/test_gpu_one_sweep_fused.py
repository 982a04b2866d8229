"""The fused form of the one-sweep loop (lz_last_engine 9, lz_last_one_sweep_fused 1; run_loop_one_sweep_fused): the sweep forms
w_j = (A v_{j-1} - alpha v_{j-1}) - beta v_{j-2} itself and works in the units of w, the SpMV divides by beta on read - no three-term
pass.  Forced at small sizes (TUNE_LOOP = 6) and compared with the six-launch loop (TUNE_LOOP = 1) and with the unfused one-sweep
loop (TUNE_LOOP = 7).  The bars are those of tests/test_gpu_one_sweep.py: 1e-12 of the spectral scale on the coefficients and
vectors the reference arithmetic itself determines (the prefix a reordered evaluation reproduces to 1e-13)."""
import functools

import numpy as np
import pytest
import scipy.sparse

from conftest import load_golden
from lanczos_amd import _capi, synthetic
from oracle import lanczos_ref as oracle

pytestmark = pytest.mark.gpu

SIX, FUSED, UNFUSED = 1, 6, 7


def _perturbed_5pt(kind):
    """The 40 x 30 periodic 5-point Laplacian with its off-diagonal entries changed on their own pattern (five entries per row
    stay): "values" - symmetric perturbations of size 1e-3, so every value differs and only the offsets can be coded by row
    class; "asym" - 1e-9 (P - P^T): the prediction assumes A = A^T and misses by ~1e-9 at every step."""
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
    if name == "lap2d_64x48":
        return synthetic.laplacian_2d_5pt(64, 48).to_scipy()
    if name == "lap2d_33x31":
        return synthetic.laplacian_2d_5pt(33, 31).to_scipy()
    if name == "lap3d_10x9x8":
        return synthetic.laplacian_3d_7pt(10, 9, 8).to_scipy()
    if name == "values_40x30":
        return _perturbed_5pt("values")
    if name == "asym_40x30":
        return _perturbed_5pt("asym")
    if name.startswith("lap2d_big_"):
        nx, ny = name[len("lap2d_big_"):].split("x")
        return synthetic.laplacian_2d_5pt(int(nx), int(ny)).to_scipy()
    return load_golden(name)[1]


CASES = {"lap2d_64x48": 60, "lap2d_33x31": 40, "lap3d_10x9x8": 40, "values_40x30": 40}


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


def _run_fresh(hip, name, n, knob, poison=False, basis=True):
    h, v0 = _handle(hip, _matrix(name), knob, poison)
    a, b = h.run(n, v0)
    out = dict(a=np.array(a), b=np.array(b), V=h.get_basis() if basis else None, engine=h.last_engine(), trips=h.last_gate_trips(),
               fused=h.last_one_sweep_fused(), r=h.get_residual())
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
    print(f"\n[{what}] prefix {prefix}, rows {rows}, trips {got['trips']}, max |dalpha| {da:.1e}, |dbeta| {db:.1e}, |dV| {dV:.1e} (scale {scale:.2f})")
    assert da <= 1e-12 * scale and db <= 1e-12 * scale and dV <= 1e-12 * scale


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_two_pass_to_rounding(hip, name):
    n = CASES[name]
    ref, got = _run(hip, name, n, SIX), _run(hip, name, n, FUSED)
    assert ref["engine"] == "kernels" and got["engine"] == "one-sweep" and got["fused"] == 1 and ref["fused"] == 0
    scale, prefix, rows = _stable_of(hip, name, n)
    assert prefix >= min(n, 20) and rows >= min(n, 20), (prefix, rows)
    _assert_equal_to_rounding(got, ref, scale, prefix, rows, name)
    k = min(prefix, rows)
    assert np.abs(got["V"][:k] @ got["V"][:k].T - np.eye(k)).max() < 1e-13


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_unfused_one_sweep(hip, name):
    n = CASES[name]
    unf, got = _run(hip, name, n, UNFUSED), _run(hip, name, n, FUSED)
    assert unf["engine"] == "one-sweep" and unf["fused"] == 0 and got["engine"] == "one-sweep" and got["fused"] == 1
    assert unf["trips"] == 0 and got["trips"] == 0
    scale, prefix, rows = _stable_of(hip, name, n)
    _assert_equal_to_rounding(got, unf, scale, prefix, rows, name + " vs unfused")


# every positions-per-lane instantiation of the sweep (2, 4, 8, 16: chosen by the block count's balance over the CUs; the cases above
# all run one position per lane), a few steps each
@pytest.mark.parametrize("name", ["lap2d_big_500x500", "lap2d_big_1000x500", "lap2d_big_1000x1000", "lap2d_big_2000x1000"])
def test_fused_equals_unfused_at_every_sweep_width(hip, name):
    n = 6
    unf, got = _run_fresh(hip, name, n, UNFUSED, basis=False), _run_fresh(hip, name, n, FUSED, basis=False)
    assert unf["fused"] == 0 and got["fused"] == 1 and unf["trips"] == 0 and got["trips"] == 0
    scale = np.abs(np.linalg.eigvalsh(oracle.build_h_eff(unf["a"], unf["b"]))).max()
    da, db, dr = np.abs(got["a"] - unf["a"]).max(), np.abs(got["b"] - unf["b"]).max(), np.abs(got["r"] - unf["r"]).max()
    print(f"\n[{name}] max |dalpha| {da:.1e}, |dbeta| {db:.1e}, |dr| {dr:.1e} (scale {scale:.2f})")
    assert da <= 1e-12 * scale and db <= 1e-12 * scale and dr <= 1e-12 * scale


# the same four shapes with the walks' row loops run through: at n = 21 the last walks cover 19 or 20 rows, so k_os_sweep<2, 8> sees
# two full groups of rows and a tail, <4, 4> and <8, 2> several groups and a tail (n = 6 never completes a group of 8 or a second
# iteration of k).  21 steps on 250 000 rows and more are far from breakdown on the periodic Laplacian
@pytest.mark.parametrize("name", ["lap2d_big_500x500", "lap2d_big_1000x500", "lap2d_big_1000x1000", "lap2d_big_2000x1000"])
def test_fused_equals_unfused_at_every_sweep_width_over_full_row_groups(hip, name):
    n = 21
    unf, got = _run_fresh(hip, name, n, UNFUSED, basis=False), _run_fresh(hip, name, n, FUSED, basis=False)
    assert unf["engine"] == "one-sweep" and got["engine"] == "one-sweep"
    assert unf["fused"] == 0 and got["fused"] == 1 and unf["trips"] == 0 and got["trips"] == 0
    scale = np.abs(np.linalg.eigvalsh(oracle.build_h_eff(unf["a"], unf["b"]))).max()
    da, db, dr = np.abs(got["a"] - unf["a"]).max(), np.abs(got["b"] - unf["b"]).max(), np.abs(got["r"] - unf["r"]).max()
    print(f"\n[{name} n = {n}] max |dalpha| {da:.1e}, |dbeta| {db:.1e}, |dr| {dr:.1e} (scale {scale:.2f})")
    assert da <= 1e-12 * scale and db <= 1e-12 * scale and dr <= 1e-12 * scale


@pytest.mark.parametrize("n", [2, 3])
def test_first_fused_steps(hip, n):
    # n = 2: the only fused step has no beta term; n = 3: the first step with one, and still no third row to walk
    ref, got = _run(hip, "lap2d_64x48", n, SIX), _run(hip, "lap2d_64x48", n, FUSED)
    assert got["engine"] == "one-sweep" and got["fused"] == 1
    scale, prefix, rows = _stable_of(hip, "lap2d_64x48", n)
    assert prefix == n and rows == n
    _assert_equal_to_rounding(got, ref, scale, prefix, rows, f"n = {n}")


def test_fused_rerun_is_bit_identical(hip):
    r1 = _run(hip, "lap2d_64x48", 60, FUSED)
    r2 = _run_fresh(hip, "lap2d_64x48", 60, FUSED)
    assert r1["fused"] == 1 and r2["fused"] == 1
    assert np.array_equal(r1["a"], r2["a"]) and np.array_equal(r1["b"], r2["b"]) and np.array_equal(r1["V"], r2["V"])


def test_fused_correction_keeps_the_basis_orthogonal(hip):
    # (tools/one_sweep_prototype.py on this operator: the gate trips at every step after the first, the basis stays orthogonal to 1e-15)
    n = 30
    ref, got = _run(hip, "asym_40x30", n, SIX), _run(hip, "asym_40x30", n, FUSED)
    assert got["engine"] == "one-sweep" and got["fused"] == 1
    assert got["trips"] >= n // 2, got["trips"]
    orth = np.abs(got["V"] @ got["V"].T - np.eye(n)).max()
    da, db = np.abs(got["a"] - ref["a"]).max(), np.abs(got["b"] - ref["b"]).max()
    print(f"\ntrips {got['trips']}, max |V V^T - I| {orth:.1e}, |dalpha| {da:.1e}, |dbeta| {db:.1e}")
    assert orth < 1e-13
    assert da < 1e-7 and db < 1e-7


def test_fused_residual_and_resume(hip):
    name, j0, n = "lap2d_64x48", 30, 40
    unf, got, full = _run(hip, name, j0, UNFUSED), _run(hip, name, j0, FUSED), _run(hip, name, n, FUSED)
    assert got["fused"] == 1 and full["fused"] == 1 and unf["fused"] == 0
    scale, prefix, rows = _stable_of(hip, name, n)
    assert prefix == n and rows == n
    dr = np.abs(got["r"] - unf["r"]).max()
    h, _ = _handle(hip, _matrix(name), FUSED)
    a, b = h.run_resume(n, got["V"], got["r"], got["a"], got["b"])
    V = h.get_basis()
    h.close()
    da, db, dV = np.abs(np.array(a) - full["a"]).max(), np.abs(np.array(b) - full["b"]).max(), np.abs(V - full["V"]).max()
    print(f"\n|dr| {dr:.1e}; resumed: |dalpha| {da:.1e}, |dbeta| {db:.1e}, |dV| {dV:.1e} (scale {scale:.2f})")
    assert dr <= 1e-12 * scale
    assert da <= 1e-12 * scale and db <= 1e-12 * scale and dV <= 1e-12 * scale


@pytest.mark.parametrize("name,n", [("deuteron3d_N12_27pt_n100", 100), ("graph_M2000_E7000_n40", 40)])
def test_fallback_to_the_unfused_form(hip, name, n):
    got = _run_fresh(hip, name, n, FUSED, basis=False)
    assert got["engine"] == "one-sweep" and got["fused"] == 0


def test_poisoned_padding(hip):
    clean = _run(hip, "lap2d_33x31", 40, FUSED)
    got = _run_fresh(hip, "lap2d_33x31", 40, FUSED, poison=True)
    assert got["fused"] == 1
    assert np.isfinite(got["a"]).all() and np.isfinite(got["b"]).all()
    assert np.array_equal(got["a"], clean["a"]) and np.array_equal(got["b"], clean["b"])
