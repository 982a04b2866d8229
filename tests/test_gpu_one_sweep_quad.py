"""The group form of the one-sweep loop (lz_last_engine 9, lz_last_one_sweep_quads > 0; run_loop_one_sweep_quad): from step 2 on three
plain Lanczos steps run with no walk and ONE walk over the basis finishes four vectors, with coefficients predicted by the
omega-recurrence over the extended set (tools/one_sweep_group_prototype.py).  Forced at small sizes (TUNE_LOOP = 10; 11: the walk with 8
positions per lane) and compared with the six-launch loop (TUNE_LOOP = 1) and the pair form (TUNE_LOOP = 8).

Every run is held to what every correct run satisfies (tests/lanczos_invariants.py): max |V V^T - I| < 1e-13, the relation residual
within 4x of the six-launch loop's on the same input and n, the extreme Ritz values within 1e-12 of the scale (n >= 258); where the
whole run lies inside the prefix the arithmetic determines, the coefficients and the basis also agree to 1e-12 of the scale.  A wrong sum
in the group path need not show in the numbers - a leftover above tau abandons the groups and the run is repeated on the pair form - so
every test also asserts which path ran: (n - 2) // 4 groups, a pair behind them when two steps are left, no abandon, no gate trip.
CPU prototype on these inputs: no leftover above 4e-15 except on the asymmetric operator, which misses by ~1e-9 at every step."""
import functools

import numpy as np
import pytest

import lanczos_invariants as inv
from conftest import load_golden
from lanczos_amd import _capi, synthetic
from oracle import lanczos_ref as oracle

pytestmark = pytest.mark.gpu

SIX, SINGLE, PAIR, PAIR16, QUAD, QUAD8 = 1, 6, 8, 9, 10, 11
V5, V7, ASYM = "values_48x40", "values7_13x12x11", "asym_48x40"


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name.startswith("lap2d_"):
        nx, ny = name[len("lap2d_"):].split("x")
        return synthetic.laplacian_2d_5pt(int(nx), int(ny)).to_scipy()
    if name in (V5, V7, ASYM):
        return inv.long_matrix(name)
    return load_golden(name)[1]


def _handle(hip, H, knob):
    A = H.tocsr()
    h = hip.Handle(0)
    h.set_options(hip.FLAG_FUSED_NORM)
    h.set_tuning(_capi.TUNE_LOOP, knob)
    h.set_csr(A.shape[0], 0, A.indptr, A.indices, A.data)
    v0 = synthetic.reference_start_vector(A.shape[0])
    return h, v0 / np.linalg.norm(v0)


def _collect(h, a, b, basis=True):
    return dict(a=np.array(a), b=np.array(b), V=h.get_basis() if basis else None, engine=h.last_engine(), trips=h.last_gate_trips(),
                fused=h.last_one_sweep_fused(), pairs=h.last_one_sweep_pairs(), abandoned=h.last_pair_abandoned(),
                quads=h.last_one_sweep_quads(), quad_abandoned=h.last_quad_abandoned(), r=h.get_residual())


def _run_fresh(hip, name, n, knob, basis=True):
    h, v0 = _handle(hip, _matrix(name), knob)
    a, b = h.run(n, v0)
    out = _collect(h, a, b, basis)
    h.close()
    return out


_runs = {}


def _run(hip, name, n, knob):
    """one run per (input, n, loop), shared by the tests and left unchanged"""
    key = (name, n, knob)
    if key not in _runs:
        _runs[key] = _run_fresh(hip, name, n, knob)
    return _runs[key]


def _spectrum(name, ref):
    if name in (V5, V7, ASYM):
        return inv.dense_spectrum(name)
    # (short runs: only the scale is taken from it - the largest Ritz value of the six-launch run)
    return np.array([np.abs(np.linalg.eigvalsh(oracle.build_h_eff(ref["a"], ref["b"]))).max()])


def _invariants(hip, name, n, knob):
    ref, got = _run(hip, name, n, SIX), _run(hip, name, n, knob)
    assert ref["engine"] == "kernels" and ref["quads"] == 0 and ref["pairs"] == 0
    spec = _spectrum(name, ref)
    A = _matrix(name)
    for run in (ref, got):
        if "inv" not in run:
            run["inv"] = inv.invariants(A, run["a"], run["b"], run["V"], run["r"], spec)
    print(f"\n[{name} n = {n} loop {knob}] engine {got['engine']} fused {got['fused']} groups {got['quads']} pairs {got['pairs']} trips {got['trips']} "
          f"abandoned {got['quad_abandoned']}/{got['abandoned']}; {inv.describe(got['inv'])}; six-launch rel {ref['inv']['rel']:.1e}")
    inv.assert_invariants(got["inv"], ref["inv"]["rel"], f"{name} n = {n} loop {knob}")
    return ref, got


def _assert_ran_groups(got, n):
    assert got["engine"] == "one-sweep" and got["fused"] == 1
    assert got["quads"] == (n - 2) // 4 and got["pairs"] == (1 if (n - 2) % 4 == 2 else 0)
    assert got["quad_abandoned"] == 0 and got["abandoned"] == 0 and got["trips"] == 0


def _assert_equal_to_rounding(got, ref, scale, what, vectors=True):
    da, db = np.abs(got["a"] - ref["a"]).max(), np.abs(got["b"] - ref["b"]).max()
    dV = np.abs(got["V"] - ref["V"]).max() if vectors else np.abs(got["r"] - ref["r"]).max()
    print(f"\n[{what}] max |dalpha| {da:.1e}, |dbeta| {db:.1e}, |d{'V' if vectors else 'r'}| {dV:.1e} (scale {scale:.2f})")
    assert da <= inv.COEF_BAR * scale and db <= inv.COEF_BAR * scale and dV <= inv.COEF_BAR * scale


# one group with a tail of 0, 1, 2 and 3 steps; the whole run lies inside the prefix the arithmetic determines
@pytest.mark.parametrize("n", [6, 7, 8, 9])
def test_first_group_and_every_tail(hip, n):
    name = "lap2d_64x48"
    ref, got = _invariants(hip, name, n, QUAD)
    _assert_ran_groups(got, n)
    assert got["quads"] == 1
    pair = _run(hip, name, n, PAIR)
    assert pair["quads"] == 0 and pair["pairs"] == (n - 2) // 2
    scale = ref["inv"]["scale"]
    _assert_equal_to_rounding(got, ref, scale, f"n = {n} vs six-launch")
    _assert_equal_to_rounding(got, pair, scale, f"n = {n} vs pair")


# n = 31: seven groups and a single step; n = 130 (j > 64): the second trips of os_wave_dots and of the post kernel's row sums; the 33 x 31
# grid has 1023 rows (a padded last position); the seven-point rows take the other scale-on-read SpMV
@pytest.mark.parametrize("name,n", [("lap2d_64x48", 31), (V5, 130), ("lap2d_33x31", 40), (V7, 40)])
def test_group_form_keeps_the_invariants(hip, name, n):
    ref, got = _invariants(hip, name, n, QUAD)
    _assert_ran_groups(got, n)
    pair = _run(hip, name, n, PAIR)
    assert pair["engine"] == "one-sweep" and pair["quads"] == 0 and pair["pairs"] == (n - 2) // 2 and pair["abandoned"] == 0
    k = 20  # (well inside the prefix a reordered evaluation reproduces, as in tests/test_gpu_one_sweep_pair.py)
    scale = ref["inv"]["scale"]
    for other, what in ((ref, "six-launch"), (pair, "pair")):
        da, db = np.abs(got["a"] - other["a"])[:k].max(), np.abs(got["b"] - other["b"])[: k - 1].max()
        dV = np.abs(got["V"] - other["V"])[:k].max()
        print(f"[{name} n = {n} vs {what}, first {k}] |dalpha| {da:.1e}, |dbeta| {db:.1e}, |dV| {dV:.1e}")
        assert da <= inv.COEF_BAR * scale and db <= inv.COEF_BAR * scale and dV <= inv.COEF_BAR * scale


# every positions-per-lane instantiation of the group walk (2, 4 by the block count's balance over the CUs - the cases above all run one
# position per lane -, and 8 under knob 11) with its row loop run through: at n = 22 the groups start at j = 2, 6, 10, 14 and 18, so the
# walks with four rows a trip see full trips and a ragged last one, and those with two rows or one row a trip up to nine and eighteen
# trips (a group starts at an even j: two rows a trip are never ragged).  22 steps on 500 000 rows and more are far from breakdown on
# the periodic Laplacian
@pytest.mark.parametrize("name,knob", [("lap2d_1000x500", QUAD), ("lap2d_1000x1000", QUAD), ("lap2d_2000x1000", QUAD), ("lap2d_2000x1000", QUAD8)])
def test_group_equals_single_at_every_walk_width(hip, name, knob):
    n = 22
    one, got = _run_fresh(hip, name, n, SINGLE, basis=False), _run_fresh(hip, name, n, knob, basis=False)
    assert one["engine"] == "one-sweep" and one["fused"] == 1 and one["quads"] == 0 and one["pairs"] == 0 and one["trips"] == 0
    _assert_ran_groups(got, n)
    scale = np.abs(np.linalg.eigvalsh(oracle.build_h_eff(one["a"], one["b"]))).max()
    _assert_equal_to_rounding(got, one, scale, f"{name}, knob {knob}, n = {n}", vectors=False)


# the walk parks 4 waves x 4 runs of qtw_ldp(j + 4) doubles in LDS: 64 KiB hold runs of 512, so n = 512 is the longest run with groups
# and n = 513 belongs to the pair form
def test_longest_run_with_groups(hip):
    n = 512
    _, got = _invariants(hip, V5, n, QUAD)
    _assert_ran_groups(got, n)
    assert got["quads"] == 127 and got["pairs"] == 1


def test_handover_group_to_pair(hip):
    n = 513
    _, got = _invariants(hip, V5, n, QUAD)
    assert got["engine"] == "one-sweep" and got["fused"] == 1 and got["quads"] == 0 and got["quad_abandoned"] == 0
    assert got["pairs"] == (n - 2) // 2 and got["abandoned"] == 0 and got["trips"] == 0


def test_a_prediction_that_cannot_hold_abandons_the_groups(hip):
    # the groups' leftovers are ~1e-9, and so are the pairs': the run is repeated on the pair form and then on the single fused form, whose
    # gate corrects every step; the handle remembers both, so a second run forms no group and no pair
    n = 130
    one = _run(hip, ASYM, n, SINGLE)
    h, v0 = _handle(hip, _matrix(ASYM), QUAD)
    a, b = h.run(n, v0)
    got = _collect(h, a, b)
    a2, b2 = h.run(n, v0)
    again = _collect(h, a2, b2)
    h.close()
    orth, row = inv.orthogonality(got["V"])
    print(f"\n[{ASYM} n = {n}] groups {got['quads']} pairs {got['pairs']} trips {got['trips']} abandoned {got['quad_abandoned']}/{got['abandoned']}; orth {orth:.1e}")
    assert one["engine"] == "one-sweep" and one["fused"] == 1 and one["quads"] == 0 and one["pairs"] == 0
    assert got["engine"] == "one-sweep" and got["fused"] == 1
    assert got["quad_abandoned"] == 1 and got["abandoned"] == 1 and got["quads"] == 0 and got["pairs"] == 0
    assert np.array_equal(got["a"], one["a"]) and np.array_equal(got["b"], one["b"]) and np.array_equal(got["V"], one["V"])
    assert orth < inv.ORTH_BAR, f"first at row {row}"
    assert again["quad_abandoned"] == 0 and again["abandoned"] == 0 and again["quads"] == 0 and again["pairs"] == 0
    assert np.array_equal(again["a"], one["a"]) and np.array_equal(again["b"], one["b"]) and np.array_equal(again["V"], one["V"])


def test_group_rerun_is_bit_identical(hip):
    # the joint butterfly of the walk, the chunk sums of the post kernel and os_wave_dots have a fixed order
    n = 130
    r1, r2 = _run(hip, V5, n, QUAD), _run_fresh(hip, V5, n, QUAD)
    _assert_ran_groups(r2, n)
    assert np.array_equal(r1["a"], r2["a"]) and np.array_equal(r1["b"], r2["b"]) and np.array_equal(r1["V"], r2["V"])


@pytest.mark.parametrize("knob", [PAIR, PAIR16])
def test_the_pair_knobs_form_no_group(hip, knob):
    n = 31
    got = _run(hip, "lap2d_64x48", n, knob)
    assert got["engine"] == "one-sweep" and got["fused"] == 1 and got["quads"] == 0 and got["quad_abandoned"] == 0
    assert got["pairs"] == (n - 2) // 2 and got["abandoned"] == 0


def test_rows_without_a_scale_on_read_product_form_no_group(hip):
    # 27 entries per row: the unfused single form runs, as under the pair knob (the CPU prototype's m = 4 trips on this fixture at 3.5e-14;
    # tests/test_one_sweep_group_host.py holds the pair form to it)
    name, n = "deuteron3d_N12_27pt_n100", 100
    got = _run_fresh(hip, name, n, QUAD)
    orth, row = inv.orthogonality(got["V"])
    assert got["engine"] == "one-sweep" and got["fused"] == 0 and got["quads"] == 0 and got["pairs"] == 0
    assert got["quad_abandoned"] == 0 and got["abandoned"] == 0
    assert orth < inv.ORTH_BAR, f"first at row {row}"
