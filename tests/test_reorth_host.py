"""tests/reorth_reference.py checked on the CPU: the longdouble sweep against the float64 NumPy sweep on every shape the device
cases use, six deliberately wrong sweeps that the bounds must see, and the branch every device case claims against plan() and
against a short table read by hand from plan_qtw, launch_qtw_t and launch_update (lz_reorth.hip)."""
import numpy as np
import pytest
import reorth_reference as R

SECTIONS = "abcdef"


def float64_sweep(V, j, nrows, r, mode):
    """the NumPy sweep in the mode's own order of operations; returns (beta, c, row)"""
    V = V[:nrows].copy()
    beta = None
    if mode:
        beta = np.sqrt(r.dot(r))
        V[j] = r / beta
    c, row = R.numpy_sweep(V, j, nrows)
    return beta, c, row


@pytest.mark.parametrize("sec", SECTIONS)
def test_reference_against_numpy(sec):
    seen = set()
    for case in R.cases():
        key = (case.M, case.nrows, case.j, case.mode)
        if not case.id.startswith(sec + "-") or key in seen:
            continue
        seen.add(key)
        V, r = R.case_inputs(case)
        beta, c, row = float64_sweep(V, case.j, case.nrows, r, case.mode)
        ref = R.sweep_reference(V, case.j, case.nrows, r, case.mode, beta=beta if case.mode == 1 else None)
        K = R.padded(case.M) + case.nrows  # NumPy's own order is not the kernels': the classical constant
        if case.mode:
            assert abs(beta - ref.beta) <= R.gamma(R.beta_K(R.padded(case.M))) * ref.beta, case.id
            K = 3 * K + 4 if case.mode == 2 else K
        assert np.all(np.abs(c - ref.c) <= R.gamma(K) * ref.c_mag), case.id
        assert np.all(np.abs(row - ref.row) <= R.row_bound(ref, V, case.j, case.nrows, K)), case.id
        w = V[case.j] if case.mode == 0 else r / beta
        assert np.array_equal(R.replay_row(V, case.j, case.nrows, c, w), row), case.id  # NumPy's axis-0 sum is the row-order chain
    assert seen


# ---- the bounds can see the faults the device tests are there for
M_MUT, NROWS_MUT, J_MUT, L_MUT = 1300, 19, 5, 512


def mutant_inputs():
    rng = np.random.default_rng(19)
    V = rng.standard_normal((NROWS_MUT + 1, M_MUT)) / np.sqrt(M_MUT)
    V[NROWS_MUT] = 1.0  # the row behind the last one: a kernel that reads it is off by O(|w|)
    return V


def drop_last_element(V, j, nrows):
    c = np.sum(V[j, :-1] * V[:nrows, :-1], axis=1)
    return c, 2 * V[j] - np.sum(c[:, None] * V[:nrows], axis=0)


def drop_last_step_of_last_slice(V, j, nrows):
    keep = R.padded(M_MUT) - 32  # the last 32 padded elements: the last MFMA step of the ragged slice
    c = np.sum(V[j, :keep] * V[:nrows, :keep], axis=1)
    return c, 2 * V[j] - np.sum(c[:, None] * V[:nrows], axis=0)


def drop_last_partial_tile(V, j, nrows):
    c, _ = R.numpy_sweep(V, j, nrows)
    c[8 * (nrows // 8):] = 0.0
    return c, 2 * V[j] - np.sum(c[:, None] * V[:nrows], axis=0)


def self_term_from_row_below(V, j, nrows):
    c, _ = R.numpy_sweep(V, j, nrows)
    c[j] = V[j - 1].dot(V[j])
    return c, 2 * V[j] - np.sum(c[:, None] * V[:nrows], axis=0)


def last_row_twice(V, j, nrows):
    c, row = R.numpy_sweep(V, j, nrows)
    return c, row - c[nrows - 1] * V[nrows - 1]


def one_element_of_row_nrows(V, j, nrows):
    c, _ = R.numpy_sweep(V, j, nrows)
    e = M_MUT // 2
    c[nrows - 1] += (V[nrows, e] - V[nrows - 1, e]) * V[j, e]
    return c, 2 * V[j] - np.sum(c[:, None] * V[:nrows], axis=0)


MUTANTS = [drop_last_element, drop_last_step_of_last_slice, drop_last_partial_tile, self_term_from_row_below, last_row_twice, one_element_of_row_nrows]


def _violations(V, c, row):
    ref = R.sweep_reference(V, J_MUT, NROWS_MUT)
    p = R.plan(R.padded(M_MUT), 0, {0: L_MUT}, NROWS_MUT + 2)
    K = max(R.coef_K(p, R.padded(M_MUT), NROWS_MUT, 0), R.padded(M_MUT) + NROWS_MUT)  # the widest bound any case uses at this shape
    over_c = np.abs(c - ref.c) / (R.gamma(K) * ref.c_mag)
    # pass 2 is held to bit equality given c: any change of the row is a violation; the longdouble bound must see it too
    over_row = np.abs(row - ref.row) / R.row_bound(ref, V, J_MUT, NROWS_MUT, K)
    replay = np.array_equal(row, R.replay_row(V, J_MUT, NROWS_MUT, c, V[J_MUT]))
    return float(over_c.max()), float(over_row.max()), replay


def test_the_unmutated_sweep_is_inside_the_bounds():
    V = mutant_inputs()
    c, row = R.numpy_sweep(V, J_MUT, NROWS_MUT)
    over_c, over_row, replay = _violations(V, c, row)
    assert over_c <= 1.0 and over_row <= 1.0 and replay


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda f: f.__name__)
def test_the_bounds_see_a_mutant(mutant):
    V = mutant_inputs()
    c, row = mutant(V, J_MUT, NROWS_MUT)
    over_c, over_row, replay = _violations(V, c, row)
    print(f"{mutant.__name__}: c {over_c:.3g} bounds, row {over_row:.3g} bounds, replay equal: {replay}")
    if mutant is last_row_twice:  # the coefficients are right, the row is not
        assert over_c <= 1.0 and over_row > 100.0 and not replay
    else:
        assert over_c > 100.0 and over_row > 100.0


# ---- the branch table
def test_every_case_lands_on_the_branch_its_id_names():
    for case in R.cases():
        p = R.assert_claim(case)
        assert p.lds <= 155 * 1024 + 4096, case.id  # inside a CU's 160 KiB
    ids = [c.id for c in R.cases()]
    for sec in SECTIONS:
        assert any(i.startswith(sec + "-") for i in ids)


# (rows_pad, flags, knob 0, rows allocated) -> (L, G, family), by hand from plan_qtw
PASS1_BY_HAND = [
    ((1312, 0, 512, 21), (512, 3, 2)),            # a forced slice length, ragged last slice
    ((1312, 4, 512, 21), (512, 3, 0)),            # LZ_FLAG_QTW_VALU
    ((5216, 0, 5120, 802), (5120, 2, 2)),         # 158720 - 4 * 816 * 8 = 132608 >= 40960: the runs still fit
    ((1056, 0, 5120, 4100), (5120, 1, 0)),        # 158720 - 4 * 4112 * 8 = 27136 < 40960: the automatic VALU fallback
    ((60000, 0, 0, 40), (512, 118, 2)),           # fewer than 480 slices at every candidate: the 512 default
    ((10_000_000, 0, 0, 200), (5120, 1954, 2)),   # 1954 / 256 = 7.63 of 8: balanced at the longest slice
]

# (rows_pad, nrows, fused, knob 8) -> arm, by hand from launch_update
PASS2_BY_HAND = [
    ((32, 1, False, 0), "slice<1,32>"),
    ((8192, 64, True, 0), "slice<1,32>"),         # 4096 positions, not more than 64 rows
    ((8192, 65, True, 0), "elem"),
    ((8192, 65, False, 0), "slice<1,32>"),        # the element kernel is fused only
    ((8224, 65, True, 0), "slice<1,32>"),         # 4112 positions
    ((32768, 3, False, 0), "slice<1,32>"),        # 16384 positions
    ((32800, 3, False, 0), "slice<2,8>"),         # 33 blocks of P = 2 are the most blocks: best balance
    ((60000, 40, False, 0), "slice<2,8>"),
    ((243744, 3, False, 0), "slice<2,8>"),        # 121872 positions: 239 blocks of 512
    ((487456, 3, True, 0), "slice<4,4>"),         # 239 blocks of 1024
    ((974848, 3, False, 0), "slice<8,2>"),        # 238 blocks of 2048: 0.9297, no candidate balanced, the first best wins
    ((974880, 3, False, 0), "slice<8,2>"),        # 239 blocks of 2048
    ((1949696, 3, True, 0), "slice<16,1>"),       # 238 blocks of 4096: P = 16 by best balance
    ((1949728, 3, False, 0), "slice<16,1>"),      # 239 blocks of 4096
    ((66, 7, True, 1), "slice<2,8>"),             # knob 8 = 1 with the fused residual: automatic P, 16 -> the P = 2 arm
    ((66, 7, False, 1), "update<cached>"),
    ((66, 7, True, 2), "update<nt>"),
    ((40000, 70, True, 3), "slice<8,2>"),
    ((40000, 70, False, 6), "slice<16,1>"),
]


def test_plan_against_the_tables_read_by_hand():
    for (rows_pad, flags, knob0, n), want in PASS1_BY_HAND:
        assert R.plan_qtw(rows_pad, flags, {0: knob0}, n) == want, (rows_pad, flags, knob0, n)
    for (rows_pad, nrows, fused, knob8), want in PASS2_BY_HAND:
        assert R.update_arm(rows_pad, nrows, fused, knob8)[0] == want, (rows_pad, nrows, fused, knob8)
    # row split and dynamic LDS of launch_qtw_t
    assert R.plan(512, 16, {0: 512}, 202, 200, 2).Y == 25 and R.plan(512, 16, {0: 512}, 202, 200, 1).Y == 1
    assert R.plan(512, 16, {0: 512}, 10, 8, 2).Y == 1 and R.plan(65 * 512, 16, {0: 512}, 42, 40, 2).Y == 1
    assert R.plan(64 * 512, 16, {0: 512}, 42, 40, 2).Y == 4
    assert R.plan(5216, 16, {0: 5120}, 802, 800, 2).lds == 5120 * 8 + 4 * 800 * 8 == 66560
