"""What makes tests/test_gpu_ritz_exact.py decisive, checked without a GPU.

The device file compares the Ritz back-transform, the Gram matrix and the quality sums bit for bit with host products of small-integer
operands, at every width, and real-valued operands entry by entry with longdouble bounds.  Here: the host products of those operands
are exact (so they are a reference, not a second opinion); the widths and row counts reach every compiled instantiation that can be
reached; six errors planted into a NumPy restatement of the tiling each fail both kinds of comparison; and the bounds are tight
enough to mean something while a plain float64 product stays well inside them.

Why the exact comparison replaces what was there: ``test_ritz_backtransform_kernels`` checked ``|G - I| < 1e-12`` on orthonormal
Ritz vectors, and an off-diagonal tile of ``G`` that is never computed, or a lower triangle that is never mirrored, holds zeros -
exactly what ``I`` holds there (``test_the_old_identity_check_misses_a_zero_tile_and_a_missing_mirror``).

The planted errors are shown on the host restatement only, not on a device build.
"""
import numpy as np
import pytest
import ritz_reference as rr

# (n, rows) of every exact back-transform the device file runs, widest and longest first
BACKTRANSFORM_SHAPES = [(208, rr.ROWS_LONG), (128, rr.ROWS_LONG_EVEN), (128, rr.ROWS_LONG_RAGGED_EVEN), (208, rr.ROWS_SL2), (128, rr.ROWS_SL2_EVEN), (rr.N_MAX, rr.ROWS_SMALL),
                        (200, rr.ROWS_CHUNKED)]
GRAM_SHAPES = [(208, rr.ROWS_GRAM), (208, 4096), (32, rr.ROWS_GRAM), (100, 4095), (360, rr.ROWS_GRAM), (200, rr.ROWS_CHUNKED)]
ROUNDING_WIDTHS = (37, 100, 117, 128, 133, 200, 209)
GRAM_ROUNDING_WIDTHS = (48, 117, 144, 208, 290)
PLANTS_RITZ = ("last_kstep", "pair_swap", "ragged_row")
PLANTS_GRAM = ("zero_tile", "no_mirror", "slice_twice")


def test_the_host_product_of_the_exact_operands_is_exact():
    """float64 BLAS against int64 on 4000 rows of the largest shape the device runs, and the 2**53 conditions of every shape"""
    n, rows = 200, rr.ROWS_CHUNKED
    V, S = rr.exact_operands(n, rows, seed=1)
    Y = V.T @ S
    idx = np.random.default_rng(0).integers(0, rows, 4000)
    exact = V[:, idx].T.astype(np.int64) @ S.astype(np.int64)
    assert np.abs(exact).max() < 2 ** 53 and np.array_equal(Y[idx], exact.astype(np.float64))
    assert rr.VMAX // 2 < np.abs(V).max() <= rr.VMAX and rr.SMAX // 2 < np.abs(S).max() <= rr.SMAX  # the range is used: 2 x 21 bits per product
    for n, rows in BACKTRANSFORM_SHAPES:
        assert n * rr.VMAX * rr.SMAX < 2 ** 53
    for n, rows in GRAM_SHAPES:
        V, S = rr.gram_operands(n, min(rows, 2000), seed=n)  # (asserts rows max|Y|^2 < 2**53 for its rows; the full count below)
        assert rows * np.abs(S).sum(axis=0).max() ** 2 < 2 ** 53
    V, S = rr.gram_operands(208, rr.ROWS_GRAM, seed=2)
    Y = V.T @ S
    assert np.array_equal(Y.T @ Y, (Y.astype(np.int64).T @ Y.astype(np.int64)).astype(np.float64))


def test_the_widths_reach_every_instantiation_that_can_be_reached():
    """n = 1..208 at the device file's three row counts: every (NT, KS) of sl2_dispatch with NT >= 3, every pair of sreg_dispatch,
    k_gemm_tn NT = 1..13; the four wider cases add NT = 14, 16 and two column groups of 9 and 12.  The eight sl2 instantiations with
    NT = 1, 2 need n <= 32 and sl_ok needs n > 32: unreachable (recorded in DESIGN.md, the code left alone)."""
    seen = {}
    for rows in (rr.ROWS_SMALL, rr.ROWS_SL2, rr.ROWS_LONG):
        for n in range(1, 209):
            for variant in (0, 1):
                p = rr.ritz_path(n, rows, variant=variant)
                seen.setdefault(p.kind, set()).add((p.NT, p.KS))
    assert seen["sl2"] == {pair for pair in rr.SL2_PAIRS if pair[0] >= 3}
    assert seen["sreg"] == set(rr.SREG_PAIRS)
    assert {nt for nt, _ in seen["plain"]} == set(range(1, 14))
    assert all(rr.ritz_path(n, rr.ROWS_LONG).kind == "plain" for n in range(1, 33))  # NT = 1, 2 never reach sl2
    assert [rr.ritz_path(n, rr.ROWS_SMALL).NT for n in (209, 256, 257, 353)] == [14, 16, 9, 12]
    # the thresholds, from the launchers: 4096 rows for sl2; 2 x 256 x 4 = 2048 32-row tiles for sreg
    assert rr.ritz_path(100, 4095).kind == "plain" and rr.ritz_path(100, 4096).kind == "sl2"
    assert rr.ritz_path(150, rr.SREG_MIN_ROWS - 1).kind == "plain" and rr.ritz_path(150, rr.SREG_MIN_ROWS).kind == "sreg" and rr.SREG_MIN_ROWS == 65505
    assert rr.ritz_path(201, rr.ROWS_LONG).kind == "plain" and rr.ritz_path(129, rr.ROWS_SL2).kind == "plain"
    assert rr.ritz_path(100, rr.ROWS_LONG, aligned=False).kind == "plain"
    # the figures lz_ritz_info reports: n = 100 = 6 x 16 + 4: six full tiles and one 4-column panel, 25 k-steps
    assert rr.ritz_path(100, rr.ROWS_LONG) == ("sl2", 7, 25, 6, 1, 32 * 25 * 25)
    assert rr.ritz_path(50, rr.ROWS_LONG) == ("sl2", 4, 13, 4, 0, 32 * 16 * 13)   # NT < 7: no 4-column panels
    assert rr.ritz_path(200, rr.ROWS_LONG) == ("sreg", 13, 50, 13, 0, 16 * 13 * 50)
    # tiles per wave at the row counts: one each at 4099 rows; a second one for 140 waves at 70 003, the ragged one among them
    assert (rr.ROWS_SL2 + 31) // 32 == 129 and rr.ROWS_SL2 % 32 == 3 and (129 + 7) // 8 == 17
    tiles, waves = (rr.ROWS_LONG + 31) // 32, 256 * 8
    assert tiles == 2188 and tiles - waves == 140 and rr.ROWS_LONG % 32 == 19 and rr.ROWS_LONG // 32 >= waves
    assert rr.ROWS_LONG_EVEN == 2188 * 32 and rr.ROWS_SL2_EVEN % 32 == 6 and rr.ROWS_LONG_RAGGED_EVEN == 2188 * 32 + 6
    assert 2188 % waves == 140  # the wave that owns the ragged tile owns tile 140 before it
    assert rr.ROWS_SMALL == 3 * 128 + 5


def test_the_gram_widths_reach_every_kernel_of_their_range():
    single = {(rr.gram_path(n, rr.ROWS_GRAM, variant=v).CT, rr.gram_path(n, rr.ROWS_GRAM, variant=v).lds) for n in range(33, 209) for v in (0, 2)}
    assert single == {(ct, lds) for ct in range(3, 14) for lds in (False, True)}
    assert all(rr.gram_path(n, rr.ROWS_GRAM).form == "split" for n in range(1, 33)) and rr.gram_path(100, 4095).form == "split"
    grouped = {rr.gram_path(n, rr.ROWS_GRAM).GS for n in range(209, 361)}
    assert grouped == {7, 8, 9, 10}  # (GS = 11 needs n > 360: tests/test_gpu_lanczos.py::test_symmetric_gram_kernel)
    table = {n: tuple(rr.gram_path(n, rr.ROWS_GRAM)[1:]) for n, *_ in rr.GROUPED_GRAM}
    assert table == {n: (ct, gs, groups, lds) for n, ct, gs, groups, lds in rr.GROUPED_GRAM}
    assert {(gs, lds) for _, _, gs, _, lds in rr.GROUPED_GRAM} == {(gs, lds) for gs in (7, 8, 9, 10) for lds in (False, True)}
    assert any(gs * groups > ct for _, ct, gs, groups, _ in rr.GROUPED_GRAM) and any(groups >= 3 for _, _, _, groups, _ in rr.GROUPED_GRAM)
    assert rr.gram_slices(rr.ROWS_GRAM) == (5, 820) and rr.ROWS_GRAM - 4 * 820 == 819
    assert rr.gram_slices(rr.ROWS_GRAM, 1) == (1, 4100) and rr.gram_slices(rr.ROWS_GRAM, 3) == (3, 1368)
    assert max(512 * n * n * 8 for n, *_ in rr.GROUPED_GRAM) < 1 << 30  # the scratch lz_ritz_gram keeps


@pytest.mark.parametrize("n,rows", [(37, 1027), (100, 1027), (200, 1027), (209, 389)])
def test_planted_errors_in_the_back_transform_fail_both_comparisons(n, rows):
    Ve, Se = rr.exact_operands(n, rows, seed=n)
    Vr, Sr = rr.real_operands(n, rows, seed=n)
    idx = np.arange(rows)
    ref, bound = rr.sampled_longdouble(Vr, Sr, idx)
    assert np.array_equal(rr.restated_ritz(Ve, Se), Ve.T @ Se)
    assert rr.worst(rr.restated_ritz(Vr, Sr), ref, bound) <= 1.0
    for plant in PLANTS_RITZ:
        assert not np.array_equal(rr.restated_ritz(Ve, Se, plant), Ve.T @ Se), plant
        assert rr.worst(rr.restated_ritz(Vr, Sr, plant), ref, bound) > 1.0, plant


@pytest.mark.parametrize("n,rows", [(48, 4099), (117, 4099), (208, 4096), (290, 4099)])
def test_planted_errors_in_the_gram_matrix_fail_both_comparisons(n, rows):
    Ve, Se = rr.gram_operands(n, rows, seed=n)
    Vr, Sr = rr.real_operands(n, rows, seed=n)
    Ye, Yr = Ve.T @ Se, Vr.T @ Sr
    ref, bound = rr.gram_longdouble(Yr)
    slices = rr.gram_slices(rows)[0]
    assert np.array_equal(rr.restated_gram(Ye, slices), Ye.T @ Ye)
    assert rr.worst(rr.restated_gram(Yr, slices), ref, bound) <= 1.0
    for plant in PLANTS_GRAM:
        G = rr.restated_gram(Ye, slices, plant)
        assert not np.array_equal(G, Ye.T @ Ye), plant
        assert np.array_equal(G, G.T) == (plant != "no_mirror")
        assert rr.worst(rr.restated_gram(Yr, slices, plant), ref, bound) > 1.0, plant


def test_the_old_identity_check_misses_a_zero_tile_and_a_missing_mirror():
    """orthonormal V and S: Y^T Y = I, and a tile left at zero is what I holds there.  The check this file's device tests replace
    passes both plants; the exact comparison and the entry-wise bound fail them (the two tests above)."""
    n, rows = 117, 4099
    rng = np.random.default_rng(5)
    V = np.linalg.qr(rng.standard_normal((rows, n)))[0].T
    S = np.linalg.qr(rng.standard_normal((n, n)))[0]
    Y = V.T @ S
    for plant in (None, "zero_tile", "no_mirror"):
        assert np.abs(rr.restated_gram(Y, 5, plant) - np.eye(n)).max() < 1e-12, plant
    assert np.abs(rr.restated_gram(Y, 5, "slice_twice") - np.eye(n)).max() > 1e-3  # (a doubled slice it does see)


@pytest.mark.parametrize("n", ROUNDING_WIDTHS)
def test_the_back_transform_bound_is_tight_and_a_float64_product_stays_inside(n):
    V, S = rr.real_operands(n, rr.ROWS_LONG, seed=n)
    idx = rr.sample_rows(rr.ROWS_LONG, seed=n)
    assert len(idx) >= 64 + 64 + 64 + 400 and idx[0] == 0 and idx[-1] == rr.ROWS_LONG - 1 and 32 * 2048 in idx
    ref, bound = rr.sampled_longdouble(V, S, idx)
    mags = np.abs(V[:, idx]).T @ np.abs(S)
    assert np.all(bound < 1e-10 * mags) and np.all(bound > 0)
    ratio = rr.worst(V[:, idx].T @ S, ref, bound)
    print(f"n = {n}: float64 BLAS at {ratio:.3f} of the bound")
    assert ratio <= 0.5


@pytest.mark.parametrize("n", GRAM_ROUNDING_WIDTHS)
def test_the_gram_bound_is_tight_and_a_float64_product_stays_inside(n):
    V, S = rr.real_operands(n, rr.ROWS_GRAM, seed=n)
    Y = V.T @ S
    ref, bound = rr.gram_longdouble(Y)
    assert np.all(bound < 1e-10 * (np.abs(Y).T @ np.abs(Y))) and np.all(bound > 0)
    ratio = rr.worst(Y.T @ Y, ref, bound)
    print(f"n = {n}: float64 BLAS at {ratio:.3f} of the bound")
    assert ratio <= 0.5


def test_the_quality_operands_are_exact_and_q_is_one_expression():
    """the integer sums of the two matrices of the device file at the widest basis, and q = s1 s1 / s2 evaluated once in float64"""
    for kind in ("laplacian", "ragged"):
        A = rr.quality_matrix(kind, 4100)
        V, S = rr.gram_operands(300, 4100, seed=7)
        q = rr.quality_exact(A, V.T @ S)
        assert q.shape == (300,) and np.all(np.isfinite(q)) and np.all(q >= 0)
        assert np.array_equal(A.data, np.rint(A.data))
    A = rr.quality_matrix("ragged", 2049)
    counts = np.diff(A.indptr)
    assert (counts == 0).sum() >= 200 and counts.max() >= 1000 and A.has_sorted_indices and A.indices.dtype == np.int32
