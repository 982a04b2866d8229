"""The FP64-MFMA layer of lz_gemm.hip - Ritz back-transform, Gram matrix, quality sums - against exact and longdouble references at
every width (tests/ritz_reference.py; what makes the comparison decisive: tests/test_ritz_exact_host.py).

No Lanczos run anywhere: the basis is set from the host (``basis_alloc`` + ``basis_set_rows``) on an identity matrix of ``rows`` rows,
``S`` is whatever the case needs.  With small-integer operands every kernel, chunking and window must return the bits of the host's
BLAS product (every partial sum is an integer below 2**53), so the comparisons are ``array_equal`` over all rows and columns.
Real-valued operands then cover rounding, entry by entry under the longdouble bounds.

Row counts, from the launchers: 389 (k_gemm_tn: three whole workgroups and a ragged one); 4099 and 4102 (k_gemm_tn_sl2 from 4096 rows:
128 whole 32-row tiles and a ragged one of 3 / 6 rows, one tile per wave); 70 003 (2188 tiles over 2048 waves: 140 waves carry the
fragment ring into a second tile, the ragged 19-row tile is one of those; k_gemm_tn_sreg is eligible from 65 505 rows), 70 016
(2188 whole tiles) and 70 022 (a ragged second tile of 6 rows: the even end).  Each line printed is a figure for LAB_NOTEBOOK.md.
"""
import time

import numpy as np
import pytest
import ritz_reference as rr
from test_ritz_exact_host import GRAM_ROUNDING_WIDTHS, ROUNDING_WIDTHS

from lanczos_amd import _capi

pytestmark = pytest.mark.gpu

_cache = {}


def sliced(kind, n, rows):
    """exact: the widest operands of a row count are made once, width n takes ``V[:n]`` and ``S[:n, :n]``; gram: made per width (a cut
    through the sparse S would lose its entries)"""
    if kind == "gram":
        return rr.gram_operands(n, rows, seed=n + rows)
    if rows not in _cache:
        if len(_cache) >= 2:
            _cache.pop(next(iter(_cache)))
        _cache[rows] = rr.exact_operands(208 if rows > rr.ROWS_SMALL else rr.N_MAX, rows, seed=rows)
    V, S = _cache[rows]
    return V[:n], np.ascontiguousarray(S[:n, :n])


def identity_handle(rows):
    h = _capi.Handle(0)
    i = np.arange(rows + 1, dtype=np.int32)
    h.set_csr(rows, 0, i, i[:-1], np.ones(rows))
    return h


def set_basis(h, V):
    h.basis_alloc(V.shape[0])
    h.basis_set_rows(0, V)


def check_path(h, n, rows, variant):
    info, path = h.ritz_info(), rr.ritz_path(n, rows, variant=variant)
    assert info["chunk_rows"] == 0
    assert (info["tiles"] > 0) == (path.kind != "plain") and info["mfma_floor_cycles_per_tile"] == path.floor, (n, rows, variant, info, path)
    return path


# ------------------------------------------------------------------------------------------------- 1. back-transform, exact
def _width_groups():
    """(rows, widths): the 16 widths of a column-tile count together at the short row counts, in halves at the long ones (a case
    moves 2 x 4 x rows x n doubles per width)"""
    out = []
    for nt in range(1, 14):
        w = tuple(range(16 * (nt - 1) + 1, 16 * nt + 1))
        for rows in (rr.ROWS_SMALL, rr.ROWS_SL2) + ((rr.ROWS_SL2_EVEN,) if 3 <= nt <= 8 else ()):
            out.append((rows, w))
        for rows in (rr.ROWS_LONG,) + ((rr.ROWS_LONG_EVEN, rr.ROWS_LONG_RAGGED_EVEN) if 3 <= nt <= 8 else ()):
            out += [(rows, w[:8]), (rows, w[8:])]
    return out


@pytest.mark.parametrize("rows,widths", _width_groups(), ids=lambda v: str(v) if isinstance(v, int) else f"n{v[0]}-{v[-1]}")
def test_back_transform_exact_at_every_width(rows, widths):
    """n = 1 .. 208 grouped by column tiles, one handle per group: up through the widths with TUNE_RITZ_KERNEL 0 and 1, then part of
    the way down again (a narrower basis and S, the larger Y buffer): all of Y equals the host product, the kernel that ran is the one
    ritz_path names, ritz_fetch returns the same bits, the basis is untouched"""
    t0 = time.perf_counter()
    h = identity_handle(rows)
    kinds = set()
    for n in widths + widths[-4::-5]:
        V, S = sliced("exact", n, rows)
        ref = V.T @ S
        set_basis(h, V)
        for variant in (0, 1):
            h.set_tuning(_capi.TUNE_RITZ_KERNEL, variant)
            Y = h.ritz_vectors(S)
            assert np.array_equal(Y, ref), (n, rows, variant, np.argwhere(Y != ref)[:8])
            kinds.add(check_path(h, n, rows, variant).kind)
            assert np.array_equal(h.ritz_fetch(), ref)
        assert np.array_equal(h.get_basis(), V)
    h.close()
    print(f"back-transform exact n={widths[0]}..{widths[-1]} rows={rows}: paths {sorted(kinds)}, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("n", [209, 256, 257, 353])
def test_back_transform_exact_past_208_columns(n):
    """k_gemm_tn NT = 14 and 16 (one column group) and NT = 9, 12 (n = 257, 353: two column groups, the second ragged)"""
    rows = rr.ROWS_SMALL
    path = rr.ritz_path(n, rows)
    assert (path.kind, path.NT) == ("plain", {209: 14, 256: 16, 257: 9, 353: 12}[n])
    h = identity_handle(rows)
    V, S = sliced("exact", n, rows)
    set_basis(h, V)
    for variant in (0, 1):
        h.set_tuning(_capi.TUNE_RITZ_KERNEL, variant)
        assert np.array_equal(h.ritz_vectors(S), V.T @ S)
        check_path(h, n, rows, variant)
        assert np.array_equal(h.ritz_fetch(), V.T @ S)
    h.close()


@pytest.mark.parametrize("rows,widths", [(rr.ROWS_SL2, (16, 17, 33, 129, 208, 130, 48, 5)), (rr.ROWS_LONG, (100, 200, 117, 37, 208, 130, 64))])
def test_one_handle_across_the_kernels(rows, widths):
    """npad changes with every step (d_S is re-allocated), Y shrinks into the larger buffer of the step before, and the kernel changes
    between k_gemm_tn, the S-in-LDS and the S-stationary form"""
    h = identity_handle(rows)
    for n in widths:
        V, S = sliced("exact", n, rows)
        set_basis(h, V)
        assert np.array_equal(h.ritz_vectors(S), V.T @ S), n
        check_path(h, n, rows, 0)
    h.close()


# ------------------------------------------------------------------------------------------------- 2. back-transform, rounding
@pytest.mark.parametrize("n", ROUNDING_WIDTHS)
def test_back_transform_rounding_within_the_longdouble_bound(n):
    rows = rr.ROWS_LONG
    V, S = rr.real_operands(n, rows, seed=n)
    idx = rr.sample_rows(rows, seed=n)
    ref, bound = rr.sampled_longdouble(V, S, idx)
    h = identity_handle(rows)
    set_basis(h, V)
    for variant in (0, 1):
        h.set_tuning(_capi.TUNE_RITZ_KERNEL, variant)
        Y = h.ritz_vectors(S)
        path = check_path(h, n, rows, variant)
        ratio = rr.worst(Y[idx], ref, bound)
        print(f"back-transform rounding n={n} rows={rows} {path.kind} NT={path.NT} KS={path.KS}: error / bound {ratio:.3f}")
        assert np.all(np.isfinite(Y)) and ratio <= 1.0
    h.close()


# ------------------------------------------------------------------------------------------------- 3. chunked mode and windows
@pytest.mark.parametrize("n", [100, 200])
@pytest.mark.parametrize("chunk", [65552, 65536, 4099, 16])
def test_chunked_mode_and_windows_exact(n, chunk):
    """131 100 rows in chunks of 65 552 (65 552 + 65 548 rows: two chunks on the persistent kernels, the second ragged), 65 536 (two
    such chunks and a 28-row remainder on k_gemm_tn), 4099 (rounded up to 4112: no multiple of 16 asked for; a last chunk of 3628 rows
    on k_gemm_tn) and 16 rows: all rows, windows off the 16-row grid, across chunk boundaries, of one row, of
    the last row and of no row, then the Gram matrix of the chunks - all against the exact product, the basis untouched"""
    t0 = time.perf_counter()
    rows = rr.ROWS_CHUNKED
    step = (chunk + 15) // 16 * 16
    V, S = rr.exact_operands(n, rows, seed=n + chunk)
    ref = V.T @ S
    h = identity_handle(rows)
    set_basis(h, V)
    h.set_tuning(_capi.TUNE_RITZ_CHUNK_ROWS, chunk)
    assert h.ritz_vectors(S, fetch=False) is None
    assert h.ritz_info()["chunk_rows"] == step
    assert np.array_equal(h.ritz_fetch(), ref)
    windows = [(3, 3 + step + 21), (step - 5, step + 7), (2 * step - 1, 2 * step + 1), (21, 22), (rows - 1, rows), (rows - 37, rows), (16, 48),
               (step + 16 - 3, 2 * step + 16 + 3), (rows - (rows % step) - 9, rows)]
    windows = [(r0, min(r1, rows)) for r0, r1 in windows if 0 <= r0 < min(r1, rows)]
    assert len(windows) >= 8
    for r0, r1 in windows:
        assert np.array_equal(h.ritz_fetch_rows(r0, r1), ref[r0:r1]), (r0, r1)
    sentinel = np.full((4, n), -3.0)
    h.check(h.lib.lz_get_ritz_rows(h._h, 21, 0, _capi.dptr(sentinel)))  # no row, off the grid: OK, nothing written
    assert np.all(sentinel == -3.0)
    assert np.array_equal(h.get_basis(), V)
    Vg, Sg = rr.gram_operands(n, rows, seed=n + chunk)
    h.basis_set_rows(0, Vg)
    h.ritz_vectors(Sg, fetch=False)
    Yg = Vg.T @ Sg
    G = h.ritz_gram()
    assert np.array_equal(G, Yg.T @ Yg) and np.array_equal(G, G.T)
    assert np.array_equal(h.ritz_fetch_rows(step - 5, step + 7), Yg[step - 5: step + 7])
    assert np.array_equal(h.get_basis(), Vg)
    h.close()
    print(f"chunked n={n} chunk={chunk}: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------- 4. Gram, exact
def gram_case(h, n, rows, knobs=(0, 1, 2), slices=0):
    V, S = sliced("gram", n, rows)
    Y = V.T @ S
    ref = Y.T @ Y
    set_basis(h, V)
    h.ritz_vectors(S, fetch=False)
    h.set_tuning(_capi.TUNE_GRAM_SLICES, slices)
    for knob in knobs:
        h.set_tuning(_capi.TUNE_GRAM_KERNEL, knob)
        G = h.ritz_gram()
        assert np.array_equal(G, ref), (n, rows, knob, np.argwhere(G != ref)[:8])
        assert np.array_equal(G, G.T)
        assert (h.gram_info()["ksteps"] > 0) == (knob != 1 and 32 < n <= 208 and rows >= 4096), (n, rows, knob)
        if h.gram_info()["ksteps"] > 0:  # the first slice's k-steps: the slicing is the one gram_slices restates
            assert h.gram_info()["ksteps"] == (min(rr.gram_slices(rows, slices)[1], rows) + 3) // 4
    assert np.array_equal(h.get_basis(), V)


@pytest.mark.parametrize("rows", [rr.ROWS_GRAM, 4096])
@pytest.mark.parametrize("ct", range(3, 14))
def test_gram_exact_at_every_width(ct, rows):
    """n = 16 (ct - 1) + 1 .. 16 ct with TUNE_GRAM_KERNEL 0 (LDS-staged where n is even), 1 (split-K TN GEMM), 2 (register rings), up
    and part of the way down on one handle.  4099 rows: 5 K slices, the last of 819 rows with a ragged k-step; 4096: 4 whole slices."""
    t0 = time.perf_counter()
    h = identity_handle(rows)
    widths = list(range(16 * (ct - 1) + 1, 16 * ct + 1))
    for n in widths + widths[-4::-5]:
        gram_case(h, n, rows)
    h.close()
    print(f"gram exact CT={ct} rows={rows}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("n,rows", [(1, rr.ROWS_GRAM), (16, rr.ROWS_GRAM), (17, rr.ROWS_GRAM), (32, rr.ROWS_GRAM), (100, 4095), (208, 4095), (290, 4095)])
def test_gram_exact_on_the_split_k_path(n, rows):
    """fewer than three column tiles or fewer than 4096 rows: launch_gram_sym declines whatever the knob (no clock record)"""
    assert rr.gram_path(n, rows).form == "split"
    h = identity_handle(rows)
    gram_case(h, n, rows)
    h.close()


@pytest.mark.parametrize("n,ct,gs,groups,lds", rr.GROUPED_GRAM)
def test_gram_exact_in_groups(n, ct, gs, groups, lds):
    """208 < n <= 360 (the scratch stays under 1 GB), every group size launch_gram_sym chooses there (its selection restated in
    ritz_reference.gram_path and evaluated over the range) - (n, CT, GS, groups): (209, 14, 7, 2) (224, 14, 7, 2) (225, 15, 8, 2: padded)
    (256, 16, 8, 2) (257, 17, 9, 2: padded) (288, 18, 9, 2) (289, 19, 10, 2: padded) (290, 19, 10, 2: padded) (320, 20, 10, 2)
    (321, 21, 7, 3) (336, 21, 7, 3) (337, 22, 8, 3: padded) (360, 23, 8, 3: padded); even n: k_gram_units_lds, odd n and knob 2:
    k_gram_units.  GS = 11 needs n > 360 and stays with test_gpu_lanczos.py::test_symmetric_gram_kernel."""
    assert tuple(rr.gram_path(n, rr.ROWS_GRAM)) == ("units", ct, gs, groups, lds)
    h = identity_handle(rr.ROWS_GRAM)
    gram_case(h, n, rr.ROWS_GRAM)
    h.close()


@pytest.mark.parametrize("slices", [1, 3])
def test_gram_exact_with_the_slice_count_forced(slices):
    """TUNE_GRAM_SLICES: one slice of all 4099 rows, three of 1368 / 1368 / 1363; single-group and grouped form"""
    h = identity_handle(rr.ROWS_GRAM)
    for n in (117, 144, 290):
        gram_case(h, n, rr.ROWS_GRAM, knobs=(0, 2), slices=slices)
    h.close()


# ------------------------------------------------------------------------------------------------- 5. Gram, rounding
@pytest.mark.parametrize("n", GRAM_ROUNDING_WIDTHS)
def test_gram_rounding_within_the_longdouble_bound(n):
    rows = rr.ROWS_GRAM
    V, S = rr.real_operands(n, rows, seed=n)
    h = identity_handle(rows)
    set_basis(h, V)
    Y = h.ritz_vectors(S)
    ref, bound = rr.gram_longdouble(Y)
    for knob in (0, 1):
        h.set_tuning(_capi.TUNE_GRAM_KERNEL, knob)
        G = h.ritz_gram()
        ratio = rr.worst(G, ref, bound)
        print(f"gram rounding n={n} rows={rows} knob={knob} {rr.gram_path(n, rows, variant=knob).form}: error / bound {ratio:.4f}")
        assert np.all(np.isfinite(G)) and ratio <= 1.0
        assert knob == 1 or np.array_equal(G, G.T)
    h.close()


# ------------------------------------------------------------------------------------------------- 6. quality, exact
QUALITY_WIDTHS = (1, 16, 17, 255, 256, 257, 300)


def quality_case(h, A, n, rows, modes):
    V, S = sliced("gram", n, rows)
    q = rr.quality_exact(A, V.T @ S)
    set_basis(h, V)
    for chunk, collectives in modes:
        h.set_tuning(_capi.TUNE_RITZ_CHUNK_ROWS, chunk)
        h.set_tuning(_capi.TUNE_FORCE_COLLECTIVES, collectives)
        h.ritz_vectors(S, fetch=False)
        assert h.ritz_info()["chunk_rows"] == (1008 if chunk else 0)
        got = h.ritz_quality()
        assert np.array_equal(got, q), (rows, n, chunk, collectives, np.flatnonzero(got != q)[:8])
        assert np.array_equal(h.get_basis(), V)


@pytest.mark.parametrize("rows", [2047, 2048, 2049, 4100])
@pytest.mark.parametrize("kind", ["laplacian", "ragged"])
def test_quality_exact(kind, rows):
    """q_i = (z . y_i)**2 / (z . z), z = A y_i, from integer A (a graph Laplacian; a matrix with empty rows and one long row) and Y:
    the fused CSR kernel (k_ritz_quality: one block per 2048 rows - the row counts sit on either side of that - and lanes striding
    the columns by 256), the row-block path (TUNE_FORCE_COLLECTIVES: one SpMV per Ritz vector through basis row 0) and the chunked
    mode of both (16-column batches): the same bits as the integer sums on the host, and the basis unchanged after each"""
    t0 = time.perf_counter()
    A = rr.quality_matrix(kind, rows)
    h = _capi.Handle(0)
    h.set_csr(rows, 0, A.indptr, A.indices, A.data)
    for n in QUALITY_WIDTHS:
        quality_case(h, A, n, rows, [(0, 0), (0, 1), (1000, 0), (1000, 1)])
    h.close()
    print(f"quality exact {kind} rows={rows}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("rows", [2047, 2048, 2049, 4100])
@pytest.mark.parametrize("n", QUALITY_WIDTHS)
def test_quality_exact_of_a_dense_matrix(n, rows):
    """the same Laplacian through lz_set_dense: always the row-block path, one GEMV per Ritz vector"""
    t0 = time.perf_counter()
    A = rr.quality_matrix("laplacian", rows)
    h = _capi.Handle(0)
    h.set_dense(A.toarray())
    quality_case(h, A, n, rows, [(0, 0)])
    h.close()
    print(f"quality exact dense n={n} rows={rows}: {time.perf_counter() - t0:.2f} s")
