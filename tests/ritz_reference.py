"""References for the FP64-MFMA layer behind ``lz_ritz_vectors``, ``lz_get_ritz_rows``, ``lz_ritz_gram`` and ``lz_ritz_quality``.

**Exact operands.**  With small-integer ``V`` and ``S`` every product and every partial sum of ``Y = V^T S`` is an integer below
``2**53``: the float64 result is the same bits in any summation order, so every kernel, chunking and window must return exactly what a
BLAS product returns on the host (``exact_operands``).  The Gram matrix and the quality sums square ``Y``, so their operands keep
``Y`` small (``gram_operands``: ``V`` in {-1, 0, 1}, a few entries of magnitude <= 2 per column of ``S``); ``quality_exact`` also checks
the bounds on ``z = A Y``, ``z . y`` and ``z . z``.

**Real operands** (``real_operands``: ``standard_normal * 10**uniform(-2, 2)``) go with entry-wise longdouble bounds: a dot product of
``m`` terms in any order is within ``gamma(m) sum|a_i b_i|``, ``gamma(m) = m u / (1 - m u)``, ``u = 2**-53`` (``sampled_longdouble``:
``m = n + 2``, the two more for the reference's own rounding and the last add of two partial tiles; ``gram_longdouble``: ``m = rows + 8``,
any order over ``rows`` products plus the slice and chunk sums).

**Dispatch.**  ``ritz_path`` restates ``launch_ritz_gemm``'s choice of kernel and instantiation with the figure ``lz_ritz_info`` reports
as ``mfma_floor_cycles_per_tile``; ``gram_path`` restates ``launch_gram_sym``'s (column tiles, group size, groups, LDS-staged or not).

**Restatements with planted errors** (``restated_ritz``, ``restated_gram``): NumPy walks of the same tiling - k-steps of four basis rows,
16-column tiles, K slices summed in order, upper tiles mirrored - into which the host tests plant the errors such kernels make.

A plain module: no fixtures, nothing collected from it.
"""
from collections import namedtuple

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# row counts of the device file (tests/test_gpu_ritz_exact.py), derived from the launchers in lz_gemm.hip:
ROWS_SMALL = 389      # k_gemm_tn: 128 rows per workgroup - three whole workgroups and one of 5 rows
ROWS_SL2 = 4099       # the S-in-LDS kernel starts at 4096 rows: 128 whole 32-row tiles and one of 3 rows, one tile per wave (17 workgroups)
ROWS_LONG = 70003     # 2188 tiles > 256 workgroups x 8 waves: 140 waves take a second tile, the last of them the ragged 19-row one;
                      # 2188 >= 2048 tiles: the S-stationary kernel is eligible (from 65 505 rows)
ROWS_LONG_EVEN = 70016  # 2188 x 32: whole tiles only, the last of them a wave's second tile
ROWS_LONG_RAGGED_EVEN = 70022  # 2188 whole tiles and one of 6 rows, again some wave's second tile: the ragged end on a whole row pair
ROWS_SL2_EVEN = 4102  # 128 whole tiles and one of 6 rows: a ragged tile that ends on a whole pair of rows
ROWS_CHUNKED = 131100  # chunks of 65 552 rows: two on the persistent kernels (65 552 + 65 548); of 65 536: two and a 28-row remainder on k_gemm_tn
ROWS_GRAM = 4099      # 5 K slices of 820 rows, the last of 819 with a ragged k-step
VMAX = SMAX = 2 ** 20  # |V|, |S| of the exact back-transform operands: n * 2**40 < 2**53 up to n = 8191
N_MAX = 353           # the widest basis of the device file
SREG_MIN_ROWS = 32 * (2 * 256 * 4 - 1) + 1  # ceil(rows / 32) >= 2 kNumCU (kTPB / 64)

# grouped Gram form, 208 < n <= 360: (n, CT, GS, groups, LDS-staged) - every group size launch_gram_sym can choose there, even
# (LDS-staged) and odd (register rings) n, padded last groups (GS x groups > CT), three groups
GROUPED_GRAM = ((209, 14, 7, 2, False), (224, 14, 7, 2, True), (225, 15, 8, 2, False), (256, 16, 8, 2, True), (257, 17, 9, 2, False),
                (288, 18, 9, 2, True), (289, 19, 10, 2, False), (290, 19, 10, 2, True), (320, 20, 10, 2, True), (321, 21, 7, 3, False),
                (336, 21, 7, 3, True), (337, 22, 8, 3, False), (360, 23, 8, 3, True))

RitzPath = namedtuple("RitzPath", "kind NT KS NF R4 floor")
GramPath = namedtuple("GramPath", "form CT GS groups lds")
SREG_PAIRS = ((9, 34), (9, 36), (10, 38), (10, 40), (11, 42), (11, 44), (12, 46), (12, 48), (13, 50))  # sreg_dispatch
SL2_PAIRS = tuple((nt, 4 * nt - 3 + i) for nt in range(1, 9) for i in range(4))                         # sl2_dispatch


def gamma(m):
    return m * U / (1.0 - m * U)


def exact_operands(n, rows, seed, vmax=VMAX, smax=SMAX):
    """integer-valued float64 ``V`` (n, rows) in [-vmax, vmax] and ``S`` (n, n) in [-smax, smax]"""
    assert n * vmax * smax < 2 ** 53
    rng = np.random.default_rng(seed)
    V = rng.integers(-vmax, vmax + 1, size=(n, rows)).astype(np.float64)
    S = rng.integers(-smax, smax + 1, size=(n, n)).astype(np.float64)
    return V, S


def gram_operands(n, rows, seed, per_column=3):
    """``V`` (n, rows) in {-1, 0, 1}; ``S`` (n, n) with ``min(per_column, n)`` entries of magnitude 1 or 2 per column, so that
    ``|Y| <= 2 per_column`` and ``rows max|Y|**2 < 2**53``: ``Y^T Y`` is exact in float64 in any order"""
    rng = np.random.default_rng(seed)
    V = rng.integers(-1, 2, size=(n, rows)).astype(np.float64)
    S = np.zeros((n, n))
    k = min(per_column, n)
    for j in range(n):
        S[rng.choice(n, size=k, replace=False), j] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=k)
    ymax = np.abs(S).sum(axis=0).max()
    assert ymax <= 2 * per_column and rows * ymax ** 2 < 2 ** 53
    return V, S


def real_operands(n, rows, seed):
    """entries ``standard_normal * 10**uniform(-2, 2)``: four decades of magnitude within one dot product"""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, rows)) * 10.0 ** rng.uniform(-2, 2, (n, rows))
    S = rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-2, 2, (n, n))
    return V, S


def quality_matrix(kind, rows):
    """integer matrices for the quality sums (scipy CSR, int32 sorted indices): 'laplacian' - ``random_graph_laplacian(rows, 3 rows)``;
    'ragged' - about three entries of magnitude 1 or 2 per row, every seventh row empty, row 5 with ``min(rows, 1500)`` entries"""
    import scipy.sparse

    if kind == "laplacian":
        from lanczos_amd import synthetic

        return synthetic.random_graph_laplacian(rows, 3 * rows, seed=rows).to_scipy()
    rng = np.random.default_rng(rows)
    r = rng.integers(0, rows, 3 * rows)
    c = rng.integers(0, rows, 3 * rows)
    keep = (r % 7 != 3) & (r != 5)
    long_cols = rng.choice(rows, size=min(rows, 1500), replace=False)
    r = np.concatenate([r[keep], np.full(len(long_cols), 5)])
    c = np.concatenate([c[keep], long_cols])
    key = np.unique(r.astype(np.int64) * rows + c)  # one entry per position
    r, c = key // rows, key % rows
    v = rng.choice([-2.0, -1.0, 1.0, 2.0], size=len(key))
    A = scipy.sparse.csr_matrix((v, (r, c)), shape=(rows, rows))
    A.sort_indices()
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    return A


def quality_exact(A, Y):
    """``q_i = s1_i**2 / s2_i`` with ``z = A y_i``, ``s1 = z . y_i``, ``s2 = z . z`` from integer operands (``A``: scipy sparse or dense
    array), after checking that every sum of magnitudes stays below ``2**53`` (so any order and any fused multiply-add gives the same
    bits) and that no column of ``A Y`` is zero"""
    absA = abs(A)
    Z = np.asarray(A @ Y)
    zb = np.asarray(absA @ np.abs(Y))
    assert np.array_equal(Z, np.rint(Z)) and np.array_equal(Y, np.rint(Y))
    assert zb.max() < 2 ** 53 and (zb * np.abs(Y)).sum(axis=0).max() < 2 ** 53 and (zb * zb).sum(axis=0).max() < 2 ** 53
    s1 = np.einsum("ij,ij->j", Z, Y)
    s2 = np.einsum("ij,ij->j", Z, Z)
    assert np.all(s2 > 0)
    assert np.array_equal(s1, (Z.astype(np.int64) * Y.astype(np.int64)).sum(axis=0)) and np.array_equal(s2, (Z.astype(np.int64) ** 2).sum(axis=0))
    return s1 * s1 / s2


# ---------------------------------------------------------------------------------------------------------------- dispatch
def ritz_path(n, rows, aligned=True, variant=0):
    """``launch_ritz_gemm``'s choice for an ``n``-wide back-transform of ``rows`` rows (``aligned``: 16-byte aligned ``V`` with an even
    stride; ``variant``: TUNE_RITZ_KERNEL): ``(kind, NT, KS, NF, R4, floor)``.  ``floor`` is ``mfma_floor_cycles_per_tile`` of
    ``lz_ritz_info`` - 16 x ``clk[3]`` of the kernel that ran: ``sl2`` records ``2 (4 NF + R4) KS``, ``sreg`` ``NT KS``, ``k_gemm_tn``
    records nothing (``tiles == 0``, floor 0)."""
    ct = (n + 15) // 16
    tiles32 = (rows + 31) // 32
    if variant != 1 and aligned and 32 < n <= 128 and rows >= 4096:
        nt, ks = ct, (n + 3) // 4
        assert (nt, ks) in SL2_PAIRS
        use4 = nt >= 7
        r4 = 0 if (4 * nt == ks or not use4) else ks - 4 * (nt - 1)
        nf = nt - 1 if r4 else nt
        return RitzPath("sl2", nt, ks, nf, r4, 32 * (4 * nf + r4) * ks)
    if variant != 1 and aligned and 128 < n <= 200 and tiles32 >= 2 * 256 * 4:
        nt, ks = ct, (((n + 3) // 4) + 1) & ~1
        assert (nt, ks) in SREG_PAIRS
        return RitzPath("sreg", nt, ks, nt, 0, 16 * nt * ks)
    groups = (ct + 15) // 16
    return RitzPath("plain", (ct + groups - 1) // groups, (n + 3) // 4, 0, 0, 0)


def _snake_wave(row):
    return row % 4 if (row // 4) % 2 == 0 else 3 - row % 4


def _diag_count(g, w):
    return sum(g - i for i in range(g) if _snake_wave(i) == w)


def gram_path(n, rows, variant=0, aligned=True):
    """``launch_gram_sym``'s choice: ``form`` 'split' (the split-K TN GEMM: fewer than three column tiles, fewer than 4096 rows, knob 1),
    'sym' (one group, CT <= 13) or 'units' (groups of GS column tiles); ``lds``: the LDS-staged kernels (even n, not GS = 11)"""
    ct = (n + 15) // 16
    if variant == 1 or ct < 3 or rows < 4096:
        return GramPath("split", ct, 0, 0, False)
    lds = variant != 2 and n % 2 == 0 and aligned
    if ct <= 13:
        return GramPath("sym", ct, ct, 1, lds)
    if (ct + 10) // 11 > 20:
        return GramPath("split", ct, 0, 0, False)
    best, gs, ng = 1e300, 11, (ct + 10) // 11
    for g in range(7, 12):
        k = (ct + g - 1) // g
        wt = max(_diag_count(g, w) for w in range(4))
        cost = (0.5 * k * (k - 1) * ((g + 3) // 4) * g + k * wt) * (1.12 if g == 11 else 1.0)
        if cost < best - 1e-9:
            best, gs, ng = cost, g, k
    return GramPath("units", ct, gs, ng, lds and gs < 11)


def gram_slices(rows, override=0):
    """K slices of the symmetric kernels where one launch is less than one round of workgroups (every shape of the tests):
    ``(slices, rows per slice)``"""
    cap = max(1, (rows + 1023) // 1024)
    nz = min(override, cap) if override > 0 else cap
    kchunk = (((rows + nz - 1) // nz) + 3) & ~3
    return (rows + kchunk - 1) // kchunk, kchunk


# ---------------------------------------------------------------------------------------------------------------- longdouble
def sample_rows(rows, seed=0, edge=64, random=448):
    """the first and the last ``edge`` rows, ``edge`` rows around row 32 x 2048 (where the second tile per wave of the persistent
    kernels begins) and ``random`` more"""
    mid = 32 * 2048
    idx = set(range(min(edge, rows))) | set(range(max(rows - edge, 0), rows))
    if rows > mid:
        idx |= set(range(mid - edge // 2, min(mid + edge // 2, rows)))
    idx |= set(np.random.default_rng(seed).integers(0, rows, random).tolist())
    return np.array(sorted(idx))


def sampled_longdouble(V, S, rows_idx):
    """rows ``rows_idx`` of ``V^T S`` in longdouble and their entry-wise bound ``gamma(n + 2) |V|^T |S|`` for a float64 dot product
    of n terms in any order"""
    n = V.shape[0]
    Vs = np.ascontiguousarray(V[:, rows_idx].T)
    ref = Vs.astype(LD) @ S.astype(LD)
    bound = gamma(n + 2) * (np.abs(Vs) @ np.abs(S))
    return ref, bound


def gram_longdouble(Y):
    """``Y^T Y`` in longdouble and the bound ``gamma(rows + 8) |Y|^T |Y|``"""
    YL = Y.astype(LD)
    return YL.T @ YL, gamma(Y.shape[0] + 8) * (np.abs(Y).T @ np.abs(Y))


def worst(got, ref, bound):
    """largest error / bound (entries whose bound is zero must be exact)"""
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    zero = bound == 0
    if np.any(err[zero] != 0):
        return np.inf
    return float((err[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.0


# ---------------------------------------------------------------------------------------------------------------- restatements
def restated_ritz(V, S, plant=None):
    """``Y = V^T S`` the kernels' way: 32-row tiles of ``Y``, accumulated over k-steps of four basis rows, column tiles of 16 with
    adjacent full tiles paired.  ``plant``: 'last_kstep' (the last k-step dropped), 'pair_swap' (the two tiles of the first column pair
    stored in each other's place), 'ragged_row' (the last row of a ragged last row tile not stored: the buffer's old content stays)"""
    n, rows = V.shape
    ks = (n + 3) // 4
    Y = np.full((rows, n), -7.0)  # what the buffer held before
    acc = np.zeros((rows, n))
    for t in range(ks - 1 if plant == "last_kstep" else ks):
        acc += V[4 * t: 4 * t + 4].T @ S[4 * t: 4 * t + 4]
    if plant == "pair_swap":
        assert n >= 32
        acc[:, 0:32] = np.concatenate([acc[:, 16:32], acc[:, 0:16]], axis=1)
    stored = rows - 1 if plant == "ragged_row" else rows
    assert plant != "ragged_row" or rows % 32 != 0
    Y[:stored] = acc[:stored]
    return Y


def restated_gram(Y, slices, plant=None):
    """``G = Y^T Y`` the symmetric kernels' way: the upper 16 x 16 tiles of every K slice, the slices added in order, the result
    mirrored.  ``plant``: 'zero_tile' (the off-diagonal tile (0, 1) never computed), 'no_mirror' (the lower tiles left zero),
    'slice_twice' (the last K slice added twice)"""
    rows, n = Y.shape
    kchunk = (((rows + slices - 1) // slices) + 3) & ~3
    tile = np.arange(n) // 16
    upper = tile[:, None] <= tile[None, :]
    G = np.zeros((n, n))
    starts = list(range(0, rows, kchunk))
    for k0 in starts + ([starts[-1]] if plant == "slice_twice" else []):
        Ys = Y[k0: k0 + kchunk]
        G += np.where(upper, Ys.T @ Ys, 0.0)
    if plant == "zero_tile":
        assert n > 16
        G[0:16, 16:32] = 0.0
    if plant != "no_mirror":
        G = np.where(upper, G, G.T)
    return G
