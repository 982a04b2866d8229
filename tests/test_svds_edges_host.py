"""The builders of tests/test_gpu_svds_edges.py, checked on the CPU for the properties the device tests rely on, and the solver
scenarios of that file (tiny shapes, an exhausted short space, the no-convergence counts, the matrices that share one handle) on
lanczos_amd.svds' NumPy backend.

The edge matrix is made for the work-item plan of the rectangular product (rect_plan / k_spmv_rect, lanczos_amd/csrc/lz_gk.hip):
row blocks of at most `cap` entries and at most 512 rows, segments of at most `cap` entries for longer rows.  What it has to
contain is stated here from the row lengths and the row offsets alone - never from a copy of the plan - so that a later edit of a
builder cannot silently stop covering a case.

Bars (tests/test_svds_host.py): values 1e-10 sigma_max, residuals 1e-9 sigma_max, orthonormality 1e-12 (check_triplets)."""
import functools

import numpy as np
import pytest
import scipy.sparse
from scipy.sparse.linalg import ArpackNoConvergence
from test_svds_host import check_triplets, host_svds, random_sparse

from lanczos_amd.svds import NumpyGKBackend, _pack

CAPS = (256, 4096, 8190)  # knob 4 at its lower clamp, the default tile, the upper clamp
DEFAULT_CAP = 4096        # gk_fill_meta's tile when the knob is unset
KINDS = ("wide", "wide-no-padding", "tall", "long-first")
ROW_LIMIT = 512           # rows per block
PAD = 32                  # doubles a basis row is padded to (lz_padded_rows)


def from_lengths(lengths, ncols, seed, integer=False):
    """CSR with the given row lengths: the columns of a row drawn without replacement and sorted; values standard normal, or
    (integer=True) integers of [-8, 8] without 0 stored as float64.  The pattern depends on (lengths, ncols, seed) only."""
    lengths = np.asarray(lengths, dtype=np.int64)
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    indices = np.empty(indptr[-1], dtype=np.int32)
    for r in np.flatnonzero(lengths):
        indices[indptr[r]:indptr[r + 1]] = np.sort(rng.choice(ncols, size=lengths[r], replace=False))
    vrng = np.random.default_rng([seed, 1])
    if integer:
        data = (vrng.integers(1, 9, indptr[-1]) * vrng.choice([-1, 1], indptr[-1])).astype(np.float64)
    else:
        data = vrng.standard_normal(indptr[-1])
    return scipy.sparse.csr_matrix((data, indices, indptr.astype(np.int32)), shape=(len(lengths), ncols))


def edge_lengths(cap, tail, long_first=False):
    """(row lengths, ncols) of the edge matrix for a tile of `cap` entries"""
    lengths = [3, cap, cap + 1, 0, 0, 2 * cap, 2 * cap + 1, 1] + [0] * 600 + [cap - 1, 1, 2, cap - 2] + [5] * tail + [3 * cap + 7]
    if long_first:
        lengths = lengths[-1:] + lengths[:-1]
    return np.array(lengths, dtype=np.int64), 3 * cap + 57


def edge_case(cap, kind):
    """(row lengths, ncols) of one of KINDS"""
    ncols = 3 * cap + 57
    if kind == "wide":
        return edge_lengths(cap, 0)
    if kind == "wide-no-padding":
        return edge_lengths(cap, 27)
    if kind == "long-first":
        return edge_lengths(cap, 0, long_first=True)
    assert kind == "tall"
    tail = ncols - 613
    while (613 + tail) % PAD == 0 or 613 + tail < ncols:
        tail += 1
    return edge_lengths(cap, tail)


@functools.lru_cache(maxsize=None)
def edge_matrix(cap, kind, integer=False):
    """(cached: treat the result as read-only)"""
    lengths, ncols = edge_case(cap, kind)
    return from_lengths(lengths, ncols, seed=cap + KINDS.index(kind), integer=integer)


def step_matrix(p, q):
    """(A, A^T) of the extension tests in tests/test_gpu_svds.py"""
    return _pack(random_sparse(p, q, density=8.0 / q, seed=22))[:2]


# svds at the size limits: (M, N, k, ncv), every one with ncv = min(M, N) (an exhausted short space), three below one padded row
TINY = [(7, 3, 1, 3), (3, 7, 1, 3), (33, 33, 4, 33), (64, 32, 3, 32), (40, 31, 2, 31), (1000, 5, 2, 5), (60, 25, 4, 25)]


def tiny_matrix(M, N):
    return random_sparse(M, N, density=0.6, seed=M + N)


# no convergence: shape -> converged triplets after one cycle at NOCONV_TOL (k = 6).  The first cycle's estimates relative to
# sigma_max are 1.1e-5, 1.2e-4, 2.5e-3, ... and 1.0e-5, 1.6e-2, ...: the nearest one is 4x from the tolerance on either side.
NOCONV = {(300, 120): 2, (120, 300): 1}
NOCONV_TOL = 5e-4


def shared_handle_calls():
    """the calls of the one-handle test in order: (name, matrix, keyword arguments of svds)"""
    small = random_sparse(300, 120)
    big = edge_matrix(256, "tall")
    return [("small", small, {"ncv": 20}), ("big", big, {"ncv": 40}), ("small-12", small, {"ncv": 12}), ("small-again", small, {"ncv": 20})]


# ------------------------------------------------------------------ the builders


def test_from_lengths_gives_what_it_says():
    lengths = [0, 3, 40, 0, 1, 17]
    A = from_lengths(lengths, 40, seed=3)
    assert A.shape == (6, 40) and np.array_equal(np.diff(A.indptr), lengths)
    assert A.has_canonical_format  # sorted columns without duplicates
    assert A.indices.min() >= 0 and A.indices.max() < 40
    assert np.array_equal(A[2].indices, np.arange(40))
    Z = from_lengths(lengths, 40, seed=3, integer=True)
    assert np.array_equal(Z.indices, A.indices) and np.array_equal(Z.indptr, A.indptr)  # same pattern
    assert Z.data.dtype == np.float64 and np.array_equal(Z.data, np.round(Z.data))
    assert np.abs(Z.data).min() >= 1 and np.abs(Z.data).max() <= 8
    big = from_lengths([3000], 3000, seed=4, integer=True).data
    assert set(np.unique(big)) == set(range(-8, 0)) | set(range(1, 9))
    g = from_lengths([3000], 3000, seed=4).data
    assert abs(g.mean()) < 0.1 and abs(g.std() - 1.0) < 0.1
    assert not np.array_equal(from_lengths(lengths, 40, seed=5).indices, A.indices)


def test_edge_lengths_is_the_stated_list():
    for cap in CAPS:
        lengths, ncols = edge_lengths(cap, 4)
        assert ncols == 3 * cap + 57
        assert list(lengths[:8]) == [3, cap, cap + 1, 0, 0, 2 * cap, 2 * cap + 1, 1]
        assert not lengths[8:608].any() and len(lengths) == 8 + 600 + 4 + 4 + 1
        assert list(lengths[608:]) == [cap - 1, 1, 2, cap - 2, 5, 5, 5, 5, 3 * cap + 7]
        first, _ = edge_lengths(cap, 4, long_first=True)
        assert first[0] == 3 * cap + 7 and np.array_equal(first[1:], lengths[:-1])


def runs_that_fit(lengths, cap):
    """for every start row the number of consecutive rows whose entries together are at most cap"""
    off = np.concatenate([[0], np.cumsum(lengths)])
    return np.searchsorted(off, off[:-1] + cap, side="right") - 1 - np.arange(len(lengths))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cap", CAPS)
def test_edge_case_covers_the_plan(cap, kind):
    lengths, ncols = edge_case(cap, kind)
    rows = len(lengths)
    off = np.concatenate([[0], np.cumsum(lengths)])
    assert lengths.max() <= ncols  # (columns without replacement)
    assert rows <= 50_000 and off[-1] <= 250_000
    # the shape and the padding each kind is there for
    if kind == "tall":
        assert rows >= ncols and rows % PAD != 0
    else:
        assert rows < ncols
    if kind in ("wide", "long-first"):
        assert rows == 613 and -rows % PAD == 27
    if kind == "wide-no-padding":
        assert rows == 640 and rows % PAD == 0
    # a row of exactly cap entries that starts at an odd entry: a full tile whose even-aligned image needs cap + 2 slots
    # (long-first moves every row by an odd count of entries: there the odd full tile is made of two rows)
    full = np.flatnonzero(lengths == cap)
    assert len(full) == 1
    whole = (lengths > 0) & np.isin(off[:-1] + cap, off)  # rows at which a run of whole rows with exactly cap entries starts
    assert (off[full] % 2 == 1).any() if kind != "long-first" else (whole & (off[:-1] % 2 == 1)).any()
    # ... and full tiles made of several rows, at even entries (long-first: odd ones)
    pair = np.flatnonzero((lengths[:-1] + lengths[1:] == cap) & (lengths[:-1] > 0) & (lengths[1:] > 0))
    assert len(pair) == 2 and (off[pair] % 2 == (1 if kind == "long-first" else 0)).all()
    # the shortest split row (cap + 1: a segment of one entry), exact multiples of the segment length and one entry more
    for n in (cap + 1, 2 * cap, 2 * cap + 1, 3 * cap + 7):
        assert (lengths == n).sum() == 1
    # empty rows directly in front of a long row, and a one-entry row directly behind one
    r = int(np.flatnonzero(lengths == 2 * cap)[0])
    assert lengths[r - 1] == 0 and lengths[r - 2] == 0
    r = int(np.flatnonzero(lengths == 2 * cap + 1)[0])
    assert lengths[r + 1] == 1
    # more than 512 consecutive rows fit the tile: the row limit, not the tile, ends that block
    assert runs_that_fit(lengths, cap).max() > ROW_LIMIT
    # a long row first or last: the first or the last work item is a segment
    if kind == "long-first":
        assert lengths[0] > cap and lengths[-1] <= cap
    else:
        assert lengths[-1] > cap and lengths[0] <= cap
    # both paths in one matrix
    assert (lengths > cap).sum() == 4 and ((lengths > 0) & (lengths <= cap)).sum() >= 7


def test_edge_matrix_values_keep_integer_sums_exact():
    """|entry| <= 8, |x| <= 4 and at most 3 cap + 7 entries per row: every partial sum is an integer below 2^20, exact in any order"""
    for cap in CAPS:
        lengths, _ = edge_case(cap, "tall")
        assert 8 * 4 * lengths.max() < 2**20
    Z = edge_matrix(256, "wide", integer=True)
    G = edge_matrix(256, "wide")
    assert np.array_equal(Z.indices, G.indices) and np.array_equal(np.diff(Z.indptr), edge_case(256, "wide")[0])
    ZT = Z.T.tocsr()
    assert 8 * 4 * np.diff(ZT.indptr).max() < 2**20


def test_longdouble_carries_the_reference():
    """the split-row bound's factor 1.01 assumes a reference with at least 64 bits of significand"""
    assert np.finfo(np.longdouble).eps <= 2.0**-63


# ------------------------------------------------------------------ the solver scenarios on the NumPy backend


@pytest.mark.parametrize("M,N,k,ncv", TINY)
def test_tiny_shapes_converge_in_one_cycle(M, N, k, ncv):
    assert ncv == min(M, N)
    A = tiny_matrix(M, N)
    info = {}
    u, s, vh = host_svds(A, k=k, ncv=ncv, info=info)
    check_triplets(A, u, s, vh, "LM", k, info)
    assert info["cycles"] == 1 and info["breakdowns"] == 0


def test_exhausted_space_leaves_a_dead_last_row():
    """ncv = min(M, N): beta_{m-1} vanishes and V[m] is noise (NaN or a normalised rounding error); nothing reads it afterwards"""
    M, N, k, ncv = TINY[-1]
    A = tiny_matrix(M, N)
    be = NumpyGKBackend(_pack(A)[0])
    be.begin(ncv, np.random.default_rng(0).uniform(-1.0, 1.0, N))
    _, alpha, beta = be.extend(0, ncv)
    assert beta[ncv - 1] <= 1e-12 * alpha.max()
    assert np.all(beta[: ncv - 1] > 1e-8 * alpha.max())
    backends = []
    info = {}
    u, s, vh = host_svds(A, k=k, ncv=ncv, info=info, backends=backends)
    check_triplets(A, u, s, vh, "LM", k, info)
    assert np.isfinite(backends[0].U[:k]).all() and np.isfinite(backends[0].V[:k]).all()


@pytest.mark.parametrize("shape", sorted(NOCONV))
def test_no_convergence_counts(shape):
    A = random_sparse(*shape)
    with pytest.raises(ArpackNoConvergence) as ei:
        host_svds(A, k=6, tol=NOCONV_TOL, maxiter=1)
    err = ei.value
    nconv = NOCONV[shape]
    D = A.toarray()
    ref = np.linalg.svd(D, compute_uv=False)
    assert err.nconv == nconv and err.eigenvalues.shape == (nconv,) and err.eigenvectors.shape == (shape[1], nconv)
    assert np.all(np.diff(err.eigenvalues) > 0)
    assert np.abs(err.eigenvalues - ref[:nconv][::-1]).max() <= NOCONV_TOL * ref[0]
    assert np.abs(err.eigenvectors.T @ err.eigenvectors - np.eye(nconv)).max() <= 1e-12
    assert np.abs(np.linalg.norm(D @ err.eigenvectors, axis=0) - err.eigenvalues).max() <= NOCONV_TOL * ref[0]
    # the margin the device test relies on: a tolerance 3x smaller or larger gives the same counts
    for tol in (NOCONV_TOL / 3, NOCONV_TOL * 3):
        with pytest.raises(ArpackNoConvergence) as ei:
            host_svds(A, k=6, tol=tol, maxiter=1)
        assert ei.value.nconv == nconv


def test_shared_handle_calls_converge():
    for name, A, kw in shared_handle_calls():
        info = {}
        u, s, vh = host_svds(A, k=6, info=info, **kw)
        check_triplets(A, u, s, vh, "LM", 6, info)
        assert info["breakdowns"] == 0, name
