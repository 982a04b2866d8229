"""Non-canonical CSR for the tests: rows whose stored entries are unsorted, hold unsummed duplicates and explicit zeros - all of it
legal CSR, and what ``A @ B``, ``A[:, perm]``, ``hstack`` and ``csr_matrix((data, indices, indptr))`` hand a user.  SciPy's ``B @ x``
adds a row's stored entries one after the other, in stored order; so must every kernel that claims SciPy's bits.

``noncanonical`` / ``noncanonical_hermitian`` build such matrices; ``stored_product`` is the longdouble (clongdouble) sum of the stored
entries with the entry-wise forward bound of ``bicgstab_reference.product_bound`` (``hermitian_reference.product_bound`` for complex
input); ``stored_sum_float64`` is the sequential float64 sum in stored order (SciPy's bits); ``sorted_order`` and
``one_value_per_column`` are two wrong products ("mutants") that the references must tell from the right one.

Beware of SciPy itself: ``abs(B)``, ``B.power()``, ``B.multiply()`` and a few more first sum the duplicates of ``B`` IN PLACE (and a
``sp.csr_matrix(B)`` shares B's arrays, so a wrapper does not protect it): a reference that calls one of them changes the matrix under
test to the canonical one.  ``stored_abs`` is the entry-wise ``|B|``; the tests assert ``untouched`` around what they share.

A plain module: no fixtures, nothing collected from it; of the package it imports ``synthetic`` alone, for the device tests' matrices."""
import numpy as np
import scipy.sparse as sp
from bicgstab_reference import LD, Operator, product_bound

CLD = np.clongdouble
PAD_ENTRIES = 5       # ``padded=True``: entries behind ``indptr[-1]``
PAD_VALUE = 1.0e300   # their value: a kernel that reads one shows it


def _canonical(A):
    C = sp.csr_matrix(A, copy=True)
    C.sum_duplicates()
    C.sort_indices()
    return C


def _exact_split(v, draw):
    """``(t, v - t)`` with ``t + (v - t) == v`` in floating point (a few draws find one): the summed matrix is then ``A`` itself"""
    for _ in range(64):
        t = draw()
        u = v - t
        if t + u == v:
            return t, u
    return v, v - v


def _assemble(rows, shape, dtype, padded):
    lens = np.array([len(c) for c, _ in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    data = np.concatenate([np.asarray(v, dtype=dtype) for _, v in rows] + [np.zeros(0, dtype=dtype)]).astype(dtype)
    B = sp.csr_matrix((data, indices, indptr), shape=shape)
    if padded:  # (the constructor prunes such a tail; arrays assigned later, or left by an in-place operation, keep it)
        B.indices = np.concatenate([indices, np.zeros(PAD_ENTRIES, dtype=np.int32)])
        B.data = np.concatenate([data, np.full(PAD_ENTRIES, PAD_VALUE, dtype=dtype)])
    assert B.indices.dtype == np.int32 and B.indptr.dtype == np.int32 and B.nnz == int(indptr[-1])
    return B


def noncanonical(A, seed, dup=True, zeros=True, shuffle=True, every=4, same_order=False, padded=False, hermitian=False, offdiag=False,
                 integer=False):
    """The canonical CSR of ``A`` made non-canonical.  In every row with an entry, except rows with ``r % every == every - 1`` (those stay
    canonical; ``every=None``: no row is spared): ``dup`` splits one random entry ``v`` into the stored entries ``t`` and ``v - t`` of one
    column (``t`` normal), ``zeros`` appends one explicit ``0.0`` at a random column (which may be occupied), ``shuffle`` permutes the
    row's entries.  Empty rows stay empty.  ``offdiag=True``: the split entry and the explicit zero keep off the diagonal.
    ``integer=True``: ``t`` is a small integer (an integer matrix stays one: every sum of it is exact in any order).

    ``same_order=True`` (a matrix with as many entries in every row; no row is spared): the entry at one fixed position of the sorted row
    (the next one where that is the diagonal) is split with one ``t`` for all rows, the explicit zero goes to the column of another fixed
    off-diagonal position, and ONE permutation of the positions is applied to every row - a stencil keeps a handful of row classes, with
    its diagonal wherever the permutation puts it.

    ``padded=True``: ``indices`` / ``data`` are longer than ``indptr[-1]`` (SciPy allows that); the tail holds ``PAD_VALUE``.
    ``hermitian=True`` (complex input): splits are complex and exact, ``t + (v - t) == v``, so the matrix stays Hermitian as a matrix -
    the sum of the stored entries at ``(i, j)`` is the conjugate of the sum at ``(j, i)`` - though not entry by entry.

    Returns ``csr_matrix((data, indices, indptr))`` with int32 indices, neither sorted nor canonical."""
    C = _canonical(A)
    n, ncols = C.shape
    cplx = np.dtype(C.dtype).kind == "c"
    dtype = np.complex128 if cplx else np.float64
    rng = np.random.default_rng(seed)
    normal = (lambda: complex(rng.standard_normal(), rng.standard_normal())) if cplx else (lambda: float(rng.standard_normal()))
    if integer:
        normal = lambda: float(rng.integers(1, 4))  # noqa: E731
    lens = np.diff(C.indptr)
    rows = []
    if same_order:
        K = int(lens[0])
        assert np.all(lens == K) and K >= 3
        j_dup, t_all = int(rng.integers(K)), normal()
        j_zero = int(rng.integers(K))
        Kn = K + int(bool(dup)) + int(bool(zeros))
        perm = rng.permutation(Kn) if shuffle else np.arange(Kn)
        while shuffle and np.array_equal(perm, np.arange(Kn)):
            perm = rng.permutation(Kn)
    for r in range(n):
        a, b = int(C.indptr[r]), int(C.indptr[r + 1])
        cols, vals = list(C.indices[a:b]), list(C.data[a:b].astype(dtype))
        spared = (not same_order) and every is not None and r % every == every - 1
        if b > a and not spared:
            if same_order:
                off = [k for k in range(K) if cols[k] != r]  # positions off the diagonal, in sorted order
                jd = off[j_dup % len(off)]
                jz = off[(j_dup + 1 + j_zero % (len(off) - 1)) % len(off)]  # another one
                if dup:
                    v = vals[jd]
                    vals[jd] = t_all
                    cols.append(cols[jd])
                    vals.append(v - t_all)
                if zeros:
                    cols.append(cols[jz])
                    vals.append(dtype(0.0))
                cols, vals = [cols[p] for p in perm], [vals[p] for p in perm]
            else:
                cand = [k for k in range(len(cols)) if cols[k] != r] if offdiag else list(range(len(cols)))
                if dup and cand:
                    j = cand[int(rng.integers(len(cand)))]
                    t, u = _exact_split(vals[j], normal) if hermitian else (normal(), None)
                    u = vals[j] - t if u is None else u
                    vals[j] = t
                    cols.append(cols[j])
                    vals.append(u)
                if zeros:
                    c = int(rng.integers(ncols))
                    while offdiag and c == r:
                        c = int(rng.integers(ncols))
                    cols.append(c)
                    vals.append(dtype(0.0))
                if shuffle:
                    p = rng.permutation(len(cols))
                    cols, vals = [cols[q] for q in p], [vals[q] for q in p]
        rows.append((cols, vals))
    B = _assemble(rows, C.shape, dtype, padded)
    assert not B.has_sorted_indices and not B.has_canonical_format
    return B


def noncanonical_hermitian(A, seed, **kw):
    """the complex twin: ``A`` complex Hermitian; entries are split in the complex plane, exactly, so that the stored entries still sum
    to a Hermitian matrix (asserted), which no longer is Hermitian entry by entry"""
    A = sp.csr_matrix(A).astype(np.complex128)
    assert abs(A - A.getH()).max() == 0.0
    B = noncanonical(A, seed, hermitian=True, **kw)
    S = _canonical(trimmed(B))
    assert abs(S - S.getH()).max() == 0.0
    return B


def reshuffled(B, seed):
    """the stored entries of every row of ``B`` in another random order (nothing added, nothing summed)"""
    B = trimmed(B)
    rng = np.random.default_rng(seed)
    order = np.arange(B.nnz)
    for r in range(B.shape[0]):
        a, b = int(B.indptr[r]), int(B.indptr[r + 1])
        order[a:b] = a + rng.permutation(b - a)
    return sp.csr_matrix((B.data[order], B.indices[order].astype(np.int32), B.indptr.copy()), shape=B.shape)


def trimmed(B):
    """``B`` without the entries behind ``indptr[-1]`` (``B`` itself where there are none)"""
    nnz = int(B.indptr[-1])
    if len(B.data) == nnz:
        return B
    return sp.csr_matrix((B.data[:nnz].copy(), B.indices[:nnz].copy(), B.indptr.copy()), shape=B.shape)


def stored_abs(B):
    """``|B|`` entry by entry as stored, with arrays of its own (SciPy's ``abs(B)`` would sum B's duplicates first, in place)"""
    T = trimmed(B)
    return sp.csr_matrix((np.abs(T.data), T.indices.copy(), T.indptr.copy()), shape=B.shape)


def as_stored(B):
    """a copy of ``B`` that SciPy takes for canonical, for a reference that calls ``abs(A)`` on the very object it is given: with the flag
    set SciPy sums nothing, ``abs`` is entry by entry as stored and ``@`` walks the stored entries as always (neither needs sorted
    rows).  A ``sp.csr_matrix(A)`` wrapper does not inherit the flag.  Never hand it to the code under test."""
    C = trimmed(B).copy()
    C.has_canonical_format = True
    return C


def arrays_of(B):
    """copies of the three arrays as the caller holds them, and the sorted flag: what a call must leave as it found it"""
    return B.indptr.copy(), B.indices.copy(), B.data.copy(), bool(B.has_sorted_indices)


def untouched(B, before):
    indptr, indices, data, flag = before
    same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()  # noqa: E731  (bit for bit, NaN and -0.0 too)
    return same(B.indptr, indptr) and same(B.indices, indices) and same(B.data, data) and bool(B.has_sorted_indices) == flag


# ---------------------------------------------------------------- the references
def _nonempty(B):
    """``(rows with an entry, the CSR matrix of those rows alone)``: what ``bicgstab_reference.Operator`` accepts"""
    B = trimmed(B)
    full = np.diff(B.indptr) > 0
    sub = sp.csr_matrix((B.data, B.indices, np.concatenate([B.indptr[:-1][full], B.indptr[-1:]])), shape=(int(full.sum()), B.shape[1]))
    return full, sub


def stored_product(B, x):
    """``(y, bound)``: ``y`` the longdouble (clongdouble for a complex ``B`` or ``x``) sum of every row's stored entries times ``x``, zero
    for an empty row, and the entry-wise bound of a float64 product that adds those entries in any order:
    real ``gamma(stored row length) (|B||x|)_i`` with ``|B|`` entry by entry as stored (``bicgstab_reference.product_bound``),
    complex ``hermitian_reference.product_bound``"""
    if np.dtype(B.dtype).kind == "c" or np.iscomplexobj(x):
        import hermitian_reference as hr

        T = trimmed(B)
        return hr.matvec(T, x), hr.product_bound(T, x)
    full, sub = _nonempty(B)
    y, bound = np.zeros(B.shape[0], dtype=LD), np.zeros(B.shape[0])
    if full.any():
        op = Operator(sub)
        y[full] = op.matvec(x)
        bound[full] = product_bound(op, x)
    return y, bound


def _sequential(indptr, indices, data, x, n):
    y = np.zeros(n, dtype=np.result_type(data.dtype, np.asarray(x).dtype))
    lens = np.diff(indptr)
    start = indptr[:-1].astype(np.int64)
    for k in range(int(lens.max()) if n else 0):
        rows = np.flatnonzero(lens > k)
        at = start[rows] + k
        y[rows] = y[rows] + data[at] * x[indices[at]]
    return y


def stored_sum_float64(B, x):
    """the plain sequential float64 loop over every row's entries in stored order, one position of all rows at a time: SciPy's ``B @ x``
    bit for bit.  (Real input: NumPy's complex multiplication is not SciPy's to the bit.)"""
    assert np.dtype(B.dtype).kind == "f" and not np.iscomplexobj(x)
    return _sequential(B.indptr, B.indices, B.data, np.asarray(x), B.shape[0])


# ---------------------------------------------------------------- two wrong products
def sorted_order(B, x):
    """MUTANT: every row summed in column order (what a layout does that sorts, or assumes sorted rows)"""
    B = trimmed(B)
    rows = np.repeat(np.arange(B.shape[0]), np.diff(B.indptr))
    order = np.lexsort((B.indices, rows))  # stable: duplicates keep their stored order
    return _sequential(B.indptr, B.indices[order], B.data[order], np.asarray(x), B.shape[0])


def one_value_per_column(B, x):
    """MUTANT: a column stored more than once in a row takes the LAST of its values at every one of its positions (what a layout does that
    keeps one slot per column)"""
    B = trimmed(B)
    rows = np.repeat(np.arange(B.shape[0]), np.diff(B.indptr))
    order = np.lexsort((np.arange(B.nnz), B.indices, rows))
    key = rows[order].astype(np.int64) * B.shape[1] + B.indices[order]
    last = np.flatnonzero(np.append(key[1:] != key[:-1], True))  # the last entry of every run of one (row, column)
    run = np.searchsorted(last, np.arange(B.nnz))
    data = np.empty_like(B.data)
    data[order] = B.data[order][last[run]]
    return _sequential(B.indptr, B.indices, data, np.asarray(x), B.shape[0])


def duplicate_rows(B, x):
    """rows that hold a duplicate of a non-zero entry with ``x`` non-zero there: where ``one_value_per_column`` must be caught"""
    B = trimmed(B)
    rows = np.repeat(np.arange(B.shape[0]), np.diff(B.indptr))
    key = rows.astype(np.int64) * B.shape[1] + B.indices
    uniq, inv, count = np.unique(key, return_inverse=True, return_counts=True)
    nz = np.zeros(len(uniq), dtype=bool)
    np.logical_or.at(nz, inv, B.data != 0)
    hit = (count[inv] > 1) & nz[inv] & (np.asarray(x)[B.indices] != 0)
    out = np.zeros(B.shape[0], dtype=bool)
    out[rows[hit]] = True
    return out


def order_sensitive_share(B, x):
    """the share of the rows in which ``sorted_order`` differs in bits from the stored-order sum"""
    a, b = sorted_order(B, x), stored_sum_float64(B, x)
    return float(np.mean(a != b)) if len(a) else 0.0


# ---------------------------------------------------------------- the matrices of the device tests (tests/test_gpu_noncanonical.py)
# One registry, so that tests/test_noncanonical_host.py can hold every matrix and x of a bit-exact device case to the condition that
# makes bit-equality a test of the ORDER: summed in column order, at least a quarter of the rows get other bits.
def sym_random(n, seed=None):
    """symmetric, about seven entries a row, ragged (tests/test_gpu_cg.py's step matrices); dense for ``n <= 5``"""
    rng = np.random.default_rng(n if seed is None else seed)
    if n <= 5:
        G = rng.standard_normal((n, n))
        return sp.csr_matrix(G + G.T)
    S = sp.random(n, n, density=3.0 / n, random_state=rng, data_rvs=rng.standard_normal)
    return (S + S.T + sp.diags(rng.standard_normal(n))).tocsr()


def long_row_3000():
    """tests/test_gpu_kernels.py's ``ragged_3000``: 24 entries a row on average and one row (and column) of 3000"""
    rng = np.random.default_rng(5)
    R = sp.random(3000, 3000, density=0.004, random_state=rng, format="csr")
    E = sp.csr_matrix((rng.standard_normal(3000), (np.full(3000, 17), np.arange(3000))), shape=(3000, 3000))
    return (R + R.T + sp.diags(rng.standard_normal(3000)) + E + E.T).tocsr()


def fixed_k_random(M, K, seed):
    """tests/test_gpu_kernels.py's ``_fixed_k_random``: M rows of exactly K entries at random distinct columns, real values"""
    rng = np.random.default_rng(seed)
    W = min(M, 256)
    offs = np.argsort(rng.random((M, W)), axis=1)[:, :K]
    cols = np.sort(rng.integers(0, M - W + 1, (M, 1)) + offs, axis=1)
    return sp.csr_matrix((rng.standard_normal(M * K), cols.ravel().astype(np.int32), np.arange(0, M * K + 1, K, dtype=np.int32)), shape=(M, M))


def fixed_k_case(K, M):
    """fixed-K rows, shuffled: K = 5 and 27 the random rows themselves, K = 7 the K = 5 rows plus one duplicate and one explicit zero"""
    if K == 7:
        return noncanonical(fixed_k_random(M, 5, seed=5 * M), seed=7 * M, every=None)
    return noncanonical(fixed_k_random(M, K, seed=K * M), seed=K * M + 1, dup=False, zeros=False, every=None)


def stencil(name):
    from lanczos_amd import synthetic

    if name == "lap2d_37x29":
        return synthetic.laplacian_2d_5pt(37, 29).to_scipy()
    if name == "lap3d_21x17x13":
        return synthetic.laplacian_3d_7pt(21, 17, 13).to_scipy()
    assert name == "stencil27"
    return stencil27()


def stencil27(nx=9, ny=8, nz=7):
    """a periodic 27-point stencil with constant, non-symmetric coefficients (504 rows: with a random diagonal more than 256 classes of
    offsets and values, so that the diagonal has to stream)"""
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    row = ((z * ny + y) * nx + x).ravel()
    rows, cols, vals = [], [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                rows.append(row)
                cols.append(((((z + dz) % nz) * ny + (y + dy) % ny) * nx + (x + dx) % nx).ravel())
                w = 26.0 if (dx, dy, dz) == (0, 0, 0) else -(1.0 + 0.25 * dx + 0.125 * dy + 0.0625 * dz) / (abs(dx) + abs(dy) + abs(dz))
                vals.append(np.full(row.size, w))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nx * ny * nz,) * 2)
    assert np.all(np.diff(_canonical(A).indptr) == 27)
    return A


def with_potential(A, seed=5):
    return (A + sp.diags(np.random.default_rng(seed).uniform(-1, 1, A.shape[0]))).tocsr()


def diagonal_position(B):
    """the position of the diagonal in every row of a fixed-K matrix (-1: none)"""
    B = trimmed(B)
    K = int(B.indptr[1])
    on = B.indices.reshape(-1, K) == np.arange(B.shape[0])[:, None]
    return np.where(on.any(axis=1), on.argmax(axis=1), -1)


def graph_20000():
    """``random_graph_laplacian(20000, 70000)`` with real values (products and partial sums really round), symmetric"""
    from lanczos_amd import synthetic

    G = synthetic.random_graph_laplacian(20000, 70000, seed=8).to_scipy().tocoo()
    rng = np.random.default_rng(11)
    lo, hi = np.minimum(G.row, G.col), np.maximum(G.row, G.col)
    key = lo.astype(np.int64) * 20000 + hi
    _, inv = np.unique(key, return_inverse=True)
    vals = rng.standard_normal(inv.max() + 1)[inv]  # one value per unordered pair: symmetric
    A = sp.csr_matrix((vals, (G.row, G.col)), shape=G.shape)
    A.sort_indices()
    return A


def without_diagonal(A, keep):
    """``A`` with the diagonal entry removed from the rows where ``keep`` is False"""
    C = _canonical(A).tocoo()
    drop = (C.row == C.col) & ~np.asarray(keep)[C.row]
    return sp.csr_matrix((C.data[~drop], (C.row[~drop], C.col[~drop])), shape=A.shape)


def zero_diagonal_only(A, seed):
    """``A`` without its diagonal, every row shuffled with an explicit 0.0 stored ON the diagonal: the diagonal is present only as a zero"""
    n = A.shape[0]
    C = _canonical(without_diagonal(A, np.zeros(n, dtype=bool)))
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n):
        a, b = int(C.indptr[r]), int(C.indptr[r + 1])
        cols, vals = list(C.indices[a:b]) + [r], list(C.data[a:b]) + [0.0]
        p = rng.permutation(len(cols))
        rows.append(([cols[q] for q in p], [vals[q] for q in p]))
    B = _assemble(rows, C.shape, np.float64, False)
    assert not B.has_sorted_indices
    return B


def first_and_last_only(n=257):
    """canonical but for its first and its last row"""
    C = _canonical(sym_random(n))
    rng = np.random.default_rng(n)
    rows = []
    for r in range(n):
        a, b = int(C.indptr[r]), int(C.indptr[r + 1])
        cols, vals = list(C.indices[a:b]), list(C.data[a:b])
        if r in (0, n - 1):
            cols, vals = cols + [cols[0], int(rng.integers(n))], vals + [0.25 * vals[0], 0.0]
            vals[0] = vals[0] - vals[-2]
            cols, vals = cols[::-1], vals[::-1]
        rows.append((cols, vals))
    B = _assemble(rows, C.shape, np.float64, False)
    assert not B.has_sorted_indices and not B.has_canonical_format
    return B


def x_of(B, seed=1):
    return np.random.default_rng(seed).uniform(-1, 1, B.shape[1])


ORDER_SHARE = 0.25  # the least share of rows whose bits the column-order sum must change, in every bit-exact case but the edge cases below
# edge cases that cannot meet it by construction: no entries at all, one row, and two non-canonical rows of 257
ORDER_EXEMPT = ("empty_257", "one_row", "first_and_last_257")

SCALAR, STREAM = 8, 32  # LZ_FLAG_SPMV_SCALAR, LZ_FLAG_SPMV_STREAM
T_FIXED_ROWS, T_PB_ENTRIES, T_SPMV_PLAN, T_FIXED_LAYOUT, T_CLS_GROUP = 5, 10, 14, 17, 23  # lz_set_tuning indices (asserted against _capi)


def class_count(B, values, diagonal=True):
    """the number of different rows of a fixed-K matrix up to translation, BY POSITION: tuples of offsets ``col - row``, with the values
    where ``values`` (``diagonal=False``: but the diagonal's)"""
    B = trimmed(B)
    K = int(B.indptr[1])
    off = B.indices.reshape(-1, K).astype(np.int64) - np.arange(B.shape[0])[:, None]
    key = off.astype(np.float64)
    if values:
        v = B.data.reshape(-1, K).copy()
        if not diagonal:
            v[off == 0] = 0.0
        key = np.concatenate([key, v], axis=1)
    return len(np.unique(key, axis=0))


_BUILT = {}


def _once(name, build):
    if name not in _BUILT:
        _BUILT[name] = build()
    return _BUILT[name]


def _same_order(name, seed=0, values=None, potential=False, **kw):
    A = stencil(name)
    if values == "random":
        A = _canonical(A)
        A.data = np.random.default_rng(7).standard_normal(A.nnz)
    if potential:
        A = with_potential(A)
    return noncanonical(A, seed=seed, same_order=True, **kw)


def product_cases():
    """``{name: case}`` of the real square product's device cases.  A case: ``build`` (-> B, built once), ``flags``, ``tune``
    (``[(index, value)]``), ``plan`` (what ``spmv_plan()`` must say), ``coding`` (``spmv_coding()[0]``, a tuple of the acceptable
    ones), ``classes`` (``None`` or how to count them: ``(values, diagonal)`` of ``class_count``)"""
    cases = {}

    def add(name, build, plan, flags=0, tune=(), coding=("none",), classes=None, matrix=None):
        key = matrix or name
        cases[name] = {"build": (lambda: _once(key, build)), "flags": flags, "tune": list(tune), "plan": plan, "coding": coding, "classes": classes}

    # ---- CSR-stream <0> and the scalar kernel
    ragged = {"ragged_5": lambda: noncanonical(sym_random(5), seed=5), "ragged_257": lambda: noncanonical(sym_random(257), seed=257),
              "ragged_257_padded": lambda: noncanonical(sym_random(257), seed=258, padded=True),
              "long_row_3000": lambda: noncanonical(long_row_3000(), seed=3),
              "empty_257": lambda: sp.csr_matrix((257, 257), dtype=np.float64),
              "one_row": lambda: sp.csr_matrix((np.array([0.75, 0.0, -2.0]), np.array([0, 0, 0], dtype=np.int32), np.array([0, 3], dtype=np.int32)), shape=(1, 1)),
              "first_and_last_257": first_and_last_only}
    for name, build in ragged.items():
        add(name, build, "csr-stream")
        add(name + "_scalar", build, "scalar", flags=SCALAR, matrix=name)
    # ---- fixed K on the CSR-order kernel (512- and 1024-row blocks), on CSR-stream <5 / 7>, and the uncoded ELL copy
    for K in (5, 7):
        for M in (1300, 2049):
            key = f"fixed_{K}_{M}"
            build = (lambda K=K, M=M: fixed_k_case(K, M))
            for rb in (512, 1024):
                add(f"{key}_rb{rb}", build, "fixed-k", tune=[(T_FIXED_LAYOUT, 1), (T_FIXED_ROWS, rb)], matrix=key)
            add(f"{key}_stream", build, "csr-stream", flags=STREAM, tune=[(T_FIXED_LAYOUT, 1)], matrix=key)
    for K, M in ((5, 1300), (7, 2049), (27, 777)):
        for layout in (2, 3):
            add(f"fixed_{K}_{M}_ell{layout}", (lambda K=K, M=M: fixed_k_case(K, M)), "fixed-k", tune=[(T_FIXED_LAYOUT, layout)], matrix=f"fixed_{K}_{M}")
    # ---- row-class coding
    for name in ("lap2d_37x29", "lap3d_21x17x13"):
        for group in (0, 1, 3):
            add(f"{name}_same_order_g{group}", (lambda name=name: _same_order(name, dup=False, zeros=False)), "fixed-k", tune=[(T_CLS_GROUP, group)],
                coding=("offsets+values",), classes=(True, True), matrix=name + "_same_order")
            add(f"{name}_potential_same_order_g{group}", (lambda name=name: _same_order(name, potential=True, dup=False, zeros=False)), "fixed-k",
                tune=[(T_CLS_GROUP, group)], coding=("offsets+values, diagonal streamed",), classes=(True, False), matrix=name + "_potential_same_order")
    add("lap2d_37x29_random_values_same_order", lambda: _same_order("lap2d_37x29", values="random", dup=False, zeros=False), "fixed-k", coding=("offsets",),
        classes=(False, True))
    add("stencil27_same_order", lambda: _same_order("stencil27", dup=False, zeros=False), "fixed-k", coding=("offsets+values",), classes=(True, True))
    add("stencil27_potential_same_order", lambda: _same_order("stencil27", potential=True, dup=False, zeros=False), "fixed-k",
        coding=("offsets+values, diagonal streamed",), classes=(True, False))
    add("lap3d_21x17x13_rows_shuffled_apart", lambda: noncanonical(stencil("lap3d_21x17x13"), seed=2, dup=False, zeros=False, every=None), "fixed-k")
    add("lap2d_37x29_split_k6", lambda: _same_order("lap2d_37x29", zeros=False), "csr-stream")
    add("lap2d_37x29_k7_repeated_offset", lambda: _same_order("lap2d_37x29"), "fixed-k", coding=("offsets+values", "offsets", "none"))
    # ---- two-phase, forced
    two = [(T_SPMV_PLAN, 2)]
    add("graph_shuffled", lambda: noncanonical(graph_20000(), seed=1, dup=False, zeros=False, every=None), "two-phase", tune=two)
    add("graph_offdiag_dup_zeros", lambda: noncanonical(graph_20000(), seed=2, offdiag=True), "two-phase", tune=two)
    add("graph_dup_zeros_anywhere", lambda: noncanonical(graph_20000(), seed=3), "two-phase", tune=two)
    add("graph_no_diagonal_every_fifth", lambda: noncanonical(without_diagonal(graph_20000(), np.arange(20000) % 5 != 4), seed=4, dup=False, zeros=False, every=None),
        "two-phase", tune=two)
    add("graph_diagonal_only_a_zero", lambda: zero_diagonal_only(graph_20000(), seed=5), "two-phase", tune=two)
    add("graph_offdiag_dup_zeros_pb256", lambda: noncanonical(graph_20000(), seed=2, offdiag=True), "two-phase", tune=two + [(T_PB_ENTRIES, 256)],
        matrix="graph_offdiag_dup_zeros")
    return cases
