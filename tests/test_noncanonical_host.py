"""Non-canonical CSR on the host: the builder of tests/noncanonical_reference.py, its references and the two wrong products they must
catch; the condition that makes the device's bit-equality a test of the summation ORDER, on every matrix of a bit-exact device case;
the caller's arrays after every public function on its NumPy backend; the Jacobi diagonal; ``_pack_matrix``."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla
from bicgstab_reference import random_csr, worst
from noncanonical_reference import (ORDER_EXEMPT, ORDER_SHARE, PAD_ENTRIES, PAD_VALUE, _canonical, arrays_of, class_count, diagonal_position,
                                    duplicate_rows, first_and_last_only, noncanonical, noncanonical_hermitian, one_value_per_column,
                                    order_sensitive_share, product_cases, reshuffled, sorted_order, stencil, stored_product, stored_sum_float64,
                                    sym_random, trimmed, untouched, x_of)
from test_svds_host import host_svds

import lanczos_amd
from lanczos_amd._solver import _pack_matrix
from lanczos_amd.bicgstab import NumpyBicgstabBackend
from lanczos_amd.cg import NumpyCgBackend
from lanczos_amd.eigs import NumpyCplxBackend, _eigs
from lanczos_amd.eigsh import NumpyBackend, trl
from lanczos_amd.expm import NumpyExpmBackend
from lanczos_amd.gmres import NumpyGmresBackend
from lanczos_amd.lsmr import NumpyLsmrBackend
from lanczos_amd.minres import NumpyMinresBackend
from lanczos_amd.svds import _pack


def _err(a, b):
    return np.abs(np.asarray(a - b, dtype=np.float64))


def spd(n):
    """symmetric, strictly diagonally dominant with a positive diagonal: what ``cg`` needs"""
    S = sym_random(n)
    S = S - sp.diags(S.diagonal())
    return (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr()


def hermitian(n):
    rng = np.random.default_rng(n)
    S = sp.random(n, n, density=3.0 / n, random_state=rng, data_rvs=rng.standard_normal).tocsr()
    T = sp.random(n, n, density=3.0 / n, random_state=rng, data_rvs=rng.standard_normal).tocsr()
    G = S + 1j * T
    return (G + G.getH() + sp.diags(rng.standard_normal(n))).tocsr()


# ---------------------------------------------------------------- the builder
def test_builder():
    A = sym_random(257)
    A = (A.tolil())
    A[100, :] = 0.0
    A[:, 100] = 0.0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    C = _canonical(A)
    assert C.indptr[101] == C.indptr[100]  # an empty row
    B = noncanonical(A, seed=1)
    assert B.indices.dtype == np.int32 and not B.has_sorted_indices and not B.has_canonical_format
    lens, lens0 = np.diff(B.indptr), np.diff(C.indptr)
    spared = np.arange(257) % 4 == 3
    assert np.array_equal(lens[spared | (lens0 == 0)], lens0[spared | (lens0 == 0)]) and lens[100] == 0
    assert np.array_equal(lens[~spared & (lens0 > 0)], lens0[~spared & (lens0 > 0)] + 2)
    for r in np.flatnonzero(spared):  # those rows stay canonical, bit for bit
        a, b = B.indptr[r], B.indptr[r + 1]
        assert np.array_equal(B.indices[a:b], C.indices[C.indptr[r]:C.indptr[r + 1]]) and np.array_equal(B.data[a:b], C.data[C.indptr[r]:C.indptr[r + 1]])
    assert (B.data == 0.0).sum() == (~spared & (lens0 > 0)).sum()  # one explicit zero in each of the others
    assert duplicate_rows(B, np.ones(257)).sum() >= (~spared & (lens0 > 0)).sum()
    assert abs(_canonical(B) - C).max() <= 4 * np.finfo(float).eps * abs(C).max()  # the same matrix, up to the rounding of t + (v - t)
    assert np.array_equal(noncanonical(A, seed=1).data, B.data) and not np.array_equal(noncanonical(A, seed=2).indices, B.indices)
    only_shuffled = noncanonical(A, seed=1, dup=False, zeros=False)
    assert only_shuffled.nnz == C.nnz and abs(_canonical(only_shuffled) - C).max() == 0.0 and not only_shuffled.has_sorted_indices


def test_builder_variants():
    L = stencil("lap2d_37x29")
    B = noncanonical(L, seed=0, dup=False, zeros=False, same_order=True)
    assert np.all(np.diff(B.indptr) == 5) and class_count(B, True) == 9 and abs(_canonical(B) - L).max() == 0.0
    assert np.mean(diagonal_position(B) != diagonal_position(_canonical(L))) > 0.5
    assert class_count(noncanonical(stencil("lap3d_21x17x13"), seed=2, dup=False, zeros=False, every=None), False) > 256  # rows shuffled one by one
    K7 = noncanonical(L, seed=0, same_order=True)
    assert np.all(np.diff(K7.indptr) == 7) and class_count(K7, True) == 9 and np.all(duplicate_rows(K7, np.ones(L.shape[0])))
    off = K7.indices.reshape(-1, 7) - np.arange(L.shape[0])[:, None]
    assert all(len(set(row)) < 7 for row in off[:50])  # a class with a repeated offset
    assert np.all(np.diff(noncanonical(L, seed=0, zeros=False, same_order=True).indptr) == 6)
    # padded: SciPy takes arrays longer than indptr[-1] and never reads the tail
    A = sym_random(257)
    P = noncanonical(A, seed=258, padded=True)
    assert len(P.data) == len(P.indices) == P.indptr[-1] + PAD_ENTRIES == P.nnz + PAD_ENTRIES and np.all(P.data[P.nnz:] == PAD_VALUE)
    x = x_of(P)
    assert np.abs(P @ x).max() < 1e3 and np.array_equal(P @ x, trimmed(P) @ x) and np.array_equal(stored_sum_float64(P, x), P @ x)
    assert np.array_equal(np.asarray(stored_product(P, x)[0], dtype=np.float64), np.asarray(stored_product(trimmed(P), x)[0], dtype=np.float64))
    # the complex twin: Hermitian as a matrix, not entry by entry
    H = hermitian(257)
    Z = noncanonical_hermitian(H, seed=3)
    assert Z.dtype == np.complex128 and not Z.has_canonical_format and abs(_canonical(Z) - H).max() == 0.0
    assert abs(Z - Z.getH()).max() == 0.0  # (SciPy sums the duplicates here)
    coo = Z.tocoo()
    stored = dict()
    for r, c, v in zip(coo.row, coo.col, coo.data):
        stored.setdefault((r, c), []).append(v)
    assert any(sorted(map(complex, stored[(c, r)]), key=abs) != sorted((complex(v).conjugate() for v in vs), key=abs) for (r, c), vs in stored.items())
    R = reshuffled(Z, 4)
    assert np.array_equal(np.sort(R.indices), np.sort(Z.indices)) and abs(_canonical(R) - _canonical(Z)).max() == 0.0 and not np.array_equal(R.indices, Z.indices)
    F = first_and_last_only()
    C = _canonical(sym_random(257))
    assert np.array_equal(F.indices[F.indptr[1]:F.indptr[256]], C.indices[C.indptr[1]:C.indptr[256]])


# ---------------------------------------------------------------- the references and the two wrong products
@pytest.mark.parametrize("n", [5, 257, 1000, 3000])
def test_references_and_mutants(n):
    """``stored_sum_float64`` is SciPy's ``B @ x`` bit for bit and lies within ``stored_product``'s bound of the longdouble sum;
    ``sorted_order`` fails the first check in at least a quarter of the rows, ``one_value_per_column`` the second in every row that holds
    a duplicate of a non-zero entry where x is non-zero - and in no other row"""
    B = noncanonical(sym_random(n), seed=n)
    x = x_of(B)
    y = stored_sum_float64(B, x)
    assert np.array_equal(y, B @ x)  # SciPy adds the stored entries one after the other
    exact, bound = stored_product(B, x)
    assert worst(_err(y, exact), bound) <= 1.0
    share = order_sensitive_share(B, x)
    wrong = sorted_order(B, x)
    print(f"n = {n}: sorted_order differs in {100 * share:.0f} % of the rows; its error / bound {worst(_err(wrong, exact), bound):.2e}")
    assert share >= ORDER_SHARE and not np.array_equal(wrong, B @ x)
    assert worst(_err(wrong, exact), bound) <= 1.0  # ... and only bit-equality can see it: the same entries, another order
    assert np.array_equal(sorted_order(_canonical(B), x), _canonical(B) @ x)  # (on sorted rows it is the stored order)
    wrong = one_value_per_column(B, x)
    dup = duplicate_rows(B, x)
    err = _err(wrong, exact)
    assert dup.sum() >= (3 * n) // 4 - 1 and np.all(err[dup] > bound[dup]) and np.all(err[~dup] <= bound[~dup])
    assert worst(err, bound) > 1.0


def test_stored_product_of_empty_rows_and_complex_input():
    B = sp.csr_matrix((np.array([1.0, 2.0, 2.0, 5.0, 0.0, -2.0]), np.array([0, 3, 1, 3, 1, 1], dtype=np.int32), np.array([0, 1, 2, 2, 6, 6, 6], dtype=np.int32)), shape=(6, 6))
    x = np.arange(1.0, 7.0)
    exact, bound = stored_product(B, x)
    assert np.array_equal(np.asarray(exact, dtype=np.float64), [1.0, 8.0, 0.0, 20.0, 0.0, 0.0]) and np.all(bound[[2, 4, 5]] == 0.0) and bound[3] > bound[0] > 0
    assert np.array_equal(stored_sum_float64(B, x), B @ x)
    E = sp.csr_matrix((4, 4))
    assert not np.any(stored_product(E, np.ones(4))[0]) and not np.any(stored_product(E, np.ones(4))[1]) and not np.any(stored_sum_float64(E, np.ones(4)))
    Z = noncanonical_hermitian(hermitian(257), seed=3)
    z = x_of(Z) + 1j * x_of(Z, 2)
    exact, bound = stored_product(Z, z)
    assert exact.dtype == np.clongdouble and worst(np.abs(np.asarray(Z @ z - exact, dtype=np.complex128)), bound) <= 1.0


def test_the_references_leave_the_matrix_as_stored():
    """SciPy's ``abs(B)`` sums B's duplicates in place, through any wrapper that shares its arrays; no reference here may do that"""
    import hermitian_reference as hr
    from noncanonical_reference import stored_abs

    B, Z = noncanonical(sym_random(257), seed=257), noncanonical_hermitian(hermitian(257), seed=3)
    x = x_of(B)
    for M in (B, Z):
        before = arrays_of(M)
        stored_product(M, x), hr.matvec(M, x), hr.product_bound(M, x), stored_abs(M), duplicate_rows(M, x), _canonical(M), trimmed(M), reshuffled(M, 1)
        if M is B:
            stored_sum_float64(M, x), sorted_order(M, x), one_value_per_column(M, x), order_sensitive_share(M, x)
        assert untouched(M, before)
    exact, bound = stored_product(B, x)
    assert np.allclose(np.asarray(hr.abs_matvec(B, x)[0], dtype=np.float64), stored_abs(B) @ np.abs(x), rtol=1e-15, atol=0.0)
    big, small = stored_abs(B) @ np.abs(x), abs(B.copy()) @ np.abs(x)  # entry by entry as stored: never less than |summed entries| (to rounding)
    assert np.all(big >= small * (1.0 - 64 * np.finfo(float).eps)) and np.any(big > 1.01 * small)


def test_every_bit_exact_device_case_is_order_sensitive():
    """tests/test_gpu_noncanonical.py asserts SciPy's bits: that tests the ORDER of the sums only if another order gives other bits.  On
    every matrix and x of those cases the column-order sum changes at least a quarter of the rows (but in the three edge cases that cannot
    by construction), and the wrong-duplicates product leaves the bound in every row that can show it"""
    seen = set()
    for name, case in product_cases().items():
        B = case["build"]()
        if id(B) in seen:
            continue
        seen.add(id(B))
        x = x_of(B)
        assert np.array_equal(stored_sum_float64(B, x), B @ x), name
        share = order_sensitive_share(B, x)
        print(f"{name:44s} n = {B.shape[0]:6d}: sorted_order differs in {100 * share:5.1f} % of the rows")
        assert share >= ORDER_SHARE or name in ORDER_EXEMPT, name
        dup = duplicate_rows(B, x)
        if dup.any():
            exact, bound = stored_product(B, x)
            assert np.all(_err(one_value_per_column(B, x), exact)[dup] > bound[dup]), name
    assert set(ORDER_EXEMPT) <= set(product_cases())


# ---------------------------------------------------------------- nothing sorts or sums the caller's arrays in place
def _calls():
    S, N, Z = noncanonical(spd(257), seed=11), noncanonical(random_csr(257), seed=12), noncanonical_hermitian(hermitian(257), seed=13)
    R = noncanonical(sp.random(300, 120, density=0.05, random_state=np.random.default_rng(5), data_rvs=np.random.default_rng(6).standard_normal), seed=14)
    b = np.random.default_rng(1).standard_normal(257)
    return {
        "eigsh": (S, lambda: trl(NumpyBackend(S), 257, 3, "LA")),
        "eigsh_complex": (Z, lambda: trl(NumpyBackend(Z), 257, 3, "LA")),
        "eigs": (N, lambda: _eigs(NumpyCplxBackend(N), 257, 3, "LM", None, None, 0, None, True, None)),
        "expm_multiply": (S, lambda: lanczos_amd.expm_multiply(S, b, a=-0.01, _backend=NumpyExpmBackend(S, False))),
        "expm_multiply_complex": (Z, lambda: lanczos_amd.expm_multiply(Z, b, a=-0.01j, _backend=NumpyExpmBackend(Z, True))),
        "minres": (S, lambda: lanczos_amd.minres(S, b, rtol=1e-8, _backend=NumpyMinresBackend(S))),
        "cg": (S, lambda: lanczos_amd.cg(S, b, rtol=1e-8, M="jacobi", _backend=NumpyCgBackend(S))),
        "bicgstab": (N, lambda: lanczos_amd.bicgstab(N, b, rtol=1e-8, _backend=NumpyBicgstabBackend(N))),
        "gmres": (N, lambda: lanczos_amd.gmres(N, b, rtol=1e-8, _backend=NumpyGmresBackend(N))),
        "svds": (R, lambda: host_svds(R, k=3)),
        "svds_wide": (R, lambda: host_svds(sp.csr_matrix((R.data, R.indices, R.indptr), shape=R.shape).T, k=3)),
        "lsmr": (R, lambda: lanczos_amd.lsmr(R, np.ones(300), _backend=NumpyLsmrBackend(R))),
        "svds._pack": (R, lambda: _pack(R)),
        "_pack_matrix": (S, lambda: _pack_matrix(S)),
    }


@pytest.mark.parametrize("name", list(_calls()))
def test_callers_arrays_untouched(name):
    B, call = _calls()[name]
    before = arrays_of(B)
    assert not B.has_sorted_indices
    out = call()
    assert out is not None
    assert untouched(B, before), name


def test_pack_copies_before_it_sorts():
    """``svds`` / ``lsmr`` canonicalise (``svds._pack``): a copy, both for the tall matrix and for the wide one, whose transpose shares the
    caller's arrays"""
    R = noncanonical(sp.random(300, 120, density=0.05, random_state=np.random.default_rng(5)), seed=14)
    for A in (R, sp.csr_matrix((R.data, R.indices, R.indptr), shape=R.shape).T):
        before = arrays_of(R)
        Aop, AopT, transposed = _pack(A)
        assert untouched(R, before) and Aop.has_canonical_format and Aop.shape == (300, 120)
        assert not np.shares_memory(Aop.data, R.data) and not np.shares_memory(Aop.indices, R.indices)
        assert abs(Aop - _canonical(R)).max() == 0.0 and abs(AopT - Aop.T).max() == 0.0


# ---------------------------------------------------------------- Jacobi, formats
def test_jacobi_uses_the_summed_diagonal_and_the_formats_agree():
    from lanczos_amd.cg import preconditioner_diagonal

    A = spd(257)
    B = noncanonical(A, seed=21)
    split = [r for r in range(257) if (B.indices[B.indptr[r]:B.indptr[r + 1]] == r).sum() > 1]
    assert len(split) >= 10  # rows that store their diagonal in two (or three) pieces
    d = preconditioner_diagonal(B, "jacobi", 257)
    summed = np.array([B.data[B.indptr[r]:B.indptr[r + 1]][B.indices[B.indptr[r]:B.indptr[r + 1]] == r].sum() for r in range(257)])
    assert np.allclose(d, 1.0 / summed, rtol=4 * np.finfo(float).eps, atol=0.0) and np.allclose(d, 1.0 / A.diagonal(), rtol=1e-14, atol=0.0)
    b = np.random.default_rng(2).standard_normal(257)
    exact = np.linalg.solve(_canonical(B).toarray(), b)
    coo = trimmed(B).tocoo()  # COO with duplicates, CSC, CSR: the same matrix
    assert coo.nnz == B.nnz
    xs = {}
    for fmt, M in (("csr", B), ("coo", coo), ("csc", B.tocsc())):
        info = {}
        x, code = lanczos_amd.cg(M, b, rtol=1e-10, M="jacobi", info=info, _backend=NumpyCgBackend(M))
        assert code == 0 and info["preconditioner"] == "diagonal"
        assert np.linalg.norm(B @ x - b) <= 1e-10 * np.linalg.norm(b) * 1.001
        xs[fmt] = x
    # tests/test_cg_host.py's bar for two solutions of one system at rtol: both within rtol cond(A) |x| of the exact one
    cond = np.linalg.cond(_canonical(B).toarray())
    for fmt, x in xs.items():
        assert np.linalg.norm(x - exact) <= 1e-10 * cond * np.linalg.norm(exact), fmt
    ref, code = sla.cg(B, b, rtol=1e-10, M=sp.diags(d))
    assert code == 0 and np.linalg.norm(xs["csr"] - ref) <= 2e-10 * cond * np.linalg.norm(exact)


# ---------------------------------------------------------------- _pack_matrix
def test_pack_matrix_keeps_the_stored_order():
    B = noncanonical(sym_random(257), seed=31)
    kind, rowptr, colidx, vals = _pack_matrix(B)
    assert kind == "csr" and np.shares_memory(rowptr, B.indptr) and np.shares_memory(colidx, B.indices) and np.shares_memory(vals, B.data)
    assert np.array_equal(colidx, B.indices) and np.array_equal(vals, B.data)
    # int64 indices: converted, in stored order
    B64 = sp.csr_matrix((B.data, B.indices, B.indptr), shape=B.shape)
    B64.indices, B64.indptr = B64.indices.astype(np.int64), B64.indptr.astype(np.int64)  # (the constructor would narrow them)
    assert B64.indices.dtype == np.int64
    before = arrays_of(B64)
    kind, rowptr, colidx, vals = _pack_matrix(B64)
    assert rowptr.dtype == colidx.dtype == np.int32 and np.array_equal(colidx, B.indices) and np.array_equal(rowptr, B.indptr) and np.shares_memory(vals, B64.data)
    assert untouched(B64, before)
    # padded: the arrays as they are; the matrix ends at rowptr[-1]
    P = noncanonical(sym_random(257), seed=258, padded=True)
    kind, rowptr, colidx, vals = _pack_matrix(P)
    assert np.shares_memory(vals, P.data) and len(vals) == rowptr[-1] + PAD_ENTRIES and np.array_equal(colidx[:rowptr[-1]], trimmed(P).indices)
    # another format: converted to CSR by SciPy (which sums a COO matrix's duplicates on the way): the same matrix, within the bound
    coo = trimmed(B).tocoo()
    before = (coo.row.copy(), coo.col.copy(), coo.data.copy())
    kind, rowptr, colidx, vals = _pack_matrix(coo)
    x = x_of(B)
    exact, bound = stored_product(B, x)
    assert worst(_err(sp.csr_matrix((vals, colidx, rowptr), shape=B.shape) @ x, exact), bound) <= 1.0
    assert all(np.array_equal(a, b) for a, b in zip(before, (coo.row, coo.col, coo.data)))
