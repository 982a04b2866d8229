"""Dense input of lanczos_amd.svds on the host (no GPU): what ``_pack`` keeps dense and without a copy, the C ABI of the dense operator,
and the end-to-end cases of tests/test_gpu_svds_dense.py through ``NumpyGKBackend`` - the check that the cases themselves are sound.

Bars: those of tests/test_svds_host.py (values 1e-10 sigma_max, residuals 1e-9 sigma_max, orthonormality 1e-12)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse
from test_svds_host import check_triplets, host_svds

import lanczos_amd
from lanczos_amd import _capi
from lanczos_amd.svds import _pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (shape, k, which): Gaussian entries, np.random.default_rng(11); every case runs C- and F-ordered (CASES) but the SM one
_TABLE = [((2000, 33), 4, "LM"), ((33, 2000), 4, "LM"), ((700, 257), 4, "LM"), ((257, 700), 4, "LM"), ((129, 128), 4, "LM"),
          ((600, 65), 4, "LM"), ((65, 4100), 4, "LM"), ((4100, 130), 4, "LM"), ((1030, 3), 1, "LM"), ((3, 5000), 1, "LM")]
CASES = [(shape, order, k, which) for shape, k, which in _TABLE for order in "CF"] + [((900, 40), "C", 3, "SM")]


def case_id(case):
    shape, order, k, which = case
    return f"{shape[0]}x{shape[1]}-{order}-k{k}-{which}"


_matrices, _host_runs = {}, {}


def case_matrix(shape, order="C"):
    """the case's matrix in the given memory order (shared: never written to)"""
    if (shape, order) not in _matrices:
        A = np.random.default_rng(11).standard_normal(shape)
        A = np.asfortranarray(A) if order == "F" else A
        A.setflags(write=False)
        _matrices[shape, order] = A
    return _matrices[shape, order]


def host_run(case):
    """(u, s, vh, info) of the host loop on the case, computed once"""
    if case not in _host_runs:
        shape, order, k, which = case
        info = {}
        u, s, vh = host_svds(case_matrix(shape, order), k=k, which=which, info=info)
        _host_runs[case] = (u, s, vh, info)
    return _host_runs[case]


@pytest.mark.parametrize("shape", [(50, 20), (20, 50), (30, 30)])
def test_pack_keeps_contiguous_dense_input_as_views(shape):
    A = np.random.default_rng(1).standard_normal(shape)
    tall = shape[0] >= shape[1]
    for X in (A, np.asfortranarray(A)):
        Aop, AopT, transposed = _pack(X)
        assert isinstance(Aop, np.ndarray) and isinstance(AopT, np.ndarray)
        assert transposed == (not tall)
        assert Aop.shape == ((shape[0], shape[1]) if tall else (shape[1], shape[0])) and AopT.shape == Aop.shape[::-1]
        assert np.shares_memory(Aop, X) and np.shares_memory(AopT, X)  # no copy
        assert Aop.flags.c_contiguous or AopT.flags.c_contiguous
        assert np.array_equal(Aop, X if tall else X.T) and np.array_equal(AopT, Aop.T)


def test_pack_copies_other_layouts_and_dtypes_once():
    rng = np.random.default_rng(2)
    wide = rng.standard_normal((60, 50))
    sliced = wide[::2, 3:23]  # (30, 20): neither C- nor F-contiguous
    Aop, AopT, transposed = _pack(sliced)
    assert isinstance(Aop, np.ndarray) and isinstance(AopT, np.ndarray) and not transposed
    assert Aop.dtype == np.float64 and Aop.flags.c_contiguous and not np.shares_memory(Aop, wide)
    assert np.array_equal(Aop, sliced) and np.array_equal(AopT, sliced.T)
    f32 = rng.standard_normal((20, 30)).astype(np.float32)
    Aop, AopT, transposed = _pack(f32)
    assert isinstance(Aop, np.ndarray) and isinstance(AopT, np.ndarray) and transposed
    assert Aop.dtype == np.float64 and Aop.shape == (30, 20) and np.array_equal(Aop, f32.T.astype(np.float64))
    assert AopT.flags.c_contiguous  # the one copy is the array as the caller holds it


def test_pack_density_rule():
    rng = np.random.default_rng(3)

    def with_density(d, shape=(40, 30)):
        A = rng.standard_normal(shape)
        A[rng.random(shape) >= d] = 0.0
        return A

    Aop, AopT, _ = _pack(with_density(0.2))
    assert scipy.sparse.issparse(Aop) and scipy.sparse.issparse(AopT) and Aop.format == "csr"
    Aop, AopT, _ = _pack(with_density(0.9))
    assert isinstance(Aop, np.ndarray)
    # the edge: 12 nnz < 8 size is CSR, 12 nnz == 8 size is dense
    A = np.zeros((6, 5))
    A.ravel()[:20] = 1.0  # 12 * 20 == 8 * 30
    assert isinstance(_pack(A)[0], np.ndarray)
    A.ravel()[19] = 0.0  # 12 * 19 < 8 * 30
    Aop, AopT, _ = _pack(A)
    assert scipy.sparse.issparse(Aop) and Aop.nnz == 19 and np.array_equal(Aop.toarray(), A)
    assert scipy.sparse.issparse(_pack(np.zeros((6, 5)))[0])  # no entries at all
    S = scipy.sparse.random(30, 20, density=0.9, random_state=4, format="coo")
    assert scipy.sparse.issparse(_pack(S)[0])  # sparse input stays sparse whatever its density


def test_header_declares_and_library_exports_the_dense_operator():
    text = open(os.path.join(ROOT, "include", "lanczos_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = lanczos_amd.load_library()
    for name in ("lz_gk_set_dense", "lz_gk_plan"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/lanczos_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.SIGNATURES
    assert re.search(r"lz_gk_set_dense\s*\(\s*lz_handle h,\s*int64_t p,\s*int64_t q,\s*const double\*\s*S,\s*int64_t ld_host,\s*int stored_transposed\s*\)", text)
    assert re.search(r"lz_gk_plan\s*\(\s*lz_handle h,\s*int\*\s*out\s*\)", text)


def test_plan_and_dense_calls_refuse_a_null_handle():
    """without a handle both calls fail with LZ_ERR_ARG before anything else (there is no device here); Handle has their wrappers"""
    lib = lanczos_amd.load_library()
    out = (C.c_int * 4)(7, 7, 7, 7)
    assert lib.lz_gk_plan(None, out) == -1 and list(out) == [7, 7, 7, 7]
    S = np.ones((4, 3))
    assert lib.lz_gk_set_dense(None, 4, 3, _capi.dptr(S), 3, 0) == -1
    assert callable(_capi.Handle.gk_plan) and callable(_capi.Handle.gk_set_dense)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cases_converge_on_the_host_loop(case):
    shape, order, k, which = case
    A = case_matrix(shape, order)
    assert isinstance(_pack(A)[0], np.ndarray) and np.shares_memory(_pack(A)[0], A)
    u, s, vh, info = host_run(case)
    print(f"\n{case_id(case)}: {info['cycles']} cycles, {info['matvecs']} products")
    check_triplets(A, u, s, vh, which, k, info)
    assert info["breakdowns"] == 0
