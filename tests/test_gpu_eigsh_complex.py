"""eigsh on complex Hermitian matrices, on the device: the complex product kernels against clongdouble, one ``lz_ztrl_extend`` step on
rows set from the host under the reference's derived bounds (tests/hermitian_reference.py; the cases: tests/test_eigsh_complex_host.py),
the restart against NumPy, and ``eigsh`` end to end at the bars of tests/test_gpu_trl.py - eigenvalues within ``1e-10 |A|`` of
``numpy.linalg.eigvalsh``, residuals ``<= 1e-9 |A|``, ``|Y^H Y - I| <= 1e-12``."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from hermitian_reference import matvec, product_bound, worst
from scipy.sparse.linalg import ArpackNoConvergence
from test_eigsh_complex_host import (CONV_CASES, LONG_N, PROBE_KS, PROBE_M, STEP_CASES, Case, case_id, check_pairs, check_probed_rows,
                                     conv_matrix, probe_reference, probe_state, step_reference)

from lanczos_amd import _capi, eigsh, synthetic
from lanczos_amd.eigsh import NumpyBackend

pytestmark = pytest.mark.gpu


def _handle(A, flags=0):
    h = _capi.Handle(0)
    h.set_options(flags)
    if sp.issparse(A):
        h.set_csr_cplx(A.shape[0], A.indptr, A.indices, A.data)
    else:
        h.set_dense_cplx(A)
    return h


# ---------------------------------------------------------------- a. the product kernels alone
def _hermitian(n, rng, per_row=3):
    r = np.repeat(np.arange(n), per_row)
    B = sp.csr_matrix((rng.standard_normal(per_row * n) + 1j * rng.standard_normal(per_row * n), (r, rng.integers(0, n, per_row * n))), shape=(n, n))
    return B + B.conj().T


@functools.lru_cache(maxsize=None)
def product_matrix(name):
    rng = np.random.default_rng(41)
    if name == "hofstadter":
        A = synthetic.hofstadter(24, 17, 1 / 3)
    elif name == "ragged1000":  # about six entries per row, one row and column of 300, five empty rows
        n = 1000
        long_row = sp.csr_matrix((rng.standard_normal(300) + 1j * rng.standard_normal(300), (np.full(300, 7), rng.choice(n, 300, replace=False))), shape=(n, n))
        A = _hermitian(n, rng) + long_row + long_row.conj().T
        keep = np.ones(n)
        keep[[0, 123, 500, 501, 999]] = 0.0
        A = (sp.diags(keep) @ A @ sp.diags(keep)).tocsr()
        A.eliminate_zeros()
        counts = np.diff(A.indptr)
        assert counts[7] >= 300 and (counts == 0).sum() == 5 and 4 < counts.mean() < 8
    elif name == "band70001":  # several blocks of every launch, n odd
        n = 70001
        offs = (1, 2, 5, 40)
        up = [rng.standard_normal(n - o) + 1j * rng.standard_normal(n - o) for o in offs]
        A = sp.diags(up, offs) + sp.diags([u.conj() for u in up], [-o for o in offs]) + sp.diags(rng.standard_normal(n) + 0j)
    else:
        assert name == "n5"
        G = rng.standard_normal((5, 5)) + 1j * rng.standard_normal((5, 5))
        A = sp.csr_matrix(G + G.conj().T)
    A = sp.csr_matrix(A, dtype=np.complex128)
    A.sort_indices()
    assert abs(A - A.conj().T).max() == 0.0
    return A


def _check_product(h, A, label):
    n = A.shape[0]
    rng = np.random.default_rng(n)
    for trial in range(2):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        y = h.zspmv(x)
        ref = matvec(A, x)
        err = np.abs(np.asarray(y - ref, dtype=np.complex128))
        bound = product_bound(A, x)
        print(f"{label:16s} trial {trial}: worst error / bound {worst(err, bound):.2e}")
        assert np.all(np.isfinite(y.view(np.float64)))
        assert worst(err, bound) <= 1.0


@pytest.mark.parametrize("name", ["hofstadter", "ragged1000", "band70001", "n5"])
def test_csr_product_against_clongdouble(name):
    A = product_matrix(name)
    h = _handle(A)
    _check_product(h, A, name)
    if name == "ragged1000":  # an empty row gives an exact zero
        y = h.zspmv(np.ones(1000) + 1j)
        assert np.all(y[[0, 123, 500, 501, 999]] == 0.0)
    h.close()


@pytest.mark.parametrize("n", [5, 64, 257, 1000])
def test_dense_product_against_clongdouble(n):
    rng = np.random.default_rng(n + 7)
    G = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    A = np.ascontiguousarray(G + G.conj().T)
    h = _handle(A)
    _check_product(h, A, f"dense {n}")
    h.close()


# ---------------------------------------------------------------- b. one extension step against the reference
def one_step(h, case, rows, ref, label):
    """rows 0 .. nb - 1 set from the host, step nb - 1 on the device: everything it returns under the reference's bounds"""
    nb = case.nb
    m = max(nb, 2)
    h.ztrl_set_rows(0, rows)
    proj, beta = h.ztrl_extend(nb - 1, m)
    out = h.ztrl_get_rows(0, nb + 1)
    err = {"proj": worst(np.abs(proj[nb - 1, :nb] - (ref["c1"] + ref["c2"])), ref["e_proj"]),
           "beta": worst(abs(beta[nb - 1] - ref["beta"]), ref["e_beta"]), "v": worst(np.abs(out[nb] - ref["v"]), ref["e_v"])}
    print(f"{label:36s} error / bound: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert np.all(np.isfinite(proj[nb - 1].view(np.float64))) and np.isfinite(beta[nb - 1])
    assert all(v <= 1.0 for v in err.values()), err
    assert np.array_equal(out[:nb], rows)  # the rows below are only read
    if case.kind == "orth":  # the diagonal projection <x, A x> is real: its imaginary part is roundoff only
        assert abs(proj[nb - 1, nb - 1].imag) <= ref["e_proj"][nb - 1]


@pytest.mark.parametrize("case", STEP_CASES, ids=case_id)
def test_one_step_within_the_reference_bounds(case):
    """both launch shapes of k_zdots / k_zcgs: a padded length below 524288 doubles (every n here but LONG_N) and from it on (LONG_N)"""
    assert h_pad(LONG_N) == 524288 and h_pad(LONG_N - 1) < 524288
    A, rows, ref = step_reference(case)
    h = _handle(A, _capi.FLAG_TRL_PASS2_ALWAYS if case.force else 0)
    h.ztrl_begin(max(case.nb, 2), np.ones(case.n))
    one_step(h, case, rows, ref, case_id(case))
    h.close()


def h_pad(n):
    return -(-n // 32) * 32


def test_no_second_pass_leaks_behind_a_closed_gate():
    """a step whose gate opens, then one on the same handle whose gate stays closed: the second returns pass 1's coefficients alone"""
    near, orth = Case(1000, 17, "near", False, False), Case(1000, 17, "orth", False, False)
    assert near in STEP_CASES and orth in STEP_CASES
    A, rows, ref = step_reference(near)
    assert ref["pass2"] and not step_reference(orth)[2]["pass2"]
    h = _handle(A)
    h.ztrl_begin(17, np.ones(1000))
    one_step(h, near, rows, ref, case_id(near) + " (gate open)")
    one_step(h, orth, step_reference(orth)[1], step_reference(orth)[2], case_id(orth) + " (then closed)")
    h.close()


# ---------------------------------------------------------------- c. the restart
@pytest.mark.parametrize("m,kk", [(20, 10), (41, 30), (64, 62)])
@pytest.mark.parametrize("n", [17, 1000, 4099])
def test_restart_matches_numpy(m, kk, n):
    if n < m:
        n = n + m
    h = _handle(sp.identity(n, dtype=np.complex128, format="csr"))
    h.ztrl_begin(m, np.ones(n))
    rng = np.random.default_rng(n + m)
    V = rng.standard_normal((m + 1, n)) + 1j * rng.standard_normal((m + 1, n))
    h.ztrl_set_rows(0, V)
    S = rng.standard_normal((m, kk)) + 1j * rng.standard_normal((m, kk))
    h.ztrl_restart(m, kk, S)
    out = h.ztrl_get_rows(0, m + 1)
    ref = S.T @ V[:m]
    scale = np.abs(ref).max()
    assert np.abs(out[:kk] - ref).max() <= 1e-13 * scale
    assert np.array_equal(out[kk], V[m])  # V[m] moved to V[kk], bit for bit
    assert np.array_equal(out[kk + 1:], V[kk + 1:])  # the other rows >= kk untouched
    h.close()


# ---------------------------------------------------------------- the probe
@pytest.mark.parametrize("n", [33, 1000])
def test_probe_matches_numpy(n):
    """Guards lz_orth.hip on a two-plane basis: orth_upload_x's memset of both planes of the work vector, orth_store's two CGS passes
    over rows [0, k) - row k is the self slot and is not read -, its k == 0 norm-only branch and the scale-and-store of row k's two
    planes alone; lz_ztrl_probe's bounds on k.  The bars are tests/test_gpu_svds_edges.py's (check_probed_rows)."""
    A, V, x = probe_reference(n)
    m = PROBE_M
    h = _handle(A)
    h.ztrl_begin(m, np.ones(n))
    be = NumpyBackend(A)
    for k in PROBE_KS:
        state = probe_state(V, k)
        h.ztrl_set_rows(0, state)
        be.V = state.copy()
        h.ztrl_probe(k, x)
        be.probe(k, x)
        check_probed_rows(h.ztrl_get_rows(0, m + 1), state, be.V[k], k, f"n {n} k {k}")
    h.ztrl_set_rows(0, V)
    for k in (-1, m + 1):
        with pytest.raises(_capi.LanczosHipError):
            h.ztrl_probe(k, x)
    assert np.array_equal(h.ztrl_get_rows(0, m + 1), V)  # a refused call changes nothing
    if n == 33:  # the padded length is 64: the unpadded getter cannot see the padding of w or of row 5, the steps that stream it can
        assert h_pad(n) == 64
        be.V = V.copy()
        h.ztrl_probe(5, x)
        be.probe(5, x)
        proj, beta = h.ztrl_extend(5, m)
        ref_proj, ref_beta = be.extend(5, m)
        out = h.ztrl_get_rows(0, m + 1)
        assert np.isfinite(proj[5:].view(np.float64)).all() and np.isfinite(beta[5:]).all() and np.isfinite(out.view(np.float64)).all()
        assert np.abs(proj[5:] - ref_proj[5:]).max() <= 1e-10 and np.abs(beta[5:] - ref_beta[5:]).max() <= 1e-10
        assert np.linalg.norm(out - be.V, axis=1).max() <= 1e-10
    h.close()


# ---------------------------------------------------------------- d. eigsh end to end
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c.name)
def test_eigsh_end_to_end(case):
    A, D, ev = conv_matrix(case.matrix)
    anorm = np.abs(ev).max()
    info = {}
    theta, Y = eigsh(A, k=case.k, which=case.which, ncv=case.ncv, info=info)
    print({k: v for k, v in info.items() if k != "residuals"})
    check_pairs(case, theta, Y, case.name)
    host_res = np.linalg.norm(D @ Y - Y * theta, axis=0)
    assert np.abs(info["residuals"] - host_res).max() <= 1e-12 * anorm
    assert np.array_equal(eigsh(A, k=case.k, which=case.which, ncv=case.ncv, return_eigenvectors=False), theta)


def test_real_part_alone_is_another_spectrum():
    """what the parent commit returned for this input: the spectrum of Re(A)"""
    A, D, ev = conv_matrix("hof")
    theta = eigsh(A, k=6, which="SA", return_eigenvectors=False)
    wrong = np.linalg.eigvalsh(D.real)[:6]
    assert np.abs(theta - ev[:6]).max() <= 1e-10 * np.abs(ev).max() < 1e-3 < np.abs(wrong - ev[:6]).max()


def test_same_handle_same_v0_same_bits_and_the_other_arguments():
    A, D, ev = conv_matrix("hof")
    n = A.shape[0]
    v0 = np.random.default_rng(8).standard_normal(n) + 1j * np.random.default_rng(9).standard_normal(n)
    h = _capi.Handle(0)
    t1, Y1 = eigsh(A, k=6, which="SA", v0=v0, handle=h)
    t2, Y2 = eigsh(A, k=6, which="SA", v0=v0, handle=h)
    assert np.array_equal(t1, t2) and np.array_equal(Y1, Y2)
    t3 = eigsh(A, k=6, which="SA", v0=v0.real, handle=h, return_eigenvectors=False)  # a real v0 is taken too
    assert np.abs(t3 - ev[:6]).max() <= 1e-10 * np.abs(ev).max()
    t4 = eigsh(A.astype(np.complex64).tocoo(), k=6, which="SA", handle=h, return_eigenvectors=False)  # complex64, another format
    ev32 = np.linalg.eigvalsh(A.astype(np.complex64).astype(np.complex128).toarray())
    assert np.abs(t4 - ev32[:6]).max() <= 1e-10 * np.abs(ev).max()
    h.close()


def test_maxiter_one_raises_with_consistent_shapes():
    A, D, ev = conv_matrix("hof")
    with pytest.raises(ArpackNoConvergence) as e:
        eigsh(A, k=6, which="SA", maxiter=1)
    lam, vecs = e.value.eigenvalues, e.value.eigenvectors
    assert vecs.dtype == np.complex128 and vecs.shape == (408, len(lam)) and len(lam) < 6
    if len(lam):
        assert np.linalg.norm(D @ vecs - vecs * lam, axis=0).max() <= 1e-9 * np.abs(ev).max()


def test_a_handle_takes_real_and_complex_matrices_in_turn():
    A, D, ev = conv_matrix("hof")
    R = synthetic.laplacian_2d_5pt(24, 17).to_scipy()
    evR = np.linalg.eigvalsh(R.toarray())
    h = _capi.Handle(0)
    for _ in range(2):
        th = eigsh(A, k=4, which="SA", handle=h, return_eigenvectors=False)
        assert np.abs(th - ev[:4]).max() <= 1e-10 * np.abs(ev).max()
        for call in (lambda: h.trl_begin(20, np.ones(408)), lambda: h.spmv_host(np.ones(408)), lambda: h.trl_extend(0, 20)):
            with pytest.raises(_capi.LanczosHipError) as e:  # a complex matrix is set: the real entry points have no matrix
                call()
            assert e.value.status == -4
        th = eigsh(R, k=4, which="LA", handle=h, return_eigenvectors=False)
        assert np.abs(th - evR[-4:]).max() <= 1e-10 * np.abs(evR).max()
        for call in (lambda: h.ztrl_begin(20, np.ones(408)), lambda: h.zspmv(np.ones(408)), lambda: h.ztrl_extend(0, 20)):
            with pytest.raises(_capi.LanczosHipError) as e:  # ... and the other way round
                call()
            assert e.value.status == -4
    h.close()


def test_state_checks_of_the_complex_basis():
    A, _, _ = conv_matrix("hof")
    h = _handle(A)
    with pytest.raises(_capi.LanczosHipError) as e:  # no basis yet
        h.ztrl_extend(0, 20)
    assert e.value.status == -4
    with pytest.raises(_capi.LanczosHipError) as e:  # the complex cap
        h.ztrl_begin(65, np.ones(408))
    assert e.value.status == -1
    h.ztrl_begin(20, np.ones(408))
    B, _, _ = conv_matrix("hofP")
    h.set_csr_cplx(B.shape[0], B.indptr, B.indices, B.data)  # another row length
    with pytest.raises(_capi.LanczosHipError) as e:
        h.ztrl_extend(0, 20)
    assert e.value.status == -4 and "changed" in str(e.value)
    h.close()
    for flag in (_capi.FLAG_REORTH_PARTIAL, _capi.FLAG_ONE_REDUCE):
        h = _handle(A, flag)
        with pytest.raises(_capi.LanczosHipError) as e:
            h.ztrl_begin(20, np.ones(408))
        assert e.value.status == -4
        h.close()


def test_the_fixed_n_classes_refuse_complex_input():
    import warnings

    import lanczos_amd

    A, D, _ = conv_matrix("hofP")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a ComplexWarning would mean that something was converted after all
        for cls in (lanczos_amd.Lanczos, lanczos_amd.IrrLanczos):
            for H in (A, np.array(D)):
                s = cls(H)
                s.verbose = False
                with pytest.raises(NotImplementedError, match="complex input: use lanczos_amd.eigsh"):
                    s.execute_Lanczos(10)


def test_dense_input_row_major_or_not():
    A, D, ev = conv_matrix("dense96")
    F = np.asfortranarray(A)
    view = F[::1, :]
    assert not view.flags.c_contiguous
    t0 = eigsh(A, k=4, which="SA", return_eigenvectors=False)
    t1 = eigsh(view, k=4, which="SA", return_eigenvectors=False)
    assert np.array_equal(t0, t1)
    assert np.abs(t0 - ev[:4]).max() <= 1e-10 * np.abs(ev).max()
