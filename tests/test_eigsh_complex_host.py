"""eigsh on complex Hermitian matrices, without a GPU: the outer loop ``trl`` on the complex NumPy backend converges on the cases that
tests/test_gpu_eigsh_complex.py runs on the device (which imports the matrices, the cases and the bars from here), the argument rules
of the complex path, the refusal of complex input everywhere else, and - bit for bit - that a real backend still gets the loop it had.

The bars are the project's own (tests/test_gpu_trl.py): eigenvalues within ``1e-10 |A|`` of ``numpy.linalg.eigvalsh``, residuals
``<= 1e-9 |A|``, ``|Y^H Y - I| <= 1e-12``, all at the default ``maxiter``.

The cases of one extension step (``STEP_CASES``, ``step_reference``) are those of tests/test_arnoldi_step_host.py made complex: the
rows are complex, the matrix is Hermitian (``n`` rows of about six complex entries plus a real diagonal), ``orth`` keeps the gate
closed, ``near`` opens it, ``skew`` with ``force`` runs the second pass on rows that are not orthonormal.  Here they are checked for
what makes them decisive - the gate decided far from its edge, the second pass's coefficients large where it runs - and the complex
NumPy backend for lying within the clongdouble reference's bounds (tests/hermitian_reference.py).
"""
import collections
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from hermitian_reference import step, worst
from scipy.sparse.linalg import ArpackNoConvergence

from lanczos_amd import eigsh as eigsh_fn
from lanczos_amd import synthetic
from lanczos_amd._solver import _pack_matrix
from lanczos_amd.eigsh import (_EPS, _SEED, NumpyBackend, _fill, _order, _start, check_args, trl,
                               upload_complex_matrix)

# ---------------------------------------------------------------- the matrices and the convergence cases
Conv = collections.namedtuple("Conv", "name matrix which k ncv")
CONV_CASES = [Conv("hof-SA", "hof", "SA", 6, None), Conv("hof-LA", "hof", "LA", 6, None), Conv("hof-LM", "hof", "LM", 6, None),
              Conv("hof-SM", "hof", "SM", 4, 64), Conv("hofP-SA-3fold", "hofP", "SA", 6, None), Conv("dense96-SA-double", "dense96", "SA", 4, None)]


@functools.lru_cache(maxsize=None)
def conv_matrix(name):
    """``(A, dense copy, ascending eigenvalues)`` of a convergence case, computed once"""
    if name == "hof":
        A = synthetic.hofstadter(24, 17, 1 / 3, disorder=0.5)
    elif name == "hofP":
        A = synthetic.hofstadter(12, 12, 1 / 3, periodic=True)
    else:
        assert name == "dense96"
        rng = np.random.default_rng(5)
        n = 96
        Q = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0]
        d = np.sort(rng.uniform(-1, 1, n))
        d[1] = d[0]
        A = (Q * d) @ Q.conj().T
        A = np.ascontiguousarray((A + A.conj().T) / 2)
    D = A.toarray() if sp.issparse(A) else A
    assert abs(D - D.conj().T).max() == 0.0 and np.abs(D.imag).max() > 0.1
    ev = np.linalg.eigvalsh(D)
    D.setflags(write=False)
    ev.setflags(write=False)
    return A, D, ev


def check_pairs(case, theta, Y, label):
    """the bars of the module docstring on ``k`` returned pairs; returns the three figures"""
    _, D, ev = conv_matrix(case.matrix)
    anorm = np.abs(ev).max()
    ref = np.sort(ev[_order(ev, case.which)[: case.k]])
    assert theta.dtype == np.float64 and theta.shape == (case.k,) and np.all(np.diff(theta) >= 0)
    assert Y.dtype == np.complex128 and Y.shape == (D.shape[0], case.k)
    err = np.abs(theta - ref).max() / anorm
    res = np.linalg.norm(D @ Y - Y * theta, axis=0).max() / anorm
    orth = np.abs(Y.conj().T @ Y - np.eye(case.k)).max()
    print(f"{label:32s} err/|A| {err:.1e}  res/|A| {res:.1e}  |Y^H Y - I| {orth:.1e}")
    assert err <= 1e-10 and res <= 1e-9 and orth <= 1e-12, (err, res, orth)
    return err, res, orth


def test_the_cases_are_what_they_claim():
    _, _, ev = conv_matrix("hofP")
    assert ev[2] - ev[0] < 1e-12 and ev[3] - ev[2] > 1e-3  # the lowest level is three-fold
    _, _, ev = conv_matrix("dense96")
    assert ev[1] - ev[0] < 1e-14 and ev[2] - ev[1] > 1e-4
    assert conv_matrix("hof")[0].shape == (408, 408)


def test_hofstadter_is_the_harper_hamiltonian():
    A = synthetic.hofstadter(5, 4, 0.25, disorder=0.3, seed=2)
    D = A.toarray()
    assert A.dtype == np.complex128 and A.format == "csr" and A.has_sorted_indices
    assert abs(D - D.conj().T).max() == 0.0
    idx = lambda x, y: x * 4 + y  # noqa: E731
    assert D[idx(3, 1), idx(2, 1)] == -1.0 and D[idx(2, 2), idx(2, 1)] == -np.exp(2j * np.pi * 0.25 * 2)
    assert D[idx(0, 0), idx(4, 0)] == 0.0 and D[idx(0, 0), idx(0, 3)] == 0.0  # open boundaries
    diag = 0.3 * np.random.default_rng(2).uniform(-1, 1, 20)
    assert np.array_equal(np.diag(D), diag + 0j)
    P = synthetic.hofstadter(4, 4, 0.25, periodic=True).toarray()
    assert P[idx(0, 0), idx(3, 0)] == -1.0 and P[idx(1, 0), idx(1, 3)] == -np.exp(2j * np.pi * 0.25)
    # a uniform flux: the phase around every plaquette is exp(2 pi i alpha)
    loop = D[idx(1, 0), idx(0, 0)] * D[idx(1, 1), idx(1, 0)] * D[idx(0, 1), idx(1, 1)] * D[idx(0, 0), idx(0, 1)]
    assert abs(loop - np.exp(2j * np.pi * 0.25)) < 1e-15


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c.name)
def test_trl_converges_on_the_complex_numpy_backend(case):
    A, _, _ = conv_matrix(case.matrix)
    be = NumpyBackend(A)
    theta, info = trl(be, A.shape[0], case.k, case.which, ncv=case.ncv)
    print(info)
    check_pairs(case, theta, be.get_vectors(case.k), case.name)


def test_real_and_complex_start_vectors():
    A, _, _ = conv_matrix("dense96")
    case = CONV_CASES[-1]
    rng = np.random.default_rng(3)
    for v0 in (rng.standard_normal(96), rng.standard_normal(96) + 1j * rng.standard_normal(96)):
        be = NumpyBackend(A)
        theta, _ = trl(be, 96, case.k, case.which, v0=v0)
        check_pairs(case, theta, be.get_vectors(case.k), f"v0 {v0.dtype}")
    with pytest.raises(ValueError, match="v0"):
        trl(NumpyBackend(A), 96, 4, "SA", v0=np.zeros(96))


def test_no_convergence_carries_the_converged_pairs():
    A, _, _ = conv_matrix("hof")
    with pytest.raises(ArpackNoConvergence) as e:
        trl(NumpyBackend(A), 408, 6, "SA", maxiter=1)
    assert e.value.eigenvectors.dtype == np.complex128 and e.value.eigenvectors.shape == (408, len(e.value.eigenvalues))


# ---------------------------------------------------------------- arguments
def test_the_complex_ncv_cap():
    assert check_args(408, 6, "SA", None, complex_A=True) == 20
    assert check_args(408, 6, "SA", 64, complex_A=True) == 64
    with pytest.raises(ValueError, match="complex cap"):
        check_args(408, 6, "SA", 65, complex_A=True)
    with pytest.raises(ValueError, match="complex cap"):
        check_args(408, 40, "SA", None, complex_A=True)  # the default, 81, exceeds it
    assert check_args(408, 40, "SA", None) == 81  # a real matrix keeps its cap
    A, _, _ = conv_matrix("hof")
    with pytest.raises(ValueError, match="complex cap"):
        eigsh_fn(A, k=40)  # (raised before a device is asked for)
    with pytest.raises(ValueError, match="complex cap"):
        eigsh_fn(A, k=6, ncv=8)


@pytest.mark.parametrize("kw", [{"filter_degree": 8, "which": "SA"}, {"sigma": 0.0}, {"block_size": 2}], ids=lambda kw: next(iter(kw)))
def test_real_only_modes_refuse_a_complex_matrix(kw):
    for A in (conv_matrix("hof")[0], conv_matrix("dense96")[0], conv_matrix("hof")[0].astype(np.complex64)):
        with pytest.raises(NotImplementedError, match="complex matrix"):
            eigsh_fn(A, k=4, **kw)


def test_pack_matrix_refuses_complex_input():
    A, D, _ = conv_matrix("hof")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no ComplexWarning either: nothing is converted
        for H in (A, A.tocoo(), A.astype(np.complex64), np.array(D), np.array(D, order="F"), D.astype(np.complex64)):
            with pytest.raises(NotImplementedError, match="complex input: use lanczos_amd.eigsh"):
                _pack_matrix(H)
    kind, rowptr, colidx, vals = _pack_matrix(A.real.tocsr())  # real input keeps its path
    assert kind == "csr" and vals.dtype == np.float64
    assert _pack_matrix(D.real)[0] == "dense"


def test_the_two_sided_class_refuses_complex_input_before_it_converts():
    import lanczos_amd

    A = synthetic.hofstadter(6, 5, 1 / 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for H in (A, A.toarray()):
            s = lanczos_amd.IrrLanczos(H)
            s.verbose = False
            with pytest.raises(NotImplementedError, match="complex input: use lanczos_amd.eigsh"):
                s.execute_Lanczos(5)


class _Recorder:
    """stands in for a ``_capi.Handle``: records what ``upload_complex_matrix`` hands to the device"""

    def set_csr_cplx(self, n, rowptr, colidx, vals):
        self.got = ("csr", n, np.asarray(rowptr), np.asarray(colidx), np.asarray(vals))

    def set_dense_cplx(self, A):
        self.got = ("dense", A)


def test_upload_converts_complex64_and_copies_what_is_not_row_major():
    A, D, _ = conv_matrix("dense96")
    h = _Recorder()
    assert upload_complex_matrix(h, A.astype(np.complex64)) == 96
    assert h.got[1].dtype == np.complex128 and np.array_equal(h.got[1], A.astype(np.complex64).astype(np.complex128))
    F = np.asfortranarray(A)
    for view in (F, F[::1, :]):  # an F-ordered Hermitian array read by rows would be the conjugate
        upload_complex_matrix(h, view)
        assert h.got[1].flags.c_contiguous and np.array_equal(h.got[1], A) and not np.array_equal(h.got[1], A.conj())
    S = conv_matrix("hof")[0]
    for fmt in ("csr", "csc", "coo"):
        upload_complex_matrix(h, S.asformat(fmt).astype(np.complex64))
        kind, n, rowptr, colidx, vals = h.got
        assert kind == "csr" and n == 408 and vals.dtype == np.complex128
        assert abs(sp.csr_matrix((vals, colidx, rowptr), shape=(408, 408)) - S).max() < 1e-6


# ---------------------------------------------------------------- a real backend gets the loop it had
def _trl_before(backend, n, k, which="LM", ncv=None, maxiter=None, tol=0.0, v0=None):
    """the outer loop as it was before the complex path existed (converging runs only), kept here as the yardstick"""
    m = check_args(n, k, which, ncv)
    rng, tol_eff, v0 = _start(n, tol, v0, None)
    backend.begin(m, v0)
    T = np.zeros((m, m))
    kcur, nw, last = 0, k, None
    anorm = 0.0
    draws = 0
    while True:
        j0 = kcur
        while True:
            proj, beta = backend.extend(j0, m)
            for j in range(j0, m):
                T[: j + 1, j] = proj[j, : j + 1]
                T[j, : j + 1] = proj[j, : j + 1]
                if j + 1 < m:
                    T[j + 1, j] = T[j, j + 1] = beta[j]
            scale = max(anorm, np.abs(T).max())
            bad = [j for j in range(j0, m - 1) if not beta[j] > 10 * _EPS * scale]
            if not bad:
                break
            jb = bad[0]
            T[jb + 1:, :] = 0.0
            T[:, jb + 1:] = 0.0
            _fill(T, proj, beta, j0, jb + 1, couplings=False)
            backend.probe(jb + 1, rng.standard_normal(n))
            draws += 1
            j0 = jb + 1
        b_last = beta[m - 1]
        theta, S = np.linalg.eigh((T + T.T) / 2)
        anorm = max(np.abs(theta).max(), anorm)
        res = b_last * np.abs(S[m - 1])
        order = _order(theta, which)
        want = order[:nw]
        ok = res <= tol_eff * anorm
        dead = not b_last > 10 * _EPS * anorm
        done = ok[want].all()
        if done:
            top = order[:k]
            cur = np.sort(theta[top])
            if last is not None and np.abs(cur - last).max() <= 1e3 * tol_eff * anorm:
                sel = top[np.argsort(theta[top], kind="stable")]
                backend.restart(m, k, np.ascontiguousarray(S[:, sel]))
                return theta[sel], draws
            last = cur
            backend.restart(m, nw, np.ascontiguousarray(S[:, want]))
            backend.probe(nw, rng.standard_normal(n))
            draws += 1
            T = np.zeros((m, m))
            T[np.arange(nw), np.arange(nw)] = theta[want]
            kcur, nw = nw, min(nw + 1, m - 3)
        else:
            nconv = int(ok[want].sum())
            kk = min(m - 2, nw + max(nconv, (m - nw) // 2))
            keep = order[:kk]
            backend.restart(m, kk, np.ascontiguousarray(S[:, keep]))
            T = np.zeros((m, m))
            T[np.arange(kk), np.arange(kk)] = theta[keep]
            if dead:
                backend.probe(kk, rng.standard_normal(n))
                draws += 1
            else:
                T[:kk, kk] = T[kk, :kk] = b_last * S[m - 1, keep]
            kcur = kk


@pytest.mark.parametrize("name,which,k", [("lap", "SA", 5), ("lap", "LM", 3), ("diag", "SA", 4)])
def test_a_real_matrix_gets_the_same_bits_as_before(name, which, k):
    """the real loop's arithmetic and its generator's draw sequence: ``lap`` has double eigenvalues (probe rounds), ``diag`` has six
    distinct eigenvalues (breakdowns, fresh directions)"""
    if name == "lap":
        A = synthetic.laplacian_2d_5pt(12, 12).to_scipy()
    else:
        A = sp.diags(np.repeat(np.arange(1.0, 7.0), 10)).tocsr()
    n = A.shape[0]
    old, new = NumpyBackend(A), NumpyBackend(A)
    theta0, draws = _trl_before(old, n, k, which)
    theta1, info = trl(new, n, k, which)
    assert draws >= 1 and draws >= info["probes"] + info["breakdowns"]  # the generator was drawn from: its sequence is part of the check
    assert theta1.dtype == np.float64 and new.V.dtype == np.float64
    assert np.array_equal(theta0, theta1) and np.array_equal(old.V, new.V)
    assert _SEED == 0x5EED


# ---------------------------------------------------------------- the cases of one extension step
Case = collections.namedtuple("Case", "n nb kind force dense seed", defaults=(1,))
CAPTURE = 0.08  # the share of |w|^2 that the rows other than x hold (at most)
# the launch shapes of k_zdots / k_zcgs (lz_ztrl.hip): a padded length of at least 256 * 4 * 256 * 2 = 524288 doubles takes four
# positions per lane, anything shorter one.  524257 is the smallest n that pads to 524288, 524256 the largest of the other branch.
LONG_N = 524257


def _cases():
    out = []
    for n in (33, 1000, 4099):
        for nb in (1, 2, 17, 63)[: 4 if n >= 64 else 3]:  # (63 rows do not fit into 33 dimensions)
            out.append(Case(n, nb, "orth", False, False))  # the gate stays closed
            if nb > 1:
                out.append(Case(n, nb, "near", False, False))  # the gate opens
            out.append(Case(n, nb, "skew" if nb > 1 else "orth", True, False))  # the forced second pass
    out += [Case(33, 17, "near", False, True), Case(1000, 17, "near", False, True), Case(1000, 2, "skew", True, True)]  # the dense product
    out += [Case(LONG_N, 2, "orth", False, False), Case(LONG_N, 5, "skew", True, False), Case(LONG_N - 1, 2, "near", False, False)]
    assert len(set(out)) == len(out)
    return out


STEP_CASES = _cases()


def case_id(c):
    return f"{c.n}-{c.nb}-{c.kind}" + ("-forced" if c.force else "") + ("-dense" if c.dense else "")


@functools.lru_cache(maxsize=None)
def zmatrix(n):
    """Hermitian: three complex standard normal entries per row at random columns plus their mirror images, and a real diagonal"""
    rng = np.random.default_rng(2000 + n)
    r = np.repeat(np.arange(n), 3)
    B = sp.csr_matrix((rng.standard_normal(3 * n) + 1j * rng.standard_normal(3 * n), (r, rng.integers(0, n, 3 * n))), shape=(n, n))
    A = (B + B.conj().T + sp.diags(rng.uniform(0.6, 1.0, n) + 0j)).tocsr()
    A.sort_indices()
    assert abs(A - A.conj().T).max() == 0.0
    return A


def make_rows(A, nb, kind, seed, coupling=0.3):
    """the ``(nb, n)`` complex128 rows of a case, the last one ``x`` (see tests/test_arnoldi_step_host.py)"""
    n = A.shape[0]
    rng = np.random.default_rng([seed, n, nb])

    def draw(count):
        return rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))

    x = draw(1)[0]
    x /= np.linalg.norm(x)
    if nb == 1:
        assert kind == "orth"
        return np.ascontiguousarray(x[None, :])
    w = A @ x
    wp = w - np.vdot(x, w) * x
    wp /= np.linalg.norm(wp)
    G = draw(nb - 1)
    s = min(1.0, np.sqrt(CAPTURE * n / (nb - 1)))
    G -= (1.0 - s) * np.outer(G @ wp.conj(), wp)
    Q = np.linalg.qr(np.vstack([x, G]).T)[0].T  # row 0 is x up to a phase, the others are orthonormal to it
    rows = np.vstack([Q[1:], x])
    if kind == "near":
        g = draw(1)[0] * (np.linalg.norm(w) / np.sqrt(2 * n))
        u = w + 0.05 * g
        rows[0] = u / np.linalg.norm(u)
    elif kind == "skew":
        M = np.eye(nb) + coupling * (rng.standard_normal((nb, nb)) + 1j * rng.standard_normal((nb, nb))) / np.sqrt(2 * nb)
        M[nb - 1] = 0.0
        M[nb - 1, nb - 1] = 1.0  # the last row stays x: the step is the same product
        rows = M @ rows
    else:
        assert kind == "orth"
    return np.ascontiguousarray(rows)


@functools.lru_cache(maxsize=None)
def step_reference(case):
    """``(A, rows, ref)`` of a case, computed once and never changed: ``A`` as the device gets it (CSR, or its dense copy)"""
    A = zmatrix(case.n)
    rows = make_rows(A, case.nb, case.kind, case.seed)
    if case.dense:
        A = A.toarray()
    ref = step(A, rows, case.force)
    for a in (rows, ref["c1"], ref["c2"], ref["v"], ref["e_proj"], ref["e_v"]):
        a.setflags(write=False)
    return A, rows, ref


@pytest.mark.parametrize("case", STEP_CASES, ids=case_id)
def test_step_cases_are_decisive_and_numpy_is_within_the_bounds(case):
    A, rows, ref = step_reference(case)
    wn = ref["w_norm"]
    print(f"{case_id(case):28s} ratio {ref['ratio']:.3f} pass2 {int(ref['pass2'])} max|c2|/|w| {np.abs(ref['c2']).max() / wn:.2e} "
          f"e_proj/|w| {ref['e_proj'].max() / wn:.2e} e_beta/|w| {ref['e_beta'] / wn:.2e} |e_v| {np.linalg.norm(ref['e_v']):.2e}")
    assert abs(ref["ratio"] - 0.5) > 0.15  # the gate is decided far from its edge
    assert ref["pass2"] == (case.force or case.kind == "near")
    if case.kind in ("near", "skew"):
        assert np.abs(ref["c2"]).max() > 1e-3 * wn  # a dropped or doubled second pass shows
    assert ref["e_proj"].max() < 1e-8 * wn and ref["e_beta"] < 1e-8 * wn  # the bounds bind
    if case.kind == "orth":  # <x, A x> is real, and with orthonormal rows so is what pass 2 adds to it
        assert abs((ref["c1"] + ref["c2"])[-1].imag) <= ref["e_proj"][-1]
    be = NumpyBackend(A, force_second_pass=case.force)
    nb = case.nb
    be.V = np.zeros((nb + 1, case.n), dtype=np.complex128)
    be.V[:nb] = rows
    proj, beta = be.extend(nb - 1, nb)
    assert worst(np.abs(proj[nb - 1, :nb] - (ref["c1"] + ref["c2"])), ref["e_proj"]) <= 1.0
    assert worst(abs(beta[nb - 1] - ref["beta"]), ref["e_beta"]) <= 1.0
    assert worst(np.abs(be.V[nb] - ref["v"]), ref["e_v"]) <= 1.0


# ---------------------------------------------------------------- the probe: a row stored at k > 0 behind rows set from the host
PROBE_M = 17
PROBE_KS = (0, 1, 5, 17)


@functools.lru_cache(maxsize=None)
def probe_reference(n):
    """``(A, V, x)``, computed once and never changed: the NumPy backend's ``PROBE_M + 1`` rows after ``extend(0, PROBE_M)`` and the
    direction that is probed"""
    A = zmatrix(n)
    rng = np.random.default_rng([7, n])
    be = NumpyBackend(A)
    be.begin(PROBE_M, rng.standard_normal(n) + 1j * rng.standard_normal(n))
    be.extend(0, PROBE_M)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    for a in (be.V, x):
        a.setflags(write=False)
    return A, be.V, x


def probe_state(V, k):
    """``V`` with the rows at and behind ``k`` filled with NaN: a probe of row ``k`` must not read them"""
    W = V.copy()
    W[k:] = np.nan
    return W


def check_probed_rows(new, old, ref_row, k, tag):
    """the bars of tests/test_gpu_svds_edges.py's ``check_probe`` on complex rows: ``new`` after a probe of row ``k`` from the state
    ``old``, ``ref_row`` what the NumPy backend stored"""
    assert np.isfinite(new[k].view(np.float64)).all(), tag
    assert np.linalg.norm(new[k] - ref_row) <= 1e-10, tag
    assert abs(np.linalg.norm(new[k]) - 1.0) <= 1e-12, tag
    if k:
        assert np.abs(new[:k].conj() @ new[k]).max() <= 1e-12, tag
    keep = np.arange(len(new)) != k
    assert np.array_equal(new[keep], old[keep], equal_nan=True), tag  # the other rows: bit-unchanged


@pytest.mark.parametrize("n", [33, 1000])
def test_probe_on_the_numpy_backend_holds_the_bars(n):
    """what tests/test_gpu_eigsh_complex.py asks of ``lz_ztrl_probe``, asked of the reference first; the row from the NaN-filled state
    is compared with the one from the whole basis"""
    A, V, x = probe_reference(n)
    assert np.abs(V.conj() @ V.T - np.eye(PROBE_M + 1)).max() <= 1e-12
    for k in PROBE_KS:
        clean, be = NumpyBackend(A), NumpyBackend(A)
        clean.V, be.V = V.copy(), probe_state(V, k)
        clean.probe(k, x)
        be.probe(k, x)
        check_probed_rows(be.V, probe_state(V, k), clean.V[k], k, f"n {n} k {k}")
