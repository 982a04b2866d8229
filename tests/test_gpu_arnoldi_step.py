"""lz_trl_extend as an Arnoldi step, against longdouble: one step on rows set from the host under the reference's derived bounds
(tests/arnoldi_reference.py; the cases and what makes them decisive: tests/test_arnoldi_step_host.py), nothing of pass 2 behind a
closed gate, the Arnoldi relation A V_m^T = V_{m+1}^T H over an extension, a Krylov-Schur restart and a second extension on every
product plan with a non-symmetric matrix, and the recovery from a breakdown (NaN rows, probe, re-extension) on the plans that had
never seen one."""
import functools

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
from arnoldi_reference import EPS, relation, worst
from test_arnoldi_step_host import STEP_CASES, THREE_KINDS, Case, case_id, matrix, reference
from test_eigs_host import matrix as eigs_matrix
from test_gpu_eigs import _stencil_csr
from test_gpu_kernels import layered_stencil27

from lanczos_amd import _capi
from lanczos_amd.eigs import DeviceCplxBackend, NumpyCplxBackend, _blocks, _front, _rank, _take

pytestmark = pytest.mark.gpu


def _handle(A, flags=0, tune=()):
    h = _capi.Handle(0)
    for index, value in tune:
        h.set_tuning(index, value)
    h.set_options(flags)
    if sp.issparse(A):
        h.set_csr(A.shape[0], 0, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data)
    else:
        h.set_dense(A)
    return h


# ---------------------------------------------------------------- a. one step against the reference
def one_step(h, case, rows, ref, label):
    """rows 0 .. nb - 1 set from the host, step nb - 1 on the device: everything it returns under the reference's bounds"""
    n, nb = case.n, case.nb
    pad = h.padded_rows(n)
    V = np.zeros((nb, pad))
    V[:, :n] = rows
    h.trl_set_rows(0, V)
    proj, beta = h.trl_extend(nb - 1, nb)
    out = h.trl_get_rows(0, nb + 1)
    err = {"proj": worst(np.abs(proj[nb - 1, :nb] - (ref["c1"] + ref["c2"])), ref["e_proj"]),
           "beta": worst(abs(beta[nb - 1] - ref["beta"]), ref["e_beta"]), "v": worst(np.abs(out[nb, :n] - ref["v"]), ref["e_v"])}
    print(f"{label:44s} error / bound: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert np.all(np.isfinite(proj[nb - 1])) and np.isfinite(beta[nb - 1])
    assert all(v <= 1.0 for v in err.values()), err
    assert np.array_equal(out[:nb], V)  # the rows below are only read
    assert np.all(out[nb, n:] == 0.0)  # the new row's padding


def _step_params():
    out = [(c, 0) for c in STEP_CASES]
    out += [(c, _capi.FLAG_QTW_VALU) for c in STEP_CASES if (c.n, c.nb) in THREE_KINDS and not c.dense]
    return out


@pytest.mark.parametrize("case,flags", _step_params(), ids=lambda p: case_id(p) if isinstance(p, Case) else ("valu" if p else "default"))
def test_one_step_within_the_reference_bounds(case, flags):
    A, rows, ref = reference(case)
    h = _handle(A, flags | (_capi.FLAG_TRL_PASS2_ALWAYS if case.force else 0))
    assert (h.spmv_plan() == "dense") == case.dense
    h.trl_begin(case.nb, np.ones(case.n))
    one_step(h, case, rows, ref, case_id(case) + (" valu" if flags else ""))
    h.close()


# ---------------------------------------------------------------- b. nothing leaks behind a closed gate
@pytest.mark.parametrize("n,nb", THREE_KINDS)
def test_no_second_pass_leaks_behind_a_closed_gate(n, nb):
    """a step whose gate opens, then one on the same handle whose gate stays closed: the second returns pass 1's coefficients alone"""
    thin = next(c.thin for c in STEP_CASES if (c.n, c.nb) == (n, nb))
    near, orth = Case(n, nb, "near", False, False, 1, thin), Case(n, nb, "orth", False, False, 1, thin)
    assert near in STEP_CASES and orth in STEP_CASES
    A, rows, ref = reference(near)
    assert ref["pass2"] and not reference(orth)[2]["pass2"]
    h = _handle(A)
    h.trl_begin(nb, np.ones(n))
    one_step(h, near, rows, ref, case_id(near) + " (gate open)")
    one_step(h, orth, reference(orth)[1], reference(orth)[2], case_id(orth) + " (then closed)")
    h.close()


# ---------------------------------------------------------------- c. the relation over a cycle, per product plan
def _stencil5_csr(nx, ny):
    """a constant-coefficient non-symmetric 5-point stencil on a periodic nx x ny grid"""
    def ring(n, lo, hi):
        S = sp.diags([np.full(n - 1, lo), np.full(n - 1, hi)], [-1, 1], format="lil")
        S[0, n - 1] += lo
        S[n - 1, 0] += hi
        return S.tocsr()
    A = (sp.kron(sp.identity(ny), ring(nx, -1.4, -0.6)) + sp.kron(ring(ny, -1.1, -0.9), sp.identity(nx)) + 4.0 * sp.identity(nx * ny)).tocsr()
    A.sort_indices()
    return A


def _fill(H, proj, beta, j0, m):
    for j in range(j0, m):
        H[: j + 1, j] = proj[j, : j + 1]
        H[j + 1, j] = beta[j]


def cycle(be, basis, A, n, m, k):
    """An extension, a Krylov-Schur restart and a second extension, driven as ``krylov_schur`` drives them; ``basis()`` returns the
    ``m + 1`` basis rows.  Returns ``[(stage, worst column defect of the relation, max|V V^T - I|, max|H|)]`` of the three stages."""
    be.begin(m, np.random.default_rng(5).uniform(-1.0, 1.0, n))
    be.set_filter(None)
    H = np.zeros((m + 1, m))
    proj, beta = be.extend(0, m)
    _fill(H, proj, beta, 0, m)
    out = []

    def stage(name, cols):
        defect, orth = relation(A, basis()[: cols + 1], H[: cols + 1, :cols])
        out.append((name, float(defect.max()), orth, float(np.abs(H).max())))

    stage("extend", m)
    R, Q = scipy.linalg.schur(H[:m], output="real")
    blocks = _blocks(R)
    chosen, kq = _take(blocks, _rank(blocks, "LM"), k)
    R, Q = _front(R, Q, blocks, chosen)
    blocks = _blocks(R)
    lead = [b for b in range(len(blocks)) if blocks[b][0] < kq]
    rest = [b for b in _rank(blocks, "LM") if blocks[b][0] >= kq]
    extra, kk = _take(blocks, rest, min(m - 3, k + (m - k) // 2) - kq)
    kk += kq
    R, Q = _front(R, Q, blocks, lead + extra)
    be.restart(m, kk, np.ascontiguousarray(Q[:, :kk]))
    b_last = beta[m - 1]
    H[:] = 0.0
    H[:kk, :kk] = R[:kk, :kk]
    H[kk, :kk] = b_last * Q[m - 1, :kk]
    stage("restart", kk)
    proj, beta = be.extend(kk, m)
    _fill(H, proj, beta, kk, m)
    stage("extend again", m)
    return out


@functools.lru_cache(maxsize=None)
def plan_matrix(name):
    if name in ("csr-stream", "scalar", "dense", "csr-stream-m128"):
        return eigs_matrix("c")
    if name == "two-phase":
        return matrix(5000)
    if name == "stencil7":
        return _stencil_csr(7, 9, 11)
    if name == "stencil5":
        return _stencil5_csr(23, 19)
    if name == "stencil27":
        return layered_stencil27()[0]
    raise KeyError(name)


def plan_handle(name, A):
    """the handle of a plan with ``A`` on it, the plan asserted"""
    if name == "scalar":
        h = _handle(A, _capi.FLAG_SPMV_SCALAR)
    elif name == "two-phase":
        h = _handle(A, tune=[(_capi.TUNE_SPMV_PLAN, 2)])
    elif name == "dense":
        h = _handle(A.toarray())
    else:
        h = _handle(A)
    want = {"stencil7": "fixed-k", "stencil5": "fixed-k", "stencil27": "fixed-k", "csr-stream-m128": "csr-stream"}.get(name, name)
    assert h.spmv_plan() == want, (name, h.spmv_plan())
    if name.startswith("stencil"):
        assert h.spmv_coding()[0] == "offsets+values", h.spmv_coding()
    if name == "stencil27":
        assert h.spmv_coding() == ("offsets+values", 216)
    return h


def _bars(numpy_stages, m):
    """per stage: ten times the larger of the NumPy backend's figure and ``m eps max|H|`` (orthonormality: ``m eps``)"""
    return [(10 * max(d, m * EPS * hmax), 10 * max(o, m * EPS)) for _, d, o, hmax in numpy_stages]


@pytest.mark.parametrize("name,m", [("csr-stream", 20), ("scalar", 20), ("two-phase", 20), ("dense", 20), ("stencil7", 20), ("stencil5", 20),
                                    ("stencil27", 20), ("csr-stream-m128", 128)])
def test_arnoldi_relation_over_a_cycle(name, m):
    A = plan_matrix(name)
    assert abs(A - A.T).max() > 0.1
    n, k = A.shape[0], 4
    nb = NumpyCplxBackend(A.toarray() if name == "dense" else A)
    bars = _bars(cycle(nb, lambda: nb.V, A, n, m, k), m)
    h = plan_handle(name, A)
    be = DeviceCplxBackend(h, n)
    got = cycle(be, lambda: h.trl_get_rows(0, m + 1)[:, :n], A, n, m, k)
    h.close()
    for (stage, defect, orth, _), (bar_d, bar_o) in zip(got, bars):
        print(f"{name:16s} m={m:3d} {stage:13s} defect {defect:.2e} (bar {bar_d:.2e})  |V V^T - I| {orth:.2e} (bar {bar_o:.2e})")
    for (stage, defect, orth, _), (bar_d, bar_o) in zip(got, bars):
        assert defect <= bar_d and orth <= bar_o, stage


# ---------------------------------------------------------------- d. recovery from a breakdown, per plan
def _empty_column(A, p):
    """``A`` with column ``p`` zeroed; the entries stay (explicit zeros), so a fixed-k matrix keeps its row lengths"""
    A = A.copy().tocsr()
    A.data[A.indices == p] = 0.0
    return A


@pytest.mark.parametrize("name", ["dense", "two-phase", "stencil7", "scalar"])
def test_breakdown_recovery(name):
    """``v0 = e_p`` with column ``p`` of ``A`` empty: step 0 gives ``w = 0`` exactly, ``beta_0 = 0`` and NaN in every later row; the probe and the
    re-extension from row 1 must leave a finite basis with zero paddings for which the relation holds (on columns ``1 .. m - 1``)"""
    m, p = 20, 7
    A = _empty_column(_stencil_csr(7, 9, 11) if name == "stencil7" else matrix(1501), p)
    n = A.shape[0]
    assert n % 32 != 0 and not np.any(A[:, [p]].toarray())
    v0 = np.zeros(n)
    v0[p] = 1.0
    x = np.random.default_rng(9).standard_normal(n)

    def after_the_probe(be, basis):
        be.probe(1, x)
        proj, beta = be.extend(1, m)
        H = np.zeros((m + 1, m))
        _fill(H, proj, beta, 1, m)
        defect, orth = relation(A, basis(), H)
        return proj, beta, float(defect[1:].max()), orth, float(np.abs(H).max())

    nb = NumpyCplxBackend(A.toarray() if name == "dense" else A)
    nb.begin(m, v0)
    _, _, d0, o0, hmax = after_the_probe(nb, lambda: nb.V)
    bar_d, bar_o = 10 * max(d0, m * EPS * hmax), 10 * max(o0, m * EPS)

    h = plan_handle(name, A)
    if name == "stencil7":
        assert int(np.diff(A.indptr).min()) == 7
    h.trl_begin(m, v0)
    proj, beta = h.trl_extend(0, m)
    assert proj[0, 0] == 0.0 and beta[0] == 0.0
    rows = h.trl_get_rows(0, m + 1)
    assert np.array_equal(rows[0, :n], v0) and not np.any(np.isfinite(rows[1:, :n]))
    be = DeviceCplxBackend(h, n)
    proj, beta, defect, orth, _ = after_the_probe(be, lambda: h.trl_get_rows(0, m + 1)[:, :n])
    rows = h.trl_get_rows(0, m + 1)
    h.close()
    print(f"{name:10s} after the breakdown: defect {defect:.2e} (bar {bar_d:.2e})  |V V^T - I| {orth:.2e} (bar {bar_o:.2e})")
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(proj[1:])) and np.all(np.isfinite(beta[1:]))
    assert np.all(rows[:, n:] == 0.0)
    assert defect <= bar_d and orth <= bar_o
