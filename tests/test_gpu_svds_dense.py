"""The dense operator of lanczos_amd.svds on the device (lz_gk_set_dense): both products in every form against exact integer and
longdouble references, the extension step against NumPy, svds end to end against numpy.linalg.svd and the host loop, handle reuse, errors.

The products' bar is derived, not measured: n eps (|S| |x|) per output for n terms, twice Higham's gamma_n for any summation order."""
import numpy as np
import pytest
import scipy.sparse
from test_svds_dense_host import CASES, case_id, case_matrix, host_run
from test_svds_host import check_triplets, random_sparse

import lanczos_amd
from lanczos_amd import _capi
from lanczos_amd.svds import NumpyGKBackend

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps

# form codes of lz_gk_plan (include/lanczos_hip.h) and the constants of the kernels (lanczos_amd/csrc/lz_internal.h, lz_gk.hip)
RD_SHORT, RD_WAVE, RD_SEG = 1, 2, 3
CS_SLAB, CS_ONE, CS_NARROW = 11, 12, 13
KNOB_FORMS, KNOB_SEG, KNOB_SLAB = 14, 4, 2  # rowdot form + 4 * colsum form (0: by shape), segment length, rows per slab
TILE_COLS = 128  # colsum: columns per workgroup tile; below it the narrow form
SHORT_MAX = 128  # rowdot: the longest row of the lane-group form
MEDIUM_MAX = 1024  # rowdot: the longest row that a wave takes whole in groups of four (the segment form with one segment)
SEG_MAX_ROWS = 768  # rowdot: longer rows are cut into segments only when there are fewer of them than this
SEG = 128        # the segment length the forced runs set (knob 4): C = 127, 128, 129 and 257 lie on both sides of its edges
SLAB = 256       # the slab height the forced runs set (knob 2): R = 255, 256, 257 lie on both sides of its edge
COLS = [2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 1024, 1025]
ROWS = [2, 3, 255, 256, 257, 1501]
GRID = [(R, Cn) for R in ROWS for Cn in COLS]
# the automatic plan's own edges: 767 / 768 rows (two segments or a wave per row), 35 segments and 547 column tiles with few rows
# (one slab by the tiles alone), a wide matrix of 65 rows
AUTO_EDGES = [(SEG_MAX_ROWS - 1, 2100), (SEG_MAX_ROWS, 2100), (3, 70001), (65, 4100), (129, 128)]
assert SHORT_MAX in COLS and SHORT_MAX + 1 in COLS and MEDIUM_MAX in COLS and MEDIUM_MAX + 1 in COLS and TILE_COLS - 1 in COLS and TILE_COLS in COLS and SEG in COLS and SEG + 1 in COLS
assert SLAB - 1 in ROWS and SLAB in ROWS and SLAB + 1 in ROWS

_refs = {}


def product_inputs(R, Cn):
    """integer and Gaussian S (R x C), x (C) and u (R) with their references, computed once and never written to"""
    if (R, Cn) not in _refs:
        rng = np.random.default_rng(1000 * R + Cn)
        Si = rng.integers(-3, 4, (R, Cn)).astype(np.float64)
        xi, ui = rng.integers(-4, 5, Cn).astype(np.float64), rng.integers(-4, 5, R).astype(np.float64)
        Sg, xg, ug = rng.standard_normal((R, Cn)), rng.standard_normal(Cn), rng.standard_normal(R)
        Sl = Sg.astype(np.longdouble)
        ref = {"Si": Si, "xi": xi, "ui": ui, "Sg": Sg, "xg": xg, "ug": ug,
               "rowdot_int": Si @ xi, "colsum_int": Si.T @ ui,  # (exact: every partial sum is an integer below 2^53)
               "rowdot": Sl @ xg.astype(np.longdouble), "colsum": Sl.T @ ug.astype(np.longdouble),
               "rowdot_bar": Cn * EPS * (np.abs(Sg) @ np.abs(xg)), "colsum_bar": R * EPS * (np.abs(Sg).T @ np.abs(ug))}
        for v in ref.values():
            v.setflags(write=False)
        _refs[R, Cn] = ref
    return _refs[R, Cn]


def check_products(h, R, Cn, want_rd=None, want_cs=None):
    """S (R x C) as the dense operator of h - stored tall for R >= C, else wide -: both directions, every check; -> (plan, worst ratios)"""
    ref = product_inputs(R, Cn)
    wide = R < Cn
    worst = {}
    for kind in ("int", "gauss"):
        S = ref["Si" if kind == "int" else "Sg"]
        h.gk_set_dense(S, stored_transposed=wide)
        plan = h.gk_plan()
        rd, cs = (plan[3], plan[2]) if wide else (plan[2], plan[3])
        assert plan[:2] == (1, int(wide)) and rd in (RD_SHORT, RD_WAVE, RD_SEG) and cs in (CS_SLAB, CS_ONE, CS_NARROW), plan
        if want_rd is not None:
            assert (rd, cs) == (want_rd, want_cs), (R, Cn, plan)
        # rowdot is Aop x when stored tall and Aop^T u when stored wide; colsum the other one
        for name, vec, length, transpose in (("rowdot", "x", R, wide), ("colsum", "u", Cn, not wide)):
            v = ref[vec + ("i" if kind == "int" else "g")]
            y = h.gk_spmv(v, transpose=transpose)  # (the call pre-fills y and the padding of its input with NaN)
            tag = (name, R, Cn, plan)
            assert y.shape == (h.padded_rows(length),), tag
            assert np.all(np.isfinite(y[:length])) and np.array_equal(y[length:], np.zeros(len(y) - length)), tag
            assert np.array_equal(h.gk_spmv(v, transpose=transpose), y), tag  # same call, same bits
            if kind == "int":
                assert np.array_equal(y[:length], ref[name + "_int"]), tag
            else:
                err = np.abs(y[:length].astype(np.longdouble) - ref[name]).astype(np.float64)
                worst[name] = float((err / ref[name + "_bar"]).max())
                assert np.all(err <= ref[name + "_bar"]), (tag, worst[name])
    return (rd, cs), worst


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


def set_knobs(h, rd=0, cs=0, seg=0, slab=0):
    for knob, v in ((KNOB_FORMS, rd + 4 * cs), (KNOB_SEG, seg), (KNOB_SLAB, slab)):
        h.set_tuning(knob, v)


def test_products_automatic_plan(handle):
    set_knobs(handle)
    seen_rd, seen_cs, worst = set(), set(), {"rowdot": 0.0, "colsum": 0.0}
    for R, Cn in GRID + AUTO_EDGES:
        (rd, cs), w = check_products(handle, R, Cn)
        seen_rd.add(rd)
        seen_cs.add(cs)
        worst = {k: max(worst[k], w[k]) for k in worst}
        # the selection rule
        assert (rd == RD_SHORT) == (Cn <= SHORT_MAX) and (cs == CS_NARROW) == (Cn < TILE_COLS), (R, Cn, rd, cs)
        if SHORT_MAX < Cn <= MEDIUM_MAX:
            assert rd == RD_SEG, (R, Cn, rd)
    print(f"\nautomatic plan: worst error / bound rowdot {worst['rowdot']:.3f} colsum {worst['colsum']:.3f}")
    assert seen_rd == {RD_SHORT, RD_WAVE, RD_SEG} and seen_cs == {CS_SLAB, CS_ONE, CS_NARROW}
    set_knobs(handle)
    handle.gk_set_dense(product_inputs(SEG_MAX_ROWS - 1, 2100)["Sg"], stored_transposed=True)
    assert handle.gk_plan() == (1, 1, CS_SLAB, RD_SEG)
    handle.gk_set_dense(product_inputs(SEG_MAX_ROWS, 2100)["Sg"], stored_transposed=True)
    assert handle.gk_plan() == (1, 1, CS_SLAB, RD_WAVE)
    handle.gk_set_dense(product_inputs(3, 70001)["Sg"], stored_transposed=True)
    assert handle.gk_plan() == (1, 1, CS_ONE, RD_SEG)


@pytest.mark.parametrize("force", [1, 2, 3])
def test_products_forced_forms(handle, force):
    """knob 14 forces a form of either product at any shape; knobs 4 / 2 put the segment and slab edges inside the grid"""
    set_knobs(handle, rd=force, cs=force, seg=SEG, slab=SLAB)
    worst = {"rowdot": 0.0, "colsum": 0.0}
    try:
        for R, Cn in GRID:
            _, w = check_products(handle, R, Cn, want_rd=RD_SHORT + force - 1, want_cs=CS_SLAB + force - 1)
            worst = {k: max(worst[k], w[k]) for k in worst}
    finally:
        set_knobs(handle)
    print(f"\nforced form {force}: worst error / bound rowdot {worst['rowdot']:.3f} colsum {worst['colsum']:.3f}")


def test_knobs_are_clamped(handle):
    """a segment length below 64 or odd, a slab height of 2^30: clamped as knob 4 is, the products stay right"""
    set_knobs(handle, rd=3, cs=1, seg=7, slab=1 << 30)
    try:
        check_products(handle, 257, 129, want_rd=RD_SEG, want_cs=CS_SLAB)
        set_knobs(handle, rd=3, cs=1, seg=(1 << 30) + 1, slab=1)
        check_products(handle, 257, 129, want_rd=RD_SEG, want_cs=CS_SLAB)
    finally:
        set_knobs(handle)


def test_host_rows_further_apart_than_their_length(handle):
    """ld_host > the row length: a column slice of a wider array gives the bits of its contiguous copy"""
    rng = np.random.default_rng(7)
    for R, Cn in ((300, 37), (37, 300)):
        big = rng.standard_normal((R, Cn + 11))
        S = big[:, 5 : 5 + Cn]
        assert S.strides == (8 * (Cn + 11), 8)
        x, u = rng.standard_normal(Cn), rng.standard_normal(R)
        out = []
        for arr in (S, np.ascontiguousarray(S)):
            handle.gk_set_dense(arr, stored_transposed=R < Cn)
            out.append((handle.gk_spmv(x, transpose=R < Cn), handle.gk_spmv(u, transpose=R >= Cn)))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
        assert np.abs(out[0][0][:R] - S @ x).max() <= Cn * EPS * (np.abs(S) @ np.abs(x)).max()


@pytest.mark.parametrize("shape,m,stored_t,force", [((700, 257), 20, False, False), ((700, 257), 20, True, False), ((700, 257), 20, False, True),
                                                    ((2000, 33), 33, False, False), ((2000, 33), 33, True, False)])
def test_extension_steps_match_numpy(shape, m, stored_t, force):
    p, q = shape
    A = case_matrix(shape)
    nrm = np.linalg.norm(A, 2)
    v0 = np.random.default_rng(p + m).standard_normal(q)
    be = NumpyGKBackend(A, force_second_pass=force)
    be.begin(m, v0)
    rc, ra, rb = be.extend(0, m)
    h = _capi.Handle(0)
    if force:
        h.set_options(_capi.FLAG_TRL_PASS2_ALWAYS)
    h.gk_set_dense(np.ascontiguousarray(A.T) if stored_t else A, stored_transposed=stored_t)
    assert h.gk_plan()[:2] == (1, int(stored_t))
    h.gk_begin(m, v0)
    colproj, alpha, beta = h.gk_extend(0, m)
    U, V = h.gk_get_rows(0, 0, m + 1), h.gk_get_rows(1, 0, m + 1)
    h.close()
    print(f"\n{shape} m={m} stored_t={stored_t} force={force}: colproj {np.abs(colproj - rc).max() / nrm:.2e} alpha "
          f"{np.abs(alpha - ra).max() / nrm:.2e} beta {np.abs(beta - rb).max() / nrm:.2e} rows "
          f"{np.abs(U[:m, :p] - be.U[:m]).max():.2e} {np.abs(V[:, :q] - be.V).max():.2e}")
    assert np.abs(colproj - rc).max() <= 1e-12 * nrm
    assert np.abs(alpha - ra).max() <= 1e-12 * nrm
    assert np.abs(beta - rb).max() <= 1e-12 * nrm
    assert np.linalg.norm(U[:m, :p] - be.U[:m], axis=1).max() <= 1e-10
    # (2000, 33) with m = 33 = q exhausts the short space: beta[m - 1] is rounding noise and V[m] that noise normalised, on both sides
    last = m - 1 if m == q else m
    assert np.linalg.norm(V[: last + 1, :q] - be.V[: last + 1], axis=1).max() <= 1e-10
    assert not U[:, p:].any() and not V[:, q:].any() and not U[m].any()  # zero padding, zero row U[m]


_device_runs = {}


def device_run(case):
    if case not in _device_runs:
        shape, order, k, which = case
        info = {}
        u, s, vh = lanczos_amd.svds(case_matrix(shape, order), k=k, which=which, info=info)
        _device_runs[case] = (u, s, vh, info)
    return _device_runs[case]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_svds_dense_on_the_device(case):
    shape, order, k, which = case
    A = case_matrix(shape, order)
    u, s, vh, info = device_run(case)
    assert info["plan"] == "dense"
    check_triplets(A, u, s, vh, which, k, info)
    host_cycles = host_run(case)[3]["cycles"]
    assert abs(info["cycles"] - host_cycles) <= 2, f"{case_id(case)}: {info['cycles']} cycles on the device, {host_cycles} on the host loop"
    assert info["breakdowns"] == 0
    if order == "F":
        # the F-ordered M x N array is the C-ordered N x M transpose: the device holds the same S, u and vh change places
        u2, s2, vh2 = lanczos_amd.svds(np.ascontiguousarray(A.T), k=k, which=which)
        assert np.array_equal(s, s2) and np.array_equal(u, vh2.T) and np.array_equal(vh, u2.T)


def test_sparse_enough_dense_input_still_runs_as_csr():
    A = random_sparse(300, 120).toarray()
    info, info2 = {}, {}
    u, s, vh = lanczos_amd.svds(A, k=6, info=info)
    u2, s2, vh2 = lanczos_amd.svds(scipy.sparse.csr_matrix(A), k=6, info=info2)
    assert info["plan"] == "csr" and info2["plan"] == "csr"
    assert np.array_equal(u, u2) and np.array_equal(s, s2) and np.array_equal(vh, vh2)


def test_one_handle_serves_dense_sparse_dense():
    jobs = [(case_matrix((700, 257)), 4, "dense"), (random_sparse(300, 120), 6, "csr"), (case_matrix((65, 4100), "F"), 4, "dense")]
    fresh = [lanczos_amd.svds(A, k=k) for A, k, _ in jobs]
    h = _capi.Handle(0)
    for (A, k, plan), ref in zip(jobs, fresh):
        info = {}
        out = lanczos_amd.svds(A, k=k, handle=h, info=info)
        assert info["plan"] == plan and h.gk_plan()[0] == (1 if plan == "dense" else 0)
        assert all(np.array_equal(a, b) for a, b in zip(out, ref))
    h.close()


def test_dense_svds_leaves_the_square_problem_of_its_handle_alone():
    S = random_sparse(500, 500, density=0.02, seed=41)
    S = (S + S.T).tocsr()
    h = _capi.Handle(0)
    theta, Y = lanczos_amd.eigsh(S, k=4, which="LA", handle=h)
    res = h.trl_residuals(4, theta)
    info = {}
    lanczos_amd.svds(case_matrix((600, 65)), k=4, handle=h, info=info)
    assert info["plan"] == "dense"
    assert np.array_equal(h.trl_get_vectors(4), Y) and np.array_equal(h.trl_residuals(4, theta), res)  # matrix and basis untouched
    theta2, Y2 = lanczos_amd.eigsh(S, k=4, which="LA", handle=h)
    h.close()
    assert np.array_equal(theta, theta2) and np.array_equal(Y, Y2)


def test_errors_before_any_launch():
    h = _capi.Handle(0)
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE.*lz_gk_plan: no rectangular matrix"):
        h.gk_plan()
    S = np.ones((6, 4))
    need = "LZ_ERR_ARG.*lz_gk_set_dense: need p >= q >= 2"

    def call(p, q, ptr, ld, flag):
        h.check(h.lib.lz_gk_set_dense(h._h, p, q, ptr, ld, flag))

    with pytest.raises(_capi.LanczosHipError, match=need):
        call(4, 6, _capi.dptr(S), 6, 0)  # p < q
    with pytest.raises(_capi.LanczosHipError, match=need):
        call(6, 1, _capi.dptr(S), 1, 0)  # q < 2
    with pytest.raises(_capi.LanczosHipError, match=need):
        call(6, 4, _capi.dptr(S), 3, 0)  # ld_host below the row length of a p x q array
    with pytest.raises(_capi.LanczosHipError, match=need):
        call(6, 4, _capi.dptr(S), 5, 1)  # ... and of a q x p one
    with pytest.raises(_capi.LanczosHipError, match=need):
        call(6, 4, None, 4, 0)  # NULL
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE"):
        h.gk_plan()  # none of them set anything
    assert h.lib.lz_gk_plan(h._h, None) != 0
    h.close()
    hc = _capi.Handle(0)
    hc.comm_init_host(1, 0, lambda a: None)
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE.*lz_gk_set_dense: the Golub-Kahan-Lanczos solver runs on one rank"):
        hc.gk_set_dense(S)
    with pytest.raises(_capi.LanczosHipError, match="LZ_ERR_STATE.*lz_gk_set_csr: the Golub-Kahan-Lanczos solver runs on one rank"):
        hc.gk_set_csr(scipy.sparse.csr_matrix(S), scipy.sparse.csr_matrix(S.T))
    hc.close()
