"""The two-pass re-orthogonalisation sweep through lz_step_reorth at every edge of its launch-time plan, against longdouble
(tests/reorth_reference.py; tests/test_reorth_host.py shows on the CPU what the bounds can see and that every case below lands on
the branch its id names).

Sections of the case list (reorth_reference.cases()): a - forced slice lengths against ragged last slices, modes 0, 1 and fused 2;
b - row counts across the tile boundary of every MFMA and VALU shape, j at 0, 1, the middle and nrows - 1; c - the row split of the
fused mode at G = 1, 2, 64 and its end at 65; d - dynamic LDS above 64 KiB and the automatic VALU fallback; e - every pass-2 arm,
forced and at the automatic rule's thresholds; f - the second stage alone.

One handle per case, knobs and flags set before lz_basis_alloc (the plan is made there), nrows + 2 rows allocated, the two rows
behind the sweep and an unused r filled with NaN from the host.  Every case asserts: the branch its id names (plan()); beta, c and
row j finite; beta within gamma_(rows_pad+1); c within gamma_K sum|V_i||w| of the longdouble coefficients, K from the kernels'
summation tree; row j equal BIT FOR BIT to the NumPy replay of pass 2 on the device's own c and beta; every other row, the NaN rows
and r unchanged bit for bit; and a second (mode 0) sweep on the fetched rows held to the same standard, which it could not meet if
the first had left anything but zero in the padding [rows, rows_pad) of row j.
"""
import numpy as np
import pytest
import reorth_reference as R

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def open_case(hip, case, V, r):
    h = hip.Handle(0)
    h.set_options(case.flags)
    for knob, value in case.knobs:
        h.set_tuning(knob, value)
    ptr = np.arange(case.M + 1, dtype=np.int32)
    h.set_csr(case.M, 0, ptr, ptr[:-1], np.ones(case.M))
    h.basis_alloc(case.nrows + 2)
    h.basis_set_rows(0, V)
    h.r_set(r)
    return h


def fetch(h, n):
    return np.stack([h.basis_get_row(i) for i in range(n)])


def check_sweep(case, p, V, r, mode, beta, c, rows, what):
    """one sweep of rows V (as uploaded or fetched) that left `rows`: bounds on beta and c, bit equality of the rest"""
    j, nrows, rows_pad = case.j, case.nrows, R.padded(case.M)
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(rows[j])), f"{case.id} {what}: not finite"
    ref = R.sweep_reference(V, j, nrows, r, mode, beta=beta if mode == 1 else None)
    if mode:
        assert np.isfinite(beta) and abs(beta - ref.beta) <= R.gamma(R.beta_K(rows_pad)) * ref.beta, f"{case.id} {what}: beta {beta} against {ref.beta}"
    K = R.coef_K(p, rows_pad, nrows, mode)
    over = np.abs(c - ref.c) / (R.gamma(K) * ref.c_mag)
    print(f"{case.id} {what}: K = {K}, worst coefficient at {float(over.max()):.3g} of its bound")
    assert np.all(over <= 1.0), f"{case.id} {what}: c[{int(over.argmax())}] at {float(over.max()):.3g} of its bound (K = {K})"
    w = V[j] if mode == 0 else r / beta
    expect = R.replay_row(V, j, nrows, c, w)
    assert np.array_equal(rows[j], expect), f"{case.id} {what}: row j differs from the replay at {np.flatnonzero(rows[j] != expect)[:5]}"
    others = [i for i in range(nrows) if i != j]
    assert same_bits(rows[others], V[others]), f"{case.id} {what}: a row other than j changed"
    assert np.all(np.isnan(rows[nrows:])), f"{case.id} {what}: a row behind the sweep was written"


def run_case(hip, case):
    p = R.assert_claim(case)
    V, r = R.case_inputs(case)
    n = case.nrows + 2
    h = open_case(hip, case, V, r)
    try:
        beta, c = h.step_reorth(case.j, case.nrows, scale=case.mode != 0)
        rows = fetch(h, n)
        assert same_bits(h.r_get(), r), f"{case.id}: r changed"
        check_sweep(case, p, V, r, case.mode, beta, c, rows, "first sweep")
        # the second sweep: mode 0 on what the first left
        p2 = R.plan(R.padded(case.M), case.flags, dict(case.knobs), n, case.nrows, 0)
        _, c2 = h.step_reorth(case.j, case.nrows, scale=False)
        rows2 = fetch(h, n)
        assert same_bits(h.r_get(), r), f"{case.id}: r changed in the second sweep"
        check_sweep(case, p2, rows, None, 0, None, c2, rows2, "second sweep")
    finally:
        h.close()
    return beta, c, rows


def _ids(sec):
    return [c for c in R.cases() if c.id.startswith(sec + "-")]


def _param(sec):
    return pytest.mark.parametrize("case", _ids(sec), ids=lambda c: c.id)


@_param("a")
def test_slices(hip, case):
    run_case(hip, case)


@_param("b")
def test_tiles(hip, case):
    run_case(hip, case)


@_param("c")
def test_row_split(hip, case):
    """The split deals a slice's row tiles to Y blocks; every (row, slice, quarter) dot stays one wave's same MFMA sequence and
    every block writes its own rows of the slice's run (k_qtw_mfma4), so the code says the per-row sums do not change: the case at
    G = 1, nrows = 200 (Y = 25) is compared BIT FOR BIT with unsplit calls on the same input - a mode-0 call on V[j] = r, whose raw
    sums go through k_fused_prepare's expressions on the host (all 200 coefficients), and the fused call on the first 8 rows."""
    beta, c, _ = run_case(hip, case)
    if (case.claim["G"], case.nrows) != (1, 200):
        return
    V, r = R.case_inputs(case)
    j = case.j
    raw_case = case._replace(mode=0, flags=case.flags & ~R.FLAG_FUSED)
    Vr = V.copy()
    Vr[j] = r
    assert R.case_plan(raw_case).Y == 1
    h = open_case(hip, raw_case, Vr, r)
    _, raw = h.step_reorth(j, case.nrows, scale=False)
    h.close()
    b = np.sqrt(raw[j])
    assert beta == b
    assert np.array_equal(c[:j], raw[:j] / b) and c[j] == raw[j] / (b * b)
    few = case._replace(nrows=8, j=7)
    assert R.case_plan(few).Y == 1
    h = open_case(hip, few, V[:10], r)
    beta8, c8 = h.step_reorth(7, 8, scale=True)
    h.close()
    assert beta8 == beta and np.array_equal(c8[:7], c[:7])


@_param("d")
def test_big_lds_and_valu_fallback(hip, case):
    if "lds" in case.claim:
        assert case.claim["lds"] > 65536
    else:
        assert case.flags & R.FLAG_VALU == 0 and case.claim["family"] == 0
    run_case(hip, case)


@_param("e")
def test_update_arms(hip, case):
    run_case(hip, case)


@_param("f")
def test_second_stage(hip, case):
    run_case(hip, case)
