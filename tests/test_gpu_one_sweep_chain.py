"""The group form's chain in the units of z and its side stream (one_sweep_quad_iter; TUNE_LOOP = 10 against 12 and 13), each against the
form it replaces on the same matrix and start vector.

Part A, the chain (TUNE_LOOP 10: the unscaled chain - k_three_term_z, the plain coded product, k_final_sum_chain, the walk dividing all four
vectors on read -, 12: the scaled chain through the scale-on-read SpMV): both runs form (n - 2) // 4 groups with no abandon and no gate
trip, each satisfies tests/lanczos_invariants.py against the six-launch loop, and the two agree within the bars
tests/test_gpu_one_sweep_quad.py uses against the six-launch loop: 1e-12 of the scale on the coefficients and the basis, over the whole
run where it lies inside the prefix the arithmetic determines (n <= 22) and over the first 20 steps at n = 130.  One group through
lz_os_step holds the chain's scalars b_t = sqrt(sum of the ||z_t||^2 partials) and a_t = (sum of the z_t . A z_t partials) / ||z_t||^2 to the
longdouble reference's own bounds (tests/one_sweep_reference.py, group_step: error / bound <= 1), a second run gives the same bits, and
the padding of rows j .. j+3 is zero.  Whole runs take the plain 33 x 31 grid of tests/test_gpu_one_sweep_quad.py.  (Measured once on the
perturbed grid values_33x31 instead: the unscaled chain's relation residual is 2.2e-16 .. 4.2e-16 at n = 10 .. 22, the scaled chain's -
the form before this one - 4.0e-16 .. 8.7e-16, which at n = 12 and 22 is above four times the six-launch loop's 1.7e-16 / 1.9e-16 on
that input; eps times the scale is 8.9e-16 there.)

Part B, the side stream (TUNE_LOOP 10: the second-stage sums, post and the chat prediction beside the closing product and the next chain,
13: on the main stream): overlap changes no arithmetic, so everything is numpy.array_equal - alpha, beta, the basis and the residual of
whole runs with the counters of the path that ran, and G, H, chat, elog, the second-stage sums, the flags and the rows of one group read
back at once behind lz_os_step.  (lz_os_state_get reads the state of a step, not of a run: a run's G, H and elog are covered through the
bits of everything computed from them - every later coefficient and row.)"""
import functools

import numpy as np
import pytest

import lanczos_invariants as inv
import one_sweep_reference as R
from lanczos_amd import _capi, synthetic
from one_sweep_reference import matrix, state

pytestmark = pytest.mark.gpu

SIX, SINGLE, QUAD, SCALED, MAIN = 1, 6, 10, 12, 13  # (12: groups with the scaled chain, 13: groups without the side stream)
L33, G33, V5, V7, ASYM = "lap2d_33x31", "values_33x31", "values_48x40", "values7_13x12x11", "asym_48x40"
LONG = "values_1024x513"  # 525 312 rows: 1026 units of 512 rows, more alpha partials than the finishing block's 1024 threads


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name == L33:  # the 33 x 31 grid of tests/test_gpu_one_sweep_quad.py: 1023 rows, a padded last position
        return synthetic.laplacian_2d_5pt(33, 31).to_scipy()
    return inv.long_matrix(name) if name == ASYM else matrix(name)


def _handle(hip, name, loop):
    A = _matrix(name).tocsr()
    h = hip.Handle(0)
    h.set_options(hip.FLAG_FUSED_NORM)
    if loop:
        h.set_tuning(_capi.TUNE_LOOP, loop)
    h.set_csr(A.shape[0], 0, A.indptr, A.indices, A.data)
    return h


def _start(name):
    v0 = synthetic.reference_start_vector(_matrix(name).shape[0])
    return v0 / np.linalg.norm(v0)


def _run_fresh(hip, name, n, loop):
    h = _handle(hip, name, loop)
    a, b = h.run(n, _start(name))
    out = dict(a=np.array(a), b=np.array(b), V=h.get_basis(), r=h.get_residual(), engine=h.last_engine(), trips=h.last_gate_trips(),
               fused=h.last_one_sweep_fused(), pairs=h.last_one_sweep_pairs(), abandoned=h.last_pair_abandoned(),
               quads=h.last_one_sweep_quads(), quad_abandoned=h.last_quad_abandoned())
    h.close()
    return out


_runs = {}


def _run(hip, name, n, loop):
    """one run per (input, n, loop), shared by the tests and left unchanged"""
    key = (name, n, loop)
    if key not in _runs:
        _runs[key] = _run_fresh(hip, name, n, loop)
    return _runs[key]


@functools.lru_cache(maxsize=None)
def _dense_spectrum(name):
    return np.linalg.eigvalsh(_matrix(name).toarray())


def _assert_ran_groups(got, n):
    assert got["engine"] == "one-sweep" and got["fused"] == 1
    assert got["quads"] == (n - 2) // 4 and got["pairs"] == (1 if (n - 2) % 4 == 2 else 0)
    assert got["quad_abandoned"] == 0 and got["abandoned"] == 0 and got["trips"] == 0


def _same_run(x, y):
    return all(np.array_equal(x[k], y[k]) for k in ("a", "b", "V", "r")) and all(
        x[k] == y[k] for k in ("engine", "trips", "fused", "pairs", "abandoned", "quads", "quad_abandoned"))


# ------------------------------------------------------------------------------------------------------------------ part A, whole runs
# the 33 x 31 grid has 1023 rows (a padded last position); n = 22: groups at j = 2 .. 18; n = 130 (j > 64): the second trips of the post
# kernel's sums; n = 10 .. 13: two groups and a tail of 0, 1, 2 and 3 steps; seven-point rows take the other coded product; LONG: the
# strided loop of the two-sum kernel over more partials than it has threads
@pytest.mark.parametrize("name,n", [(L33, 22), (L33, 130), (L33, 10), (L33, 11), (L33, 12), (L33, 13), (V7, 22), (LONG, 10)])
def test_unscaled_chain_against_the_scaled_chain(hip, name, n):
    ref = _run(hip, name, n, SIX)
    new, old = _run(hip, name, n, QUAD), _run(hip, name, n, SCALED)
    assert ref["engine"] == "kernels" and ref["quads"] == 0 and ref["pairs"] == 0
    A = _matrix(name)
    # (LONG has no dense spectrum to take: only the scale is needed below 258 steps - the largest Ritz value of the six-launch run)
    spec = _dense_spectrum(name) if A.shape[0] <= 4096 else np.array([np.abs(np.linalg.eigvalsh(
        np.diag(ref["a"]) + np.diag(ref["b"][: n - 1], 1) + np.diag(ref["b"][: n - 1], -1))).max()])
    for run in (ref, new, old):
        if "inv" not in run:
            run["inv"] = inv.invariants(A, run["a"], run["b"], run["V"], run["r"], spec)
    scale = ref["inv"]["scale"]
    k = n if n <= 22 else 20
    for got, what in ((new, "unscaled chain"), (old, "scaled chain")):
        _assert_ran_groups(got, n)
        print(f"\n[{name} n = {n} {what}] groups {got['quads']} pairs {got['pairs']}; {inv.describe(got['inv'])}; six-launch rel {ref['inv']['rel']:.1e}")
        inv.assert_invariants(got["inv"], ref["inv"]["rel"], f"{name} n = {n} {what}")
    for other, what in ((old, "scaled chain"), (ref, "six-launch")):
        da, db = np.abs(new["a"] - other["a"])[:k].max(), np.abs(new["b"] - other["b"])[: k - 1].max()
        dV = np.abs(new["V"] - other["V"])[:k].max()
        print(f"[{name} n = {n} unscaled chain vs {what}, first {k}] |dalpha| {da:.1e}, |dbeta| {db:.1e}, |dV| {dV:.1e} (scale {scale:.2f})")
        assert da <= inv.COEF_BAR * scale and db <= inv.COEF_BAR * scale and dV <= inv.COEF_BAR * scale


# -------------------------------------------------------------------------------------------------------------- one group, lz_os_step
def _group(hip, name, j, n, loop=0, h=None):
    """tests/test_gpu_one_sweep_step.py's run_group: the state of ``one_sweep_reference.state`` with NaN in every row the step may write"""
    st = state(name, j, n, "skew")
    own = h is None
    h = _handle(hip, name, loop) if own else h
    h.basis_alloc(n)
    h.basis_set_rows(0, st["V"])
    h.basis_set_rows(j, np.full((n - j, st["V"].shape[1]), np.nan))
    h.step_spmv(j - 1)
    h.os_state_set(j, st["G"], st["H"], st["chat"], st["alpha_prev"], st["beta_prev"], st["beta_prev2"])
    nb = h.os_step(4, j, False)
    dev = h.os_state_get(4, j)  # (at once behind the step: nothing in between waits for the side stream)
    dev["rows"] = np.stack([h.basis_get_row(j + t) for t in range(4)])
    dev["y"] = h.r_get()
    dev["raw"], _ = h.os_raw_get(j, 4, nb * 4 * dev["ldp"])
    if own:
        h.close()
    return st, dev


STATE_KEYS = ("G", "H", "chat", "gq", "d", "elog", "alpha", "beta", "nrm2", "ist", "rows", "y", "raw")


def _same_state(x, y):
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in STATE_KEYS)


@pytest.mark.parametrize("name,j,n", [(G33, 5, 10), (V5, 70, 75), (V7, 9, 14)])
def test_chain_scalars_against_longdouble_and_zero_padding(hip, name, j, n):
    A = matrix(name)
    rows = A.shape[0]
    h = _handle(hip, name, 0)
    st, dev = _group(hip, name, j, n, h=h)
    _, again = _group(hip, name, j, n, h=h)
    h.close()
    a, b = dev["alpha"][j : j + 3], dev["beta"][j - 1 : j + 3]
    out = R.group_step(A, st, given={"a": a, "b": b})
    worst = lambda ref, got: float(np.max(np.abs(ref.v - np.asarray(got)) / ref.e))  # noqa: E731
    qa, qb, qn = worst(R.cat(out["a"]), a), worst(R.cat(out["b"]), b), worst(out["nrm2"], dev["nrm2"][0])
    print(f"\n[{name} j = {j} n = {n}] error / bound: a {qa:.2e} b {qb:.2e} ||z_3||^2 {qn:.2e}; flags {list(dev['ist'][:5])}")
    assert qa <= 1.0 and qb <= 1.0 and qn <= 1.0
    assert dev["ist"][4] == out["flag"]  # (a skew state: every leftover is far above the gate, so the reference's decision is 1)
    assert np.array_equal(dev["raw"][:, :rows], dev["rows"]) and not dev["raw"][:, rows:].any(), "the padding of rows j .. j+3 is not zero"
    assert _same_state(dev, again), "a second group on the same handle gives other bits"


# ------------------------------------------------------------------------------------------------------------------ part B, whole runs
# n = 130 ends on a group (post is long there - j up to 126 - while a chain on 1023 rows is a few microseconds: a missing wait would
# race), n = 24 on a pair, n = 23 on a single step, n = 25 on three of them
@pytest.mark.parametrize("name,n", [(L33, 130), (L33, 24), (L33, 23), (L33, 25), (V7, 22)])
def test_side_stream_changes_no_bit_of_a_run(hip, name, n):
    side, main = _run(hip, name, n, QUAD), _run(hip, name, n, MAIN)
    _assert_ran_groups(side, n)
    _assert_ran_groups(main, n)
    assert _same_run(side, main)
    assert _same_run(side, _run_fresh(hip, name, n, QUAD)), "a second run with the side stream gives other bits"


def test_side_stream_and_the_abandon_chain(hip):
    # the asymmetric operator: the groups' leftovers are ~1e-9, the run is repeated on the pair form and then on the single fused form
    n = 130
    one = _run(hip, ASYM, n, SINGLE)
    side, main = _run(hip, ASYM, n, QUAD), _run(hip, ASYM, n, MAIN)
    for got in (side, main):
        assert got["engine"] == "one-sweep" and got["fused"] == 1
        assert got["quad_abandoned"] == 1 and got["abandoned"] == 1 and got["quads"] == 0 and got["pairs"] == 0
    assert _same_run(side, main)
    assert np.array_equal(side["a"], one["a"]) and np.array_equal(side["b"], one["b"]) and np.array_equal(side["V"], one["V"])


@pytest.mark.parametrize("name,j,n", [(G33, 5, 10), (V5, 126, 130), (V5, 300, 305)])
def test_side_stream_state_read_back_at_once(hip, name, j, n):
    """lz_os_step form 4 followed at once by lz_os_state_get: j + 4 == n predicts nothing, j + 4 < n runs the chat prediction as well"""
    _, side = _group(hip, name, j, n)
    _, main = _group(hip, name, j, n, MAIN)
    assert _same_state(side, main)
    _, again = _group(hip, name, j, n)
    assert _same_state(side, again)
