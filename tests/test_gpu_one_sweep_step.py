"""One loop body of the one-sweep loop on the device, on a state set from the host, against longdouble (tests/one_sweep_reference.py).

lz_os_state_set / lz_os_step / lz_os_state_get run exactly the function lz_run's loop calls for one single step, one pair or one group
of four steps (one_sweep_fused_iter, one_sweep_pair_iter, one_sweep_quad_iter; for a group: the chain, k_os_quad_predict, k_os_quad_sweep, k_os_quad_post, the closing SpMV and k_os_sum_predict) on a basis
and a state in which every term of those kernels is O(1e-3) (``skew``), not the O(eps) of a Lanczos run, and hand back everything the
kernels keep on the device.  Every value is held to ``error / bound <= 1`` with the reference's derived bounds, stage by stage: a
stage's reference is evaluated on the device's own inputs to that stage, so the bounds do not compound.  The ratios are printed.
tests/test_one_sweep_step_host.py shows on the CPU that a dropped or mis-indexed term is at least a hundred bounds away.

Every case also asserts: the flag ints equal the reference's decision, rows below ``j`` and the entries of ``G`` and ``H`` outside the
columns the step owns are bit-unchanged, the padding of the written rows is zero (lz_os_raw_get), unused slots of the predictions, of
the second-stage sums and of the pair and group walks' partial sums are zero, the partial sums add up to the second-stage sums, and the
block count of the walk is the one of the intended ``<P, RU>`` instantiation.  A NaN in any ratio fails the case.
"""
import math

import numpy as np
import pytest
import one_sweep_reference as R
from arnoldi_reference import padded, worst
from one_sweep_reference import matrix, state

pytestmark = pytest.mark.gpu

TPB, NUM_CU = 256, 256  # kTPB, kNumCU (lz_internal.h)


def sweep_p(rows):
    """os_sweep_p: positions per lane of the single walk for this many rows"""
    n2 = padded(rows) // 2
    if n2 <= 16384:
        return 1
    bal = {}
    for cand in (16, 8, 4, 2):
        g = -(-n2 // (TPB * cand)) / NUM_CU
        bal[cand] = g / math.ceil(g)
        if bal[cand] >= 0.93:
            return cand
    return max(bal, key=lambda c: (bal[c], c))


def group_p(rows, wide):
    p = sweep_p(rows)
    return (8 if wide else 4) if p >= 8 else p


def blocks(rows, p):
    return -(-(padded(rows) // 2) // (TPB * p))


def open_handle(hip, name):
    A = matrix(name)
    h = hip.Handle(0)
    h.set_options(hip.FLAG_FUSED_NORM)
    h.set_csr(A.shape[0], 0, A.indptr, A.indices, A.data)
    return h


def upload(h, st):
    """steps 2 - 5 of a case, up to the state: the basis with NaN in every row the step may write, y = A V[j-1], the state"""
    j, n = st["j"], st["n"]
    h.basis_alloc(n)
    h.basis_set_rows(0, st["V"])
    h.basis_set_rows(j, np.full((n - j, st["V"].shape[1]), np.nan))
    h.step_spmv(j - 1)
    h.os_state_set(j, st["G"], st["H"], st["chat"], st["alpha_prev"], st["beta_prev"], st["beta_prev2"])


def run_group(h, st, wide=False):
    j, n = st["j"], st["n"]
    upload(h, st)
    y0 = h.r_get()
    nb = h.os_step(4, j, wide)
    dev = h.os_state_get(4, j)
    dev["rows_old"] = np.stack([h.basis_get_row(i) for i in range(j)])
    dev["rows"] = [h.basis_get_row(j + t) for t in range(4)]
    dev["y0"], dev["y"], dev["blocks"] = y0, h.r_get(), nb
    return dev


def group_given(dev, j):
    ldp = dev["ldp"]
    return {"a": dev["alpha"][j : j + 3], "b": dev["beta"][j - 1 : j + 3], "g": [dev["gq"][t, : j + 4] for t in range(4)],
            "D": [dev["d"][t * ldp : t * ldp + j + 4] for t in range(4)], "v_last": dev["rows"][3], "alpha_last": dev["alpha"][j + 3]}


def ratio(ref, got):
    return worst(np.abs(ref.v - np.asarray(got)), ref.e)


def check_group(name, st, dev, wide=False):
    """everything one group leaves, against the reference evaluated on the device's own stage inputs"""
    A = matrix(name)
    j, n, kind = st["j"], st["n"], st["kind"]
    rows = A.shape[0]
    k = j + 4
    given = group_given(dev, j)
    assert dev["ldg"] == n + 4 and dev["ldp"] == (j + 4 + 15) // 16 * 16
    assert dev["blocks"] == blocks(rows, group_p(rows, wide))
    assert np.array_equal(dev["rows_old"], st["V"]), "a row below j changed"
    ist = dev["ist"]
    if kind == "nan":  # NaN arithmetic, no fault: the leftover is infinity and the group is flagged
        assert ist[4] == 1 and ist[3] == 0 and ist[0] == 0 and ist[1] == 0
        assert np.all(np.isinf(dev["elog"][j:k]))
        return {}
    out = R.group_step(A, st, given=given)
    q = {"y0": ratio(out["y0"], dev["y0"]), "a": ratio(R.cat(out["a"]), given["a"]), "b": ratio(R.cat(out["b"]), given["b"]),
         "nrm2": ratio(out["nrm2"], dev["nrm2"][0]), "g": ratio(R.cat(out["g"]), np.concatenate(given["g"])),
         "D": ratio(R.cat(out["D"]), np.concatenate(given["D"])), "rows": ratio(R.cat(out["rows"]), np.concatenate(dev["rows"]))}
    G, H = out["G"], out["H"]
    q["G"] = max(ratio(G[:, j:k], dev["G"][:, j:k]), ratio(G[j:k, :], dev["G"][j:k, :]))
    q["H"] = ratio(H[:, j - 1 : k - 1], dev["H"][:, j - 1 : k - 1])
    q["elog"] = max(ratio(out["elog"], dev["elog"][j + t]) for t in range(4))
    q["y"] = ratio(out["y"], dev["y"])
    q["alpha_last"] = ratio(out["alpha_last"], dev["alpha"][k - 1])
    hcols = k - 1  # the columns of H the step owns end here ...
    if k < n:      # ... or one further: the closing writes column j + 3 and the next chat
        q["chat"] = ratio(out["chat_next"], dev["chat"][:k])
        q["H_last"] = ratio(H[:, k - 1], dev["H"][:, k - 1])
        hcols = k
    print(f"\n[group {name} {kind} j = {j} n = {n} wide {int(wide)}] blocks {dev['blocks']} flags {list(ist[:5])} "
          + " ".join(f"{key} {val:.2e}" for key, val in q.items()))
    assert all(v <= 1.0 for v in q.values()), q  # (a NaN fails: max() would drop it)
    # decisions, and what a group must leave alone
    assert ist[4] == out["flag"] and ist[3] == 0 and ist[0] == 0 and ist[1] == 0 and ist[2] == 0
    assert np.array_equal(dev["G"][:j, :j], st["G"][:j, :j]) and not dev["G"][k:, :].any() and not dev["G"][:, k:].any()
    assert np.array_equal(dev["H"][:, : j - 1], st["H"][:, : j - 1]) and not dev["H"][:, hcols:].any()
    for t in range(4):
        assert not dev["gq"][t, j + t :].any(), "a prediction slot behind its run is not zero"
        run = dev["d"][t * dev["ldp"] : (t + 1) * dev["ldp"]] if t < 3 else dev["d"][3 * dev["ldp"] : 3 * dev["ldp"] + j + 4]
        assert not run[j + t + 1 :].any(), "an unused slot of the second-stage sums is not zero"
    return q


_handles = {}


def handle_for(hip, name):
    """one handle per input, reused by every case on it (a reused handle is part of what is tested) and closed with the module"""
    if name not in _handles:
        _handles[name] = open_handle(hip, name)
    return _handles[name]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def check_raw(h, st, dev, width, runs, used):
    """what only a raw read shows: the padding of the written rows is zero, the walk's partial sums add up to the second-stage sums, and
    the slots of a run behind ``used(t)`` entries left the walk as zeros (``used`` None: the single walk writes no more than it uses)"""
    j, rows, ldp, nb = st["j"], st["V"].shape[1], dev["ldp"], dev["blocks"]
    raw, part = h.os_raw_get(j, width, nb * runs * ldp)
    assert raw.shape[1] == padded(rows)
    for t in range(width):
        assert np.array_equal(raw[t, :rows], dev["rows"][t], equal_nan=True)
    assert not raw[:, rows:].any(), "the padding of a written row is not zero"
    part = part.reshape(nb, runs, ldp)
    for t in range(runs):
        m = used(t) if used else j + 2
        total = R.B(part[:, t, :m].astype(R.LD).sum(axis=0), nb * R.EPS * np.abs(part[:, t, :m]).sum(axis=0))
        assert ratio(total, dev["d"][t * ldp : t * ldp + m]) <= 1.0, "the second-stage sums are not the sums of the walk's partials"
        if used:
            assert not part[:, t, m:].any(), "an unused slot of the walk's partial sums is not zero"


def group_case(hip, name, j, n, kind, wide=False, amp=1e-3):
    st = state(name, j, n, kind, amp=amp)
    h = handle_for(hip, name)
    dev = run_group(h, st, wide)
    q = check_group(name, st, dev, wide)
    if kind != "nan":
        check_raw(h, st, dev, 4, 4, lambda t: j + t + 1)
        assert not dev["g"].any(), "a group wrote into the pair's prediction buffers"
    return q


# ---------------------------------------------------------------------------------------------------------------- the group's walk
V5, V7 = "values_48x40", "values7_13x12x11"  # 1920 and 1716 rows


@pytest.mark.parametrize("name,p,wide", [("values_48x40", 1, False), ("values_200x165", 2, False), ("values_512x513", 4, False),
                                         ("values_1024x770", 8, True), ("values_1024x770", 4, False)])
def test_group_walk_instantiations(hip, name, p, wide):
    """<1,4>, <2,4>, <4,2> and <8,1>: j = 5 is a full trip and a ragged one at four rows a trip, an odd count at two"""
    rows = matrix(name).shape[0]
    assert group_p(rows, wide) == p, "this grid does not select the intended instantiation"
    group_case(hip, name, 5, 10, "skew", wide)


@pytest.mark.parametrize("j", [2, 3, 4, 6, 7, 12, 13])
def test_group_trip_edges(hip, j):
    """the trip edges of <1,4>, and the run lengths ldp = 16 (j = 12) and 32 (j = 13)"""
    group_case(hip, V5, j, j + 5, "skew")


def test_group_clamped_last_position(hip):
    """1023 rows: 512 double2 positions, the last one half padding"""
    group_case(hip, "values_33x31", 5, 10, "skew")


# ------------------------------------------------------------------------------------------------------ predict and post, one block
@pytest.mark.parametrize("j,n", [(63, 68), (64, 69), (65, 70), (129, 134), (300, 305), (508, 512)])
def test_group_predict_post_sizes(hip, j, n):
    """the second trip of os_wave_dots (j = 65), the mu chunks 16, 8, 5, 3, 2 of the post kernel, and the last step a group may start at"""
    group_case(hip, V5, j, n, "skew")


# --------------------------------------------------------------------------------------------------------------------------- kinds
@pytest.mark.parametrize("j", [6, 70])
@pytest.mark.parametrize("kind", ["orth", "miss", "nan"])
def test_group_kinds(hip, kind, j):
    group_case(hip, V5, j, j + 5, kind)


def test_group_seven_point(hip):
    group_case(hip, V7, 9, 14, "skew")


def test_group_last_group_of_a_run(hip):
    """j + 4 == n: the closing SpMV sums alpha and predicts nothing"""
    group_case(hip, V5, 6, 10, "skew")


# --------------------------------------------------------------------------------------------------------------------------- reuse
def _bits(dev):
    return [dev[key] for key in ("G", "H", "chat", "gq", "d", "elog", "alpha", "beta", "nrm2", "y")] + dev["rows"]


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(_bits(a), _bits(b)))


def test_group_fresh_handles_and_reuse_give_the_same_bits(hip):
    """two fresh handles agree, and a handle that ran n = 512, then n = 12, then n = 512 again gives the first answer: nothing stale in the
    state, the predictions or the partials"""
    big, small = state(V5, 300, 512, "skew"), state(V5, 7, 12, "skew")
    h1, h2 = open_handle(hip, V5), open_handle(hip, V5)
    first = run_group(h1, big)
    assert _same(first, run_group(h2, big))
    h2.close()
    small1 = run_group(h1, small)
    again = run_group(h1, big)
    assert _same(first, again)
    assert _same(small1, run_group(h1, small))
    h1.close()


def test_refused_calls_leave_everything_alone(hip):
    from test_gpu_kernels import layered_stencil27

    A = matrix(V5)
    st = state(V5, 6, 12, "skew")
    h = open_handle(hip, V5)
    h.set_tuning(hip.TUNE_LOOP, 10)  # lz_run on the group loop: it shares the state buffers with the step entries
    v0 = np.random.default_rng(3).standard_normal(A.shape[0])
    v0 /= np.linalg.norm(v0)
    a0, b0 = (np.array(x) for x in h.run(12, v0))
    first = run_group(h, st)
    for bad in (lambda: h.os_step(4, 1), lambda: h.os_step(4, 9), lambda: h.os_step(2, 11), lambda: h.os_step(3, 6),
                lambda: h.os_state_set(1, st["G"], st["H"], st["chat"][:1], 0.0, 0.0)):
        with pytest.raises(Exception) as err:
            bad()
        assert "one-sweep step" in str(err.value)
    after = h.os_state_get(4, 6)
    h.basis_alloc(12)  # a new basis: the state set for the old one no longer counts
    with pytest.raises(Exception) as err:
        h.os_step(4, 6)
    assert "no state set" in str(err.value)
    assert all(np.array_equal(first[key], after[key], equal_nan=True) for key in ("G", "H", "chat", "gq", "d", "elog", "alpha", "beta"))
    a1, b1 = (np.array(x) for x in h.run(12, v0))
    assert np.array_equal(a0, a1) and np.array_equal(b0, b1)
    assert h.last_one_sweep_quads() == 2
    h.close()
    # a 27-point matrix has no fused one-sweep form: the state setter refuses before it touches anything
    S = layered_stencil27(symmetric=True)[0].tocsr()
    h = hip.Handle(0)
    h.set_options(hip.FLAG_FUSED_NORM)
    h.set_csr(S.shape[0], 0, S.indptr, S.indices, S.data)
    h.basis_alloc(12)
    with pytest.raises(Exception) as err:
        h.os_state_set(6, st["G"], st["H"], st["chat"], 0.0, 0.0)
    assert "one-sweep step" in str(err.value)
    h.close()


# ================================================================================================================ the pair form
def pair_p(rows, wide):
    p = sweep_p(rows)
    return (16 if wide else 8) if p >= 8 else p


def run_step(h, st, form, width, wide=False):
    j = st["j"]
    upload(h, st)
    y0 = h.r_get()
    nb = h.os_step(form, j, wide)
    dev = h.os_state_get(form, j)
    dev["rows_old"] = np.stack([h.basis_get_row(i) for i in range(j)])
    dev["rows"] = [h.basis_get_row(j + t) for t in range(width)]
    dev["y0"], dev["y"], dev["blocks"] = y0, h.r_get(), nb
    return dev


def check_common(st, dev, out, q, width, flag_slot, flag):
    """the closing of a step that made ``width`` rows, the decision, and what the step must leave alone"""
    j, n = st["j"], st["n"]
    k = j + width
    G, H = out["G"], out["H"]
    q["rows"] = ratio(R.cat(out["rows"]), np.concatenate(dev["rows"]))
    q["G"] = max(ratio(G[:, j:k], dev["G"][:, j:k]), ratio(G[j:k, :], dev["G"][j:k, :]))
    q["H"] = ratio(H[:, j - 1 : k - 1], dev["H"][:, j - 1 : k - 1])
    q["y"] = ratio(out["y"], dev["y"])
    q["alpha_last"] = ratio(out["alpha_last"], dev["alpha"][k - 1])
    hcols = k - 1
    if k < n:
        q["chat"] = ratio(out["chat_next"], dev["chat"][:k])
        q["H_last"] = ratio(H[:, k - 1], dev["H"][:, k - 1])
        hcols = k
    print(f"\n[{st['kind']} j = {j} n = {n}] blocks {dev['blocks']} flags {[int(x) for x in dev['ist'][:5]]} " + " ".join(f"{key} {val:.2e}" for key, val in q.items()))
    assert all(v <= 1.0 for v in q.values()), q  # (a NaN fails: max() would drop it)
    want = [0] * 5
    want[flag_slot] = flag
    if flag_slot == 0:
        want[1] = flag  # (the trips of the run so far)
    assert [int(x) for x in dev["ist"][:5]] == want
    assert np.array_equal(dev["G"][:j, :j], st["G"][:j, :j]) and not dev["G"][k:, :].any() and not dev["G"][:, k:].any()
    assert np.array_equal(dev["H"][:, : j - 1], st["H"][:, : j - 1]) and not dev["H"][:, hcols:].any()


def pair_case(hip, name, j, n, kind, wide=False):
    A, st = matrix(name), state(name, j, n, kind)
    dev = run_step(handle_for(hip, name), st, 2, 2, wide)
    rows, ldp = A.shape[0], dev["ldp"]
    assert ldp == (j + 2 + 15) // 16 * 16 and dev["blocks"] == blocks(rows, pair_p(rows, wide))
    assert np.array_equal(dev["rows_old"], st["V"]), "a row below j changed"
    if kind == "nan":
        assert dev["ist"][3] == 1 and dev["ist"][4] == 0 and np.isinf(dev["elog"][j])
        return
    given = {"a0": dev["alpha"][j], "b": dev["beta"][j - 1], "kap": dev["g"][: j + 1], "p": dev["g"][n + 1 : n + j + 2], "d1": dev["d"][: j + 1],
             "d2": dev["d"][ldp : ldp + j + 2], "u2": dev["r2"], "v_last": dev["rows"][1], "alpha_last": dev["alpha"][j + 1]}
    out = R.pair_step(A, st, given=given)
    q = {"y0": ratio(out["y0"], dev["y0"])}
    for key in ("a0", "b", "kap", "p", "d1", "d2", "u2"):
        q[key] = ratio(out[key], given[key])
    q["b2"] = ratio(out["b2"], dev["beta"][j])
    q["nrm2"] = ratio(out["nrm2"], dev["nrm2"][0])
    q["elog"] = max(ratio(out["e1"], dev["elog"][j]), ratio(out["e2"], dev["elog"][j + 1]))
    print(f"\n[pair {name} wide {int(wide)}]", end="")
    check_common(st, dev, out, q, 2, 3, out["flag"])
    assert not dev["d"][j + 1 : ldp].any() and not dev["d"][ldp + j + 2 : 2 * ldp].any(), "an unused slot of the second-stage sums is not zero"
    assert not dev["g"][j + 1 : n + 1].any() and not dev["g"][n + j + 2 :].any(), "an unused slot of kap / p is not zero"
    check_raw(handle_for(hip, name), st, dev, 2, 2, lambda t: j + 1 + t)


def single_case(hip, name, j, n, kind):
    A, st = matrix(name), state(name, j, n, kind)
    dev = run_step(handle_for(hip, name), st, 1, 1)
    rows = A.shape[0]
    assert dev["blocks"] == blocks(rows, sweep_p(rows))
    assert np.array_equal(dev["rows_old"], st["V"]), "a row below j changed"
    if kind == "nan":  # the gate opens on a NaN leftover; the correction then runs on NaN: arithmetic, no fault
        assert dev["ist"][0] == 1 and dev["ist"][1] == 1 and np.isinf(dev["elog"][j])
        return
    given = {"d": dev["d"][: j + 2], "v_last": dev["rows"][0], "alpha_last": dev["alpha"][j]}
    if dev["ist"][0]:
        given["gcorr"] = dev["g"][:j]
    out = R.single_step(A, st, given=given)
    assert out["trip"] == int(kind == "miss") == int(dev["ist"][0])
    q = {"y0": ratio(out["y0"], dev["y0"]), "d": ratio(out["d"], given["d"]), "u": ratio(out["u"], dev["r2"]), "b": ratio(out["b"], dev["beta"][j - 1]),
         "nrm2": ratio(out["nrm2"], dev["nrm2"][0]), "elog": ratio(out["elog"], dev["elog"][j])}
    if out["trip"]:
        q["gcorr"] = ratio(out["gcorr"], dev["g"][:j])
        q["gcorr_u"] = ratio(out["gcorr_u"], dev["g"][n : n + j])
    print(f"\n[single {name}]", end="")
    check_common(st, dev, out, q, 1, 0, out["trip"])
    assert not dev["d"][j + 2 : dev["ldp"]].any(), "an unused slot of the second-stage sums is not zero"
    if out["trip"]:
        assert not dev["g"][j:n].any() and not dev["g"][n + j :].any(), "a slot behind the correction's coefficients is not zero"
    else:
        assert not dev["g"].any(), "a step whose gate stayed shut wrote correction coefficients"
    check_raw(handle_for(hip, name), st, dev, 1, 1, None)


@pytest.mark.parametrize("name,p,wide", [("values_48x40", 1, False), ("values_200x165", 2, False), ("values_512x513", 4, False),
                                         ("values_1024x770", 8, False), ("values_1024x770", 16, True)])
def test_pair_walk_instantiations(hip, name, p, wide):
    """<1,8>, <2,4>, <4,2>, <8,1> and <16,1>"""
    assert pair_p(matrix(name).shape[0], wide) == p, "this grid does not select the intended instantiation"
    pair_case(hip, name, 5, 10, "skew", wide)


@pytest.mark.parametrize("j", [2, 3, 14, 15])
def test_pair_trip_edges(hip, j):
    pair_case(hip, V5, j, j + 3, "skew")


@pytest.mark.parametrize("j,n", [(64, 67), (65, 68), (129, 132), (258, 261), (515, 518), (1006, 1009), (1021, 1023)])
def test_pair_predict_post_sizes(hip, j, n):
    """the mu chunks 16, 8, 5, 3, 1 of k_os_pair_predict and the pair walk's 64 KiB of LDS (j = 1021: the last pair of the longest run)"""
    pair_case(hip, V5, j, n, "skew")


@pytest.mark.parametrize("j", [6, 70])
@pytest.mark.parametrize("kind", ["orth", "miss", "nan"])
def test_pair_kinds(hip, kind, j):
    pair_case(hip, V5, j, j + 3, kind)


def test_pair_seven_point(hip):
    pair_case(hip, V7, 9, 12, "skew")


# ============================================================================================================= the single fused form
@pytest.mark.parametrize("j", [5, 70])
@pytest.mark.parametrize("kind", ["orth", "skew", "miss", "nan"])
def test_single_kinds(hip, kind, j):
    """``miss``: the gate opens, and the corrected row, the corrected column of G and H[:j, j-1] follow the reference with its correction;
    the trip is counted"""
    single_case(hip, V5, j, j + 3, kind)


def test_single_seven_point_and_two_positions_per_lane(hip):
    single_case(hip, V7, 9, 12, "miss")
    single_case(hip, "values_200x165", 5, 8, "miss")
