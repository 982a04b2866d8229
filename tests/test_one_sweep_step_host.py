"""The cases of tests/test_gpu_one_sweep_step.py made decisive before a GPU sees them (no GPU here).

``one_sweep_reference`` evaluates one loop body of the one-sweep loop in longdouble, with a bound for a float64 device on everything it
returns.  On a ``skew`` state (a basis from a recurrence with coefficients perturbed by ``amp``) this file asserts:

- the identities the kernels rest on: the leftover against the old rows is rounding, the new columns of ``G`` are the Gram matrix of the
  finished rows, the new columns of ``H`` satisfy ``A V_i = sum_l H[l, i] V_l`` - to the reference's own bounds, at ``amp`` 1e-3 and 3e-2;
- that every bound binds: the reference with one term removed or one index shifted (``MUTATIONS``) differs from the full one by at
  least 100 bounds of the quantity the term enters, at ``amp`` 1e-3, or where that does not reach the factor at up to 3e-2.  The bounds
  used are the forward ones (nothing given), the widest a device value is ever held to;
- that every decision is far from the gate: leftovers below ``tau / 10`` or above ``10 tau``, never in between;
- that the bounds are not too tight: the float64 prototypes (tools/one_sweep_group_prototype.py, on a float64 chain and walk) lie
  within them, forward and stage by stage.

One mutation the issue lists is an equivalent one and is not here: a predict sum one term *longer* than ``min(i + 2, j)`` reads
``H[i + 2, i]``, a structural zero of the Hessenberg ``H``, and changes nothing.
"""
import functools
import os
import sys

import numpy as np
import pytest
import one_sweep_reference as R
from arnoldi_reference import worst
from one_sweep_reference import matrix, state

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import one_sweep_group_prototype as gproto  # noqa: E402

FACTOR = 100.0
AMPS = (1e-3, 3e-2)


@functools.lru_cache(maxsize=None)
def group_ref(name, j, n, kind, amp=1e-3, mut=None):
    return R.group_step(matrix(name), state(name, j, n, kind, amp=amp), mut=mut)


HOST_CASES = [("values_24x20", 7, 12), ("values7_6x5x4", 5, 9), ("values_24x20", 12, 16)]


def gram_bound(rows):
    """the bound on ``rows_a . rows_b`` that follows from the rows' own bounds"""
    v = np.abs(np.stack([r.v for r in rows]))
    e = np.stack([r.e for r in rows])
    return v @ e.T + e @ v.T


def all_rows(st, out):
    return [R.B(r) for r in st["V"]] + list(out["rows"])


# ------------------------------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("amp", AMPS)
@pytest.mark.parametrize("name,j,n", HOST_CASES)
def test_group_identities(name, j, n, amp):
    A, st = matrix(name), state(name, j, n, "skew", amp=amp)
    out = group_ref(name, j, n, "skew", amp)
    k = j + 4
    assert float(out["e_old"].v) <= float(out["e_old"].e), "the leftover against the old rows is not rounding"
    rows = all_rows(st, out)
    Vx = np.stack([r.v for r in rows])
    gram = Vx @ Vx.T
    G = out["G"]
    r_g = worst(np.abs(G.v[:k, :k] - gram), G.e[:k, :k] + gram_bound(rows) + R.EPS * np.abs(gram))  # (the old block was rounded once)
    defect, bound = [], []
    H = out["H"]
    for i in range(k - 1):
        av = R.spmv(A, rows[i])
        comb = R.comb(H[:k, i], R.B(Vx, np.stack([r.e for r in rows])))
        defect.append(np.abs(av.v - comb.v))
        bound.append(av.e + comb.e)
    r_h = worst(np.stack(defect), np.stack(bound))
    print(f"{name} j={j} amp={amp:g}: e_old {float(out['e_old'].v):.1e} (bound {float(out['e_old'].e):.1e}), G vs Gram {r_g:.2e}, "
          f"A V - V H {r_h:.2e} of their bounds; max |G - Gram| {float(np.abs(G.v[:k, :k] - gram).max()):.1e}, "
          f"max |A V - V H| {float(np.max(defect)):.1e}")
    assert r_g <= 1.0 and r_h <= 1.0


# ------------------------------------------------------------------------------------------------------------------ every bound binds
def _g(out):
    return R.cat(out["g"])


def _rows(out):
    return R.cat(out["rows"])


def _G(out):
    return R.B(out["G"].v.ravel(), out["G"].e.ravel())


def _H(out):
    return R.B(out["H"].v.ravel(), out["H"].e.ravel())


GROUP_MUTATIONS = {  # name -> the quantity the term enters first
    "pred_b0": _g, "pred_b0_first": _g, "pred_bt_prev": _g, "pred_len_less": _g, "pred_up": _g, "pred_lo": _g, "pred_pv": _g,
    "walk_gi": _rows,
    "post_g_ingroup": _G, "post_g_triangle": _G,
    "post_h_b0c0": _H, "post_h_cjm1": _H, "post_h_chunk": _H, "post_h_start": _H,
}


def mutation_factor(ref, name, j, n, mut, pick):
    for amp in AMPS:
        full, bad = pick(ref(name, j, n, "skew", amp)), pick(ref(name, j, n, "skew", amp, mut))
        diff = np.abs(bad.v - full.v)
        k = int(np.argmax(np.where(full.e > 0, diff / np.where(full.e > 0, full.e, 1), 0)))
        factor = float(diff[k] / full.e[k]) if full.e[k] > 0 else 0.0
        if factor >= FACTOR:
            break
    return factor, amp


@pytest.mark.parametrize("mut", sorted(GROUP_MUTATIONS))
def test_group_mutation_is_seen(mut):
    name, j, n = HOST_CASES[0]
    factor, amp = mutation_factor(group_ref, name, j, n, mut, GROUP_MUTATIONS[mut])
    print(f"group {mut}: {factor:.3g} bounds away at amp {amp:g}")
    assert factor >= FACTOR


# ------------------------------------------------------------------------------------------------------- decisions far from the gate
@pytest.mark.parametrize("name,j,n", HOST_CASES)
def test_group_decisions_are_far_from_the_gate(name, j, n):
    for kind, tripped in (("orth", False), ("skew", True), ("miss", True)):
        out = group_ref(name, j, n, kind)
        for key in ("e_old", "e_in"):
            e = float(out[key].v)
            print(f"{name} j={j} {kind}: {key} = {e:.2e}")
            assert e < R.TAU / 10 or e > 10 * R.TAU, "a leftover sits at the gate"
        assert out["flag"] == int(tripped)
        if kind == "orth":
            assert max(float(out["e_old"].v), float(out["e_in"].v)) < R.TAU / 10
        if kind == "miss":
            assert float(out["e_old"].v) > 10 * R.TAU
    out = group_ref(name, j, n, "nan")
    assert out["flag"] == 1 and np.isinf(float(out["elog"].v))


# ---------------------------------------------------------------------------------------------- the float64 prototypes lie within
def float64_group(A, st):
    """one group in float64: the chain and the walk restated, predict and post tools/one_sweep_group_prototype.py's"""
    j, n, m = st["j"], st["n"], 4
    V, G, H, chat = st["V"], st["G"].copy(), st["H"].copy(), st["chat"]
    y = A @ V[j - 1]
    a, b, X = np.zeros(m), np.zeros(m), np.zeros((m, V.shape[1]))
    w = (y - st["alpha_prev"] * V[j - 1]) - st["beta_prev"] * V[j - 2]
    b[0] = np.sqrt(w @ w)
    X[0] = w / b[0]
    for t in range(m - 1):
        yt = A @ X[t]
        a[t] = X[t] @ yt
        z = (yt - a[t] * X[t]) - b[t] * (X[t - 1] if t else V[j - 1])
        b[t + 1] = np.sqrt(z @ z)
        X[t + 1] = z / b[t + 1]
    g = gproto.group_predict(G, H, chat, a, b, j, m)
    D = [V @ X[t] for t in range(m)]
    Vn, mm, vv = np.zeros((m, V.shape[1])), np.zeros((m, m)), np.zeros(m)
    for t in range(m):
        v = X[t] - g[t][:j] @ V
        for s in range(t):
            v = v - g[t][j + s] * Vn[s]
        Vn[t] = v
        for s in range(t):
            mm[s, t] = Vn[s] @ X[t]
        vv[t] = v @ v
    e_old, e_in = gproto.group_post(G, H, g, D, mm, vv, a, b, j, m, n)
    Dfull = [np.concatenate([D[t], mm[:t, t], [vv[t]], np.zeros(m - t - 1)]) for t in range(m)]
    gfull = [np.concatenate([g[t], np.zeros(m - t)]) for t in range(m)]
    y_last = A @ Vn[m - 1]
    return {"a": a[: m - 1], "b": b, "g": gfull, "D": Dfull, "rows": Vn, "G": G, "H": H, "e_old": e_old, "e_in": e_in,
            "v_last": Vn[m - 1], "alpha_last": float(Vn[m - 1] @ y_last), "y": y_last}


def group_errors(out, dev, j, n):
    """``error / bound`` of everything a float64 evaluation ``dev`` (a dict as float64_group returns) gives, against the reference ``out``"""
    k = j + 4
    q = {}
    q["a"] = worst(np.abs(np.array([x.v for x in out["a"]]) - dev["a"]), [x.e for x in out["a"]])
    q["b"] = worst(np.abs(np.array([x.v for x in out["b"]]) - dev["b"]), [x.e for x in out["b"]])
    for key in ("g", "D", "rows"):
        ref = R.cat(out[key])
        q[key] = worst(np.abs(ref.v - np.concatenate(dev[key])), ref.e)
    cols = slice(j, k)
    q["G"] = max(worst(np.abs(out["G"].v[:, cols] - dev["G"][:, cols]), out["G"].e[:, cols]),
                 worst(np.abs(out["G"].v[cols, :] - dev["G"][cols, :]), out["G"].e[cols, :]))
    hcols = slice(j - 1, k - 1)
    q["H"] = worst(np.abs(out["H"].v[:, hcols] - dev["H"][:, hcols]), out["H"].e[:, hcols])
    q["e_old"] = worst(abs(float(out["e_old"].v) - dev["e_old"]), out["e_old"].e)
    q["e_in"] = worst(abs(float(out["e_in"].v) - dev["e_in"]), out["e_in"].e)
    q["y"] = worst(np.abs(out["y"].v - dev["y"]), out["y"].e)
    q["alpha_last"] = worst(abs(float(out["alpha_last"].v) - dev["alpha_last"]), out["alpha_last"].e)
    return q


@pytest.mark.parametrize("kind", ["orth", "skew", "miss"])
@pytest.mark.parametrize("name,j,n", HOST_CASES)
def test_group_float64_prototype_within_bounds(name, j, n, kind):
    A, st = matrix(name), state(name, j, n, kind)
    dev = float64_group(A, st)
    forward = group_errors(group_ref(name, j, n, kind), dev, j, n)
    staged = group_errors(R.group_step(A, st, given=dev), dev, j, n)
    print(f"{name} j={j} {kind}: forward " + " ".join(f"{k}={v:.2e}" for k, v in forward.items()))
    print(f"{name} j={j} {kind}: staged  " + " ".join(f"{k}={v:.2e}" for k, v in staged.items()))
    assert all(v <= 1.0 for v in forward.values()) and all(v <= 1.0 for v in staged.values())  # (a NaN fails)


# ================================================================================================================ the pair form
@functools.lru_cache(maxsize=None)
def pair_ref(name, j, n, kind, amp=1e-3, mut=None):
    return R.pair_step(matrix(name), state(name, j, n, kind, amp=amp), mut=mut)


@functools.lru_cache(maxsize=None)
def single_ref(name, j, n, kind, amp=1e-3, mut=None):
    return R.single_step(matrix(name), state(name, j, n, kind, amp=amp), mut=mut)


def relation_ratio(A, rows, H, k):
    """``A V_i = sum_l H[l, i] V_l`` for ``i < k - 1`` over the ``k`` finished rows, in units of the bounds"""
    Vx = R.B(np.stack([r.v for r in rows]), np.stack([r.e for r in rows]))
    defect, bound = [], []
    for i in range(k - 1):
        av, cb = R.spmv(A, rows[i]), R.comb(H[:k, i], Vx)
        defect.append(np.abs(av.v - cb.v))
        bound.append(av.e + cb.e)
    return worst(np.stack(defect), np.stack(bound)), float(np.max(defect))


def gram_ratio(rows, G, k):
    Vx = np.stack([r.v for r in rows])
    gram = Vx @ Vx.T
    return worst(np.abs(G.v[:k, :k] - gram), G.e[:k, :k] + gram_bound(rows) + R.EPS * np.abs(gram)), float(np.abs(G.v[:k, :k] - gram).max())


@pytest.mark.parametrize("amp", AMPS)
@pytest.mark.parametrize("name,j,n", HOST_CASES)
def test_pair_identities(name, j, n, amp):
    """a pair normalises its second row by the measured norm and sets G[j+1, j+1] = 1: an identity to O(leftover^2) only, so the diagonal
    entry is compared on an orthonormal state (test_pair_decisions) and left out here"""
    A, st = matrix(name), state(name, j, n, "skew", amp=amp)
    out = pair_ref(name, j, n, "skew", amp)
    k = j + 2
    e1 = out["e1"]
    assert float(e1.v) <= float(e1.e), "the leftover against the old rows is not rounding"
    rows = all_rows(st, out)
    G = R.B(out["G"].v.copy(), out["G"].e.copy())
    G[j + 1, j + 1] = R.B(float(rows[j + 1].v @ rows[j + 1].v))
    r_g, d_g = gram_ratio(rows, G, k)
    r_h, d_h = relation_ratio(A, rows, out["H"], k)
    print(f"pair {name} j={j} amp={amp:g}: e1 {float(e1.v):.1e} (bound {float(e1.e):.1e}), G vs Gram {r_g:.2e} ({d_g:.1e}), A V - V H {r_h:.2e} ({d_h:.1e})")
    assert r_g <= 1.0 and r_h <= 1.0


@pytest.mark.parametrize("amp", AMPS)
@pytest.mark.parametrize("kind", ["skew", "miss"])
@pytest.mark.parametrize("name,j,n", HOST_CASES)
def test_single_identities(name, j, n, kind, amp):
    """``miss``: the gate opens, and the corrected row, the corrected column of G and the corrected column of H satisfy the same identities"""
    A, st = matrix(name), state(name, j, n, kind, amp=amp)
    out = single_ref(name, j, n, kind, amp)
    assert out["trip"] == int(kind == "miss")
    if kind == "skew":
        assert float(out["elog"].v) <= float(out["elog"].e), "the leftover against the old rows is not rounding"
    rows = all_rows(st, out)
    r_g, d_g = gram_ratio(rows, out["G"], j + 1)
    r_h, d_h = relation_ratio(A, rows, out["H"], j + 1)
    print(f"single {name} j={j} {kind} amp={amp:g}: leftover {float(out['elog'].v):.1e}, G vs Gram {r_g:.2e} ({d_g:.1e}), A V - V H {r_h:.2e} ({d_h:.1e})")
    assert r_g <= 1.0 and r_h <= 1.0


def _kp(out):
    return R.cat([out["kap"], out["p"]])


PAIR_MUTATIONS = {"pair_gp": _kp, "pair_q_b": _kp, "pair_mu_b": _kp, "mu_chunk": _kp, "mu_start": _kp, "pair_p_bg": _kp, "pair_kap_a0": _kp,
                  "pair_post_colj": _G, "pair_post_acc": _G, "pair_post_hb": _H}
SINGLE_MUTATIONS = {"single_vv": _G, "single_capp": _H}


@pytest.mark.parametrize("mut", sorted(PAIR_MUTATIONS))
def test_pair_mutation_is_seen(mut):
    name, j, n = HOST_CASES[0]
    factor, amp = mutation_factor(pair_ref, name, j, n, mut, PAIR_MUTATIONS[mut])
    print(f"pair {mut}: {factor:.3g} bounds away at amp {amp:g}")
    assert factor >= FACTOR


@pytest.mark.parametrize("mut", sorted(SINGLE_MUTATIONS))
def test_single_mutation_is_seen(mut):
    """the terms of the correction (the gate is open on a ``miss`` state)"""
    name, j, n = HOST_CASES[0]
    full, bad = single_ref(name, j, n, "miss"), single_ref(name, j, n, "miss", 1e-3, mut)
    a, b = SINGLE_MUTATIONS[mut](full), SINGLE_MUTATIONS[mut](bad)
    factor = worst(np.abs(a.v - b.v), np.where(a.e > 0, a.e, np.inf))
    print(f"single {mut}: {factor:.3g} bounds away")
    assert factor >= FACTOR


@pytest.mark.parametrize("name,j,n", HOST_CASES)
def test_pair_and_single_decisions_are_far_from_the_gate(name, j, n):
    for kind, tripped in (("orth", 0), ("skew", 1), ("miss", 1)):
        out = pair_ref(name, j, n, kind)
        for key in ("e1", "e2"):
            e = float(out[key].v)
            print(f"pair {name} j={j} {kind}: {key} = {e:.2e}")
            assert e < R.TAU / 10 or e > 10 * R.TAU, "a leftover sits at the gate"
        assert out["flag"] == tripped
        if kind == "orth":  # (and here the unit diagonal a pair writes is the Gram entry)
            v2 = out["rows"][1]
            assert abs(float(v2.v @ v2.v) - 1.0) <= float(gram_bound([v2])[0, 0]) + R.EPS
        if kind == "miss":
            assert float(out["e1"].v) > 10 * R.TAU
    for kind, tripped in (("orth", 0), ("skew", 0), ("miss", 1)):
        out = single_ref(name, j, n, kind)
        e = float(out["elog"].v)
        print(f"single {name} j={j} {kind}: leftover = {e:.2e}")
        assert (e < R.TAU / 10 or e > 10 * R.TAU) and out["trip"] == tripped
    assert pair_ref(name, j, n, "nan")["flag"] == 1 and np.isinf(float(pair_ref(name, j, n, "nan")["e1"].v))
    assert single_ref(name, j, n, "nan")["trip"] == 1 and np.isinf(float(single_ref(name, j, n, "nan")["elog"].v))


# ---- the float64 bodies of tools/one_sweep_prototype.py (one_sweep_pair_lanczos / one_sweep_fused_lanczos keep them inside their loops)
def float64_pair(A, st):
    j, n = st["j"], st["n"]
    V, G, Hm, chat = st["V"], st["G"].copy(), st["H"].copy(), st["chat"]
    y = A @ V[j - 1]
    w = y - st["alpha_prev"] * V[j - 1] - st["beta_prev"] * V[j - 2]
    nrm2 = w @ w
    b = np.sqrt(nrm2)
    cn = chat / b
    vo = w / b
    yo = A @ vo
    a0 = vo @ yo
    z = yo - a0 * vo - b * V[j - 1]
    Hc = Hm[: j + 1, :j].copy()
    Hc[j, j - 1] += b
    Hc[:j, j - 1] += b * cn
    mu = Hc @ cn
    gam = mu.copy()
    gam[:j] -= a0 * cn
    gp = np.concatenate([cn - G[:j, :j] @ cn, [1.0]])
    q = Hc[:j, :].T @ cn + Hc[j, :]
    vAv = a0 - 2.0 * (cn @ q)
    p = np.empty(j + 1)
    p[:j] = (Hc * gp[:, None]).sum(axis=0) - a0 * gp[:j] - b * G[:j, j - 1]
    p[j] = vAv - a0 * gp[j] - b * gp[j - 1]
    kap = gam + p
    ut = w - chat @ V
    d1 = V @ w
    v = ut / b
    d2 = V @ z
    vz = v @ z
    ut2 = z - kap[:j] @ V - kap[j] * v
    uu, uu2 = ut @ ut, ut2 @ ut2
    dn = d1 / b
    G[:j, j] = dn - G[:j, :j] @ cn
    G[j, j] = uu / nrm2
    G[j, :j] = G[:j, j]
    Hm[j, j - 1] += b
    Hm[:j, j - 1] += b * cn
    Hm[j, j] += a0
    Hm[j - 1, j] += b
    b2 = np.sqrt(uu2)
    G[:j, j + 1] = (d2 - G[:j, : j + 1] @ kap) / b2
    G[j, j + 1] = (vz - G[j, : j + 1] @ kap) / b2
    G[j + 1, j + 1] = 1.0
    G[j + 1, : j + 1] = G[: j + 1, j + 1]
    v2 = ut2 / b2
    Hm[j + 1, j] += b2
    Hm[: j + 1, j] += p
    y2 = A @ v2
    return {"a0": a0, "b": b, "kap": kap, "p": p, "d1": np.concatenate([d1, [uu]]), "d2": np.concatenate([d2, [vz, uu2]]), "u2": ut2,
            "rows": [v, v2], "G": G, "H": Hm, "v_last": v2, "y": y2, "alpha_last": float(v2 @ y2), "b2": b2}


def float64_single(A, st, tau=R.TAU):
    j = st["j"]
    V, G, Hm, chat = st["V"], st["G"].copy(), st["H"].copy(), st["chat"]
    y = A @ V[j - 1]
    w = y - st["alpha_prev"] * V[j - 1] - st["beta_prev"] * V[j - 2]
    t = chat @ V
    ut = 2 * w - (t + w)
    d = V @ w
    nrm2 = w @ w
    uu = ut @ ut
    b = np.sqrt(nrm2)
    dn, cn = d / b, chat / b
    col = np.concatenate([dn - G[:j, :j] @ cn, [uu / nrm2]])
    capp = cn.copy()
    out = {"d": np.concatenate([d, [uu, nrm2]])}
    if np.abs(dn - cn).max() > tau:
        g = col[:j].copy()
        ut = ut - (b * g) @ V
        Gjj = G[:j, :j]
        col = np.concatenate([col[:j] - Gjj @ g, [col[j] - 2.0 * g @ col[:j] + g @ Gjj @ g]])
        capp = capp + g
        out["gcorr"] = g
    v = ut / b
    Hm[j, j - 1] += b
    Hm[:j, j - 1] += b * capp
    G[: j + 1, j] = col
    G[j, : j + 1] = col
    yj = A @ v
    out.update(u=ut, rows=[v], G=G, H=Hm, v_last=v, y=yj, alpha_last=float(v @ yj), b=b)
    return out


def step_errors(out, dev, j, width, keys):
    """``error / bound`` of a float64 evaluation ``dev`` of a step that makes ``width`` rows, against the reference ``out``"""
    k = j + width
    q = {key: worst(np.abs(out[key].v - dev[key]), out[key].e) for key in keys}
    ref = R.cat(out["rows"])
    q["rows"] = worst(np.abs(ref.v - np.concatenate(dev["rows"])), ref.e)
    q["G"] = max(worst(np.abs(out["G"].v[:, j:k] - dev["G"][:, j:k]), out["G"].e[:, j:k]),
                 worst(np.abs(out["G"].v[j:k, :] - dev["G"][j:k, :]), out["G"].e[j:k, :]))
    q["H"] = worst(np.abs(out["H"].v[:, j - 1 : k - 1] - dev["H"][:, j - 1 : k - 1]), out["H"].e[:, j - 1 : k - 1])
    q["y"] = worst(np.abs(out["y"].v - dev["y"]), out["y"].e)
    q["alpha_last"] = worst(abs(float(out["alpha_last"].v) - dev["alpha_last"]), out["alpha_last"].e)
    return q


@pytest.mark.parametrize("kind", ["orth", "skew", "miss"])
@pytest.mark.parametrize("name,j,n", HOST_CASES)
def test_pair_and_single_float64_prototypes_within_bounds(name, j, n, kind):
    A, st = matrix(name), state(name, j, n, kind)
    dev = float64_pair(A, st)
    keys = ("a0", "b", "kap", "p", "d1", "d2", "u2", "b2")
    forward = step_errors(pair_ref(name, j, n, kind), dev, j, 2, keys)
    staged = step_errors(R.pair_step(A, st, given=dev), dev, j, 2, keys)
    print(f"pair {name} j={j} {kind}: forward " + " ".join(f"{k}={v:.2e}" for k, v in forward.items()))
    print(f"pair {name} j={j} {kind}: staged  " + " ".join(f"{k}={v:.2e}" for k, v in staged.items()))
    assert all(v <= 1.0 for v in forward.values()) and all(v <= 1.0 for v in staged.values())  # (a NaN fails)
    dev = float64_single(A, st)
    keys = ("d", "u", "b") + (("gcorr",) if "gcorr" in dev else ())
    forward = step_errors(single_ref(name, j, n, kind), dev, j, 1, keys)
    staged = step_errors(R.single_step(A, st, given=dev), dev, j, 1, keys)
    print(f"single {name} j={j} {kind}: forward " + " ".join(f"{k}={v:.2e}" for k, v in forward.items()))
    print(f"single {name} j={j} {kind}: staged  " + " ".join(f"{k}={v:.2e}" for k, v in staged.items()))
    assert all(v <= 1.0 for v in forward.values()) and all(v <= 1.0 for v in staged.values())  # (a NaN fails)
