"""CPU prototype of the one-sweep full re-orthogonalisation step (NumPy, float64; no GPU).

The fused-norm loop reads the basis V twice per step: pass 1 forms c = V^T w, pass 2 forms v_j = 2 w/beta - sum c_i V_i.
The one-sweep step predicts c from two small matrices and measures it in the same sweep that applies it:

* G = V^T V (n x n), H = the applied coefficients of every step with alpha and beta, so that A V_i = sum_l H[l, i] V_l holds
  to rounding.  With A symmetric, V_i . w_{j+1} = (A V_i) . v_j - alpha_j G[i, j] - beta_j G[i, j-1], where
  (A V_i) . v_j = sum_l H[l, i] G[l, j] (i < j) and V_j . A v_j = alpha_j (the SpMV's own dot).
* The sweep forms v_j with the predicted c_hat and, from the same loads, the true dots d_i = V_i . w.
* post: e_i = d_i / beta - c_hat_i; G[:, j] from d, c_hat and the old G; when max|e| > tau one correcting sweep
  v_j -= sum_i G[i, j] V_i runs (its coefficients are added to the applied ones).

Arithmetic and quirks are the reference's: V[0] is the warm-up residual, the self term c_j = ||w||^2 / beta^2 is
included, no re-normalisation.  `two_pass_lanczos` restates the two-pass step (the reference recurrence) as the yardstick;
tests/test_one_sweep_host.py ties both to the test oracle.  `predict` and `post` are the device kernels' arithmetic
(lanczos_amd/csrc/lz_reorth.hip, k_os_predict / k_os_post) and are checked against them by tests/test_one_sweep_host.py.

    python tools/one_sweep_prototype.py [--big NX] [--out profiles/one_sweep_prototype.md]
"""
from __future__ import annotations

import argparse
import ast
import os
import sys
import time

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

TAUS = (1e-15, 3e-15, 1e-14, 3e-14, 1e-13)


def start_vector(M, seed=99, v0=None):
    v = np.random.RandomState(seed).uniform(-1, 1, size=M) if v0 is None else np.array(v0, dtype=np.float64)
    return v / np.linalg.norm(v)


def two_pass_lanczos(H, n, seed=99, v0=None, reverse=False):
    """The reference recurrence with its two passes over V per step (c = V w, then v_j = 2 w - sum c_i V_i).  reverse=True
    sums every dot in the opposite order: what that moves is not determined by the arithmetic (the stable prefix)."""
    M = H.shape[0]
    dot = (lambda x, y: x[::-1] @ y[::-1]) if reverse else np.dot
    V = np.zeros((n, M))
    V[0] = start_vector(M, seed, v0)
    alpha, beta = np.zeros(n), np.zeros(n - 1)
    r = H @ V[0]
    alpha[0] = dot(r, V[0])
    r = r - alpha[0] * V[0]
    for j in range(n):
        beta[j - 1] = np.sqrt(dot(r, r))
        V[j] = r / beta[j - 1]
        c = V[: j + 1] @ V[j]
        V[j] = 2 * V[j] - np.sum(c[:, None] * V[: j + 1], axis=0)
        r = H @ V[j]
        alpha[j] = dot(V[j], r)
        r = r - V[j] * alpha[j] - V[j - 1] * beta[j - 1]
    return alpha, beta, V


def tridiag_eigs(alpha, beta):
    return np.linalg.eigvalsh(np.diag(alpha) + np.diag(beta, 1) + np.diag(beta, -1))


def predict(G, Hm, alpha_j, beta_j, nrm2, j):
    """Coefficients c_hat[0..j] of step j+1 (units of u_{j+1} = w_{j+1} / beta_{j+1}); beta_j is the norm that formed v_j,
    nrm2 = ||w_{j+1}||^2.  Sums run in index order, as the device kernel's do."""
    b_next = np.sqrt(nrm2)
    c = np.zeros(j + 1)
    for i in range(j + 1):
        if i < j:
            s = 0.0
            for l in range(i + 2):
                s += Hm[l, i] * G[l, j]
        else:
            s = alpha_j
        s = s - alpha_j * G[i, j]
        if j > 0:
            s = s - beta_j * G[i, j - 1]
        c[i] = s / b_next
    return c


def post(G, du, vv, chat, cs, j):
    """Leftovers e = du - c_hat and the new Gram column: V_i . v_j = (2 - cs) du_i - sum_l c_hat_l G[i, l]; G[j, j] = v.v
    (du_i = V_i . u_j, the dots the sweep measures)."""
    e = np.zeros(j)
    col = np.zeros(j + 1)
    for i in range(j):
        di = du[i]
        e[i] = di - chat[i]
        s = (2.0 - cs) * di
        for l in range(j):
            s -= chat[l] * G[i, l]
        col[i] = s
    col[j] = vv
    return e, col


def correct_column(G, col, g, j):
    """Gram column after v_j -= sum_i g_i V_i (g = col[:j])."""
    new = col.copy()
    for i in range(j):
        s = col[i]
        for l in range(j):
            s -= G[i, l] * g[l]
        new[i] = s
    t = col[j]
    for i in range(j):
        t -= 2.0 * g[i] * col[i]
        for l in range(j):
            t += g[i] * g[l] * G[i, l]
    new[j] = t
    return new


def one_sweep_lanczos(H, n, seed=99, v0=None, tau=1e-14, fast=True):
    """Returns (alpha, beta, V, stats).  fast=True evaluates predict/post with matrix products (same quantities, other
    summation order) so the 10^6-row case finishes in minutes."""
    H = scipy.sparse.csr_matrix(H)
    M = H.shape[0]
    V = np.zeros((n, M))
    V[0] = start_vector(M, seed, v0)
    alpha = np.zeros(n)
    bet = np.zeros(n)  # bet[j]: the norm that formed V[j]; the reference's beta is bet[1:]
    G = np.zeros((n, n))
    Hm = np.zeros((n, n))
    r = H @ V[0]
    alpha[0] = np.dot(r, V[0])
    r = r - alpha[0] * V[0]
    nrm2 = np.dot(r, r)
    chat = np.zeros(0)
    emax = np.zeros(n)
    trips = []
    for j in range(n):
        b = np.sqrt(nrm2)
        bet[j] = b
        cs = nrm2 / (b * b)
        u = r / b
        # the sweep: v_j = 2 u - (sum_{i<j} c_hat_i V_i + cs u); d_i = V_i . r from the same rows
        t = chat @ V[:j] if j else np.zeros(M)
        v = 2 * u - (t + cs * u)
        d = V[:j] @ r
        vv = np.dot(v, v)
        if fast:
            di = d / b
            e = di - chat
            col = np.concatenate([(2.0 - cs) * di - G[:j, :j] @ chat, [vv]])
        else:
            e, col = post(G, d / b, vv, chat, cs, j)
        emax[j] = np.abs(e).max() if j else 0.0
        capp = chat.copy()
        if j and emax[j] > tau:
            trips.append(j)
            g = col[:j].copy()
            v = v - g @ V[:j]
            if fast:
                Gjj = G[:j, :j]
                col = np.concatenate([col[:j] - Gjj @ g, [col[j] - 2.0 * g @ col[:j] + g @ Gjj @ g]])
            else:
                col = correct_column(G, col, g, j)
            capp = capp + g
        V[j] = v
        G[: j + 1, j] = col
        G[j, : j + 1] = col
        if j:  # w_j = b/(2 - cs) (v_j + sum_{l<j} capp_l V_l): column j-1 of H
            Hm[j, j - 1] += b / (2.0 - cs)
            Hm[:j, j - 1] += b * capp / (2.0 - cs)
        y = H @ v
        alpha[j] = np.dot(v, y)
        r = y - v * alpha[j]
        if j:
            r = r - V[j - 1] * b
        Hm[j, j] += alpha[j]
        if j:
            Hm[j - 1, j] += b
        nrm2 = np.dot(r, r)
        if j + 1 < n:
            if fast:
                p = np.empty(j + 1)
                p[:j] = (Hm[: j + 1, :j] * G[: j + 1, j][:, None]).sum(axis=0) if j else p[:j]
                p[j] = alpha[j]
                p = p - alpha[j] * G[: j + 1, j]
                if j:
                    p = p - b * G[: j + 1, j - 1]
                chat = p / np.sqrt(nrm2)
            else:
                chat = predict(G, Hm, alpha[j], b, nrm2, j)
    stats = {"emax": emax, "trips": trips, "G": G}
    return alpha, bet[1:], V, stats


def one_sweep_fused_lanczos(H, n, seed=99, v0=None, tau=1e-14):
    """The fused form of the loop (run_loop_one_sweep_fused): from step 1 on there is no three-term pass - the sweep forms
    w_j = (A v_{j-1} - alpha v_{j-1}) - beta v_{j-2} itself and works in the units of w: the predictions are not divided by beta, the
    self term is exactly 1, u~ = 2 w - (sum c'_i V_i + w), and V_i . w, u~ . u~ and ||w||^2 are measured in the same walk.  Post
    divides the measured and the predicted dots by b = sqrt(||w||^2) (deferred normalisation); v_j = u~ / b is formed by the SpMV."""
    H = scipy.sparse.csr_matrix(H)
    M = H.shape[0]
    V = np.zeros((n, M))
    V[0] = start_vector(M, seed, v0)
    alpha = np.zeros(n)
    bet = np.zeros(n)
    G = np.zeros((n, n))
    Hm = np.zeros((n, n))
    y = H @ V[0]
    alpha[0] = np.dot(y, V[0])
    r = y - alpha[0] * V[0]
    emax = np.zeros(n)
    trips = []
    chat = np.zeros(0)
    for j in range(n):
        if j == 0:  # step 0 is the unfused form's: units of u = r / b, cs = ||r||^2 / b^2
            nrm2 = np.dot(r, r)
            b = np.sqrt(nrm2)
            cs = nrm2 / (b * b)
            u = r / b
            v = 2 * u - cs * u
            col = np.array([np.dot(v, v)])
            capp = chat
        else:
            w = y - alpha[j - 1] * V[j - 1]
            if j >= 2:
                w = w - bet[j - 1] * V[j - 2]
            t = chat @ V[:j]
            ut = 2 * w - (t + w)
            d = V[:j] @ w
            nrm2 = np.dot(w, w)
            b = np.sqrt(nrm2)
            dn, cn = d / b, chat / b
            emax[j] = np.abs(dn - cn).max()
            col = np.concatenate([dn - G[:j, :j] @ cn, [np.dot(ut, ut) / nrm2]])
            capp = cn.copy()
            if emax[j] > tau:
                trips.append(j)
                g = col[:j].copy()
                ut = ut - (b * g) @ V[:j]
                Gjj = G[:j, :j]
                col = np.concatenate([col[:j] - Gjj @ g, [col[j] - 2.0 * g @ col[:j] + g @ Gjj @ g]])
                capp = capp + g
            v = ut / b  # (the SpMV's division on read)
            Hm[j, j - 1] += b
            Hm[:j, j - 1] += b * capp
        bet[j] = b
        V[j] = v
        G[: j + 1, j] = col
        G[j, : j + 1] = col
        y = H @ v
        alpha[j] = np.dot(v, y)
        Hm[j, j] += alpha[j]
        if j:
            Hm[j - 1, j] += b
        if j + 1 < n:  # un-normalised predictions V_i . w_{j+1}
            p = np.empty(j + 1)
            p[:j] = (Hm[: j + 1, :j] * G[: j + 1, j][:, None]).sum(axis=0) if j else p[:j]
            p[j] = alpha[j]
            p = p - alpha[j] * G[: j + 1, j]
            if j:
                p = p - b * G[: j + 1, j - 1]
            chat = p
    stats = {"emax": emax, "trips": trips, "G": G}
    return alpha, bet[1:], V, stats


def one_sweep_pair_lanczos(H, n, seed=99, v0=None, tau=1e-14):
    """The pair form of the loop (run_loop_one_sweep_pair): one walk over the basis per two steps.  Steps 0, 1 and an odd last
    step are the fused single form's.  A pair at step j takes the speculative SpMV of the uncorrected vo = w_j / b; the correction
    step j owes to w_{j+1} is a combination of basis rows, A (sum cn_i V_i) = sum_i cn_i sum_l H[l, i] V_l, so the one walk over
    rows 0..j-1 finishes v_j and forms u~_{j+1} = z - sum kap_i V_i with the dots of both.  alpha_j is the speculative SpMV's own
    dot and beta_{j+1} = ||u~_{j+1}||.  There is no correcting sweep in a pair: a leftover above tau (or a NaN) marks the run as
    abandoned (stats["abandoned"]); e1 / e2 hold the leftovers of the first / second step of every pair."""
    H = scipy.sparse.csr_matrix(H)
    M = H.shape[0]
    V = np.zeros((n, M))
    V[0] = start_vector(M, seed, v0)
    alpha = np.zeros(n)
    bet = np.zeros(n)
    G = np.zeros((n, n))
    Hm = np.zeros((n, n))
    y = H @ V[0]
    alpha[0] = np.dot(y, V[0])
    r = y - alpha[0] * V[0]
    emax = np.zeros(n)
    e1s, e2s = np.zeros(n), np.zeros(n)
    trips = []
    abandoned = False
    pairs = 0
    chat = np.zeros(0)

    def closing(j, b):  # y = A V[j], alpha[j], the H entries of step j and the un-normalised predictions V_i . w_{j+1}
        y = H @ V[j]
        alpha[j] = np.dot(V[j], y)
        Hm[j, j] += alpha[j]
        if j:
            Hm[j - 1, j] += b
        p = np.zeros(0)
        if j + 1 < n:
            p = np.empty(j + 1)
            p[:j] = (Hm[: j + 1, :j] * G[: j + 1, j][:, None]).sum(axis=0) if j else p[:j]
            p[j] = alpha[j]
            p = p - alpha[j] * G[: j + 1, j]
            if j:
                p = p - b * G[: j + 1, j - 1]
        return y, p

    j = 0
    while j < n:
        if j >= 2 and j + 1 < n:
            pairs += 1
            w = y - alpha[j - 1] * V[j - 1] - bet[j - 1] * V[j - 2]
            nrm2 = np.dot(w, w)
            b = np.sqrt(nrm2)
            cn = chat / b
            vo = w / b
            yo = H @ vo
            a0 = np.dot(vo, yo)
            z = yo - a0 * vo - b * V[j - 1]
            Hc = Hm[: j + 1, :j].copy()
            Hc[j, j - 1] += b
            Hc[:j, j - 1] += b * cn
            mu = Hc @ cn
            gam = mu.copy()
            gam[:j] -= a0 * cn
            gp = np.concatenate([cn - G[:j, :j] @ cn, [1.0]])
            q = Hc[:j, :].T @ cn + Hc[j, :]
            vAv = a0 - 2.0 * np.dot(cn, q)
            p = np.empty(j + 1)
            p[:j] = (Hc * gp[:, None]).sum(axis=0) - a0 * gp[:j] - b * G[:j, j - 1]
            p[j] = vAv - a0 * gp[j] - b * gp[j - 1]
            kap = gam + p
            # the one walk over rows 0..j-1
            ut = w - chat @ V[:j]
            d1 = V[:j] @ w
            v = ut / b
            d2 = V[:j] @ z
            vz = np.dot(v, z)
            ut2 = z - kap[:j] @ V[:j] - kap[j] * v
            uu = np.dot(ut, ut)
            uu2 = np.dot(ut2, ut2)
            # post
            dn = d1 / b
            e1 = np.abs(dn - cn).max()
            G[:j, j] = dn - G[:j, :j] @ cn
            G[j, j] = uu / nrm2
            G[j, :j] = G[:j, j]
            Hm[j, j - 1] += b
            Hm[:j, j - 1] += b * cn
            alpha[j] = a0
            Hm[j, j] += a0
            Hm[j - 1, j] += b
            bet[j] = b
            V[j] = v
            b2 = np.sqrt(uu2)
            G[:j, j + 1] = (d2 - G[:j, : j + 1] @ kap) / b2
            G[j, j + 1] = (vz - G[j, : j + 1] @ kap) / b2
            G[j + 1, j + 1] = 1.0
            G[j + 1, : j + 1] = G[: j + 1, j + 1]
            e2 = np.abs(G[: j + 1, j + 1]).max()
            V[j + 1] = ut2 / b2
            bet[j + 1] = b2
            Hm[j + 1, j] += b2
            Hm[: j + 1, j] += p
            e1s[j], e2s[j + 1] = e1, e2
            emax[j], emax[j + 1] = e1, e2
            if not (e1 <= tau and e2 <= tau):  # (a NaN fails both comparisons)
                abandoned = True
            y, chat = closing(j + 1, b2)
            j += 2
            continue
        if j == 0:
            nrm2 = np.dot(r, r)
            b = np.sqrt(nrm2)
            cs = nrm2 / (b * b)
            u = r / b
            v = 2 * u - cs * u
            col = np.array([np.dot(v, v)])
        else:
            w = y - alpha[j - 1] * V[j - 1]
            if j >= 2:
                w = w - bet[j - 1] * V[j - 2]
            t = chat @ V[:j]
            ut = 2 * w - (t + w)
            d = V[:j] @ w
            nrm2 = np.dot(w, w)
            b = np.sqrt(nrm2)
            dn, cn = d / b, chat / b
            emax[j] = np.abs(dn - cn).max()
            col = np.concatenate([dn - G[:j, :j] @ cn, [np.dot(ut, ut) / nrm2]])
            capp = cn.copy()
            if emax[j] > tau:
                trips.append(j)
                g = col[:j].copy()
                ut = ut - (b * g) @ V[:j]
                Gjj = G[:j, :j]
                col = np.concatenate([col[:j] - Gjj @ g, [col[j] - 2.0 * g @ col[:j] + g @ Gjj @ g]])
                capp = capp + g
            v = ut / b
            Hm[j, j - 1] += b
            Hm[:j, j - 1] += b * capp
        bet[j] = b
        V[j] = v
        G[: j + 1, j] = col
        G[j, : j + 1] = col
        y, chat = closing(j, b)
        j += 1
    stats = {"emax": emax, "e1": e1s, "e2": e2s, "trips": trips, "G": G, "abandoned": abandoned, "pairs": pairs}
    return alpha, bet[1:], V, stats


def report_case(name, H, n, seed=99, v0=None):
    t0 = time.perf_counter()
    H = scipy.sparse.csr_matrix(H)
    a0, b0, V0 = two_pass_lanczos(H, n, seed, v0)
    t1 = time.perf_counter()
    a1, b1, V1, st = one_sweep_lanczos(H, n, seed, v0, tau=np.inf)
    t2 = time.perf_counter()
    scale = np.abs(tridiag_eigs(a0, b0)).max()
    prefix, rows = n, n
    if H.shape[0] <= 200_000:  # the stable prefix / rows: where a reversed-order evaluation agrees to 1e-12 of the scale / 1e-11
        a2, b2, V2 = two_pass_lanczos(H, n, seed, v0, reverse=True)
        bad = np.abs(a2 - a0) > 1e-12 * scale
        bad[:-1] |= np.abs(b2 - b0) > 1e-12 * scale
        prefix = int(np.argmax(bad)) if bad.any() else n
        badv = np.abs(V2 - V0).max(axis=1) > 1e-11
        rows = int(np.argmax(badv)) if badv.any() else n
    e = st["emax"][1:]
    orth = np.abs(V1 @ V1.T - np.eye(n)).max()
    orth0 = np.abs(V0 @ V0.T - np.eye(n)).max()
    da = np.abs(a1 - a0)[:prefix].max() / scale
    db = np.abs(b1 - b0)[: max(prefix - 1, 1)].max() / scale
    dv = np.abs(V1 - V0)[:rows].max() if rows else 0.0
    trips = {tau: int((e > tau).sum()) for tau in TAUS}
    return {
        "name": name, "M": H.shape[0], "n": n, "e_med": float(np.median(e)), "e_p99": float(np.quantile(e, 0.99)),
        "e_max": float(e.max()), "orth": orth, "orth_ref": orth0, "prefix": prefix, "da": da, "db": db, "rows": rows, "dv": dv,
        "trips": trips, "t_ref": t1 - t0, "t_os": t2 - t1,
    }


def gated_case(name, H, n, tau, seed=99, v0=None):
    """A full run with the gate live: orthogonality and trips."""
    _, _, V, st = one_sweep_lanczos(H, n, seed, v0, tau=tau)
    return np.abs(V @ V.T - np.eye(n)).max(), len(st["trips"])


def fixtures():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
    out = []
    for name, n in (("lap2d_32x32_n30", 30), ("graph_M2000_E7000_n40", 40), ("deuteron3d_N12_27pt_n100", 100),
                    ("ragged_M700_n25", 25), ("lap3d_8x8x8_n40", 40), ("box1d_N500_n50", 50), ("c1_dense512_n20", 20)):
        g = np.load(os.path.join(here, name + ".npz"))
        M = int(g["M"])
        if "rowptr" in g.files:
            H = scipy.sparse.csr_matrix((g["vals"], g["colidx"], g["rowptr"]), shape=(M, M))
        else:  # e.g. "dense_symmetric(512, seed=0)"
            from lanczos_amd import synthetic

            call = ast.parse(str(g["generator"]).split(";")[0].strip(), mode="eval").body
            obj = getattr(synthetic, call.func.id)(*[ast.literal_eval(a) for a in call.args],
                                                   **{k.arg: ast.literal_eval(k.value) for k in call.keywords})
            H = obj.to_scipy() if hasattr(obj, "to_scipy") else scipy.sparse.csr_matrix(obj)
        out.append((name, H, int(g["n"]), g["v0"] if "v0" in g.files else None))
    return out


def lap2d(nx, ny):
    ex = np.ones(nx)
    ey = np.ones(ny)
    Tx = scipy.sparse.diags([-ex[:-1], 2 * ex, -ex[:-1]], [-1, 0, 1])
    Ty = scipy.sparse.diags([-ey[:-1], 2 * ey, -ey[:-1]], [-1, 0, 1])
    return (scipy.sparse.kron(scipy.sparse.identity(ny), Tx) + scipy.sparse.kron(Ty, scipy.sparse.identity(nx))).tocsr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=1000, help="side of the 2-D Laplacian of the large case (0: skip)")
    ap.add_argument("--big-n", type=int, default=200)
    ap.add_argument("--tau", type=float, default=1e-13)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = fixtures()
    if args.big:
        cases.append((f"lap2d_5pt_{args.big}x{args.big}_k{args.big_n}", lap2d(args.big, args.big), args.big_n, None))
    lines = ["| case | M | n | max\\|e\\| per step: median / p99 / max | gate trips at tau = " + " / ".join(f"{t:.0e}" for t in TAUS)
             + " | max\\|VᵀV−I\\| (reference) | stable prefix | max\\|Δα\\|/scale | max\\|Δβ\\|/scale | max\\|ΔV\\| (stable rows) "
             + f"| tau = {args.tau:.0e} live: trips, max\\|VᵀV−I\\| |", "|" + "---|" * 11]
    for name, H, n, v0 in cases:
        r = report_case(name, H, n, v0=v0)
        orth_g, ntrip = gated_case(name, H, n, args.tau, v0=v0)
        lines.append(f"| {name} | {r['M']} | {n} | {r['e_med']:.1e} / {r['e_p99']:.1e} / {r['e_max']:.1e} | "
                     + " / ".join(str(r["trips"][t]) for t in TAUS)
                     + f" | {r['orth']:.1e} ({r['orth_ref']:.1e}) | {r['prefix']} | {r['da']:.1e} | {r['db']:.1e} | "
                     f"{r['dv']:.1e} ({r['rows']}) | {ntrip}, {orth_g:.1e} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
