"""CPU prototype of the group form of the one-sweep loop (NumPy, float64; no GPU): ONE walk over the basis per m Lanczos steps.

Notation is tools/one_sweep_prototype.py's: G = V V^T, Hm the applied coefficients (A V_i = sum_l Hm[l, i] V_l to rounding), chat the
un-normalised predictions V_i . w_j that closing() leaves behind, y = A V[j-1].  A group starts at a step j >= 2 with j + m <= n:

1. chain: m - 1 plain Lanczos steps with no walk.  w = (y - alpha_{j-1} V[j-1]) - beta_{j-1} V[j-2], b_0 = ||w||, x_0 = w / b_0, and for
   t < m - 1: y_t = A x_t, a_t = x_t . y_t, z = (y_t - a_t x_t) - b_t x_{t-1} (x_{-1} = V[j-1]), b_{t+1} = ||z||, x_{t+1} = z / b_{t+1}.
2. predict: Paige's and Simon's omega-recurrence over the extended set B = [V_0 .. V_{j-1}, x_0 .. x_{m-1}], with the full Hm in place of
   the tridiagonal: g[t][r] = B_r . x_t for the rows r before x_t (g[t][j + s] is the in-group row x_s).
3. walk over rows 0 .. j-1: measured d_t[i] = V_i . x_t, applied r_t = x_t - sum_i g[t][i] V_i; the epilogue finishes the group with the
   predicted in-group coefficients, v_{j+t} = r_t - sum_{s<t} g[t][j+s] v_{j+s}, and measures v_{j+s} . x_t (s < t) and v_{j+t} . v_{j+t}.
4. post: the leftovers e_old = max |d_t - g[t][:j]| and e_in = max |v_{j+s} . x_t - g[t][j+s]|, the new columns of G and of Hm.
5. closing: the SpMV on the corrected V[j+m-1], whose alpha sum predicts the next chat.

There is no correcting sweep and no re-normalisation in a group: a leftover above tau (or a NaN) marks the run as abandoned.  Steps 0, 1
and the steps left over behind the last group are the single fused form's, as in one_sweep_pair_lanczos.  The device kernels
(k_os_quad_predict / k_os_quad_sweep / k_os_quad_post, lanczos_amd/csrc/lz_reorth.hip) restate this arithmetic at m = 4.

The device's default chain works in the units of z (chain="unscaled"): the product runs on the unscaled z_t, b_t = ||z_t|| and
a_t = z_t . A z_t / ||z_t||^2 come out of one pair of sums behind it, z_{t+1} = (A z_t / b_t - a_t (z_t / b_t)) - b_t x_{t-1}, and
x_t = z_t / b_t is formed by division wherever it is read.  Same leftovers (tests/test_one_sweep_chain_host.py).

    python tools/one_sweep_group_prototype.py [--m 4] [--chain unscaled]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import one_sweep_prototype as proto  # noqa: E402


def group_predict(G, Hm, chat, a, b, j, m):
    """g[t] (t < m), length j + t: the predicted dots of x_t against rows 0 .. j-1 and against x_0 .. x_{t-1}."""
    g = [np.zeros(j + t) for t in range(m)]
    g[0][:j] = chat / b[0]
    for t in range(m - 1):
        gt = g[t]
        new = g[t + 1]
        # rows of the old basis: (A V_i) . x_t = sum_{l<j} Hm[l, i] g[t][l], and column j - 1 of the extended H has b_0 in row x_0
        s = Hm[:j, :j].T @ gt[:j]
        s[j - 1] += b[0] * (gt[j] if t else 1.0)
        prev = g[t - 1][:j] if t else G[:j, j - 1]
        new[:j] = ((s - a[t] * gt[:j]) - b[t] * prev) / b[t + 1]
        for s_ in range(t):  # in-group rows x_s, s < t: column x_s of the extended H is tridiagonal
            up = 1.0 if s_ + 1 == t else gt[j + s_ + 1]
            lo = gt[j + s_ - 1] if s_ else gt[j - 1]
            pv = 1.0 if s_ == t - 1 else g[t - 1][j + s_]
            new[j + s_] = ((((b[s_ + 1] * up + a[s_] * gt[j + s_]) + b[s_] * lo) - a[t] * gt[j + s_]) - b[t] * pv) / b[t + 1]
        lo = gt[j + t - 1] if t else gt[j - 1]  # row x_t itself: the sum is the measured a_t, the diagonal is 1
        new[j + t] = -(b[t] * lo) / b[t + 1]
    return g


def group_post(G, Hm, g, D, mm, vv, a, b, j, m, n):
    """The leftovers, the m new columns of G and columns j - 1 .. j + m - 2 of Hm (in place)."""
    e_old = max(np.abs(D[t] - g[t][:j]).max() for t in range(m))
    e_in = max([abs(mm[s, t] - g[t][j + s]) for t in range(m) for s in range(t)] + [0.0])
    if any(np.isnan(D[t]).any() for t in range(m)) or np.isnan(mm).any() or np.isnan(vv).any():
        e_old = np.inf
    for t in range(m):
        col = np.zeros(j + t + 1)
        col[:j] = D[t] - G[:j, : j + t] @ g[t]
        for s in range(t):
            col[j + s] = mm[s, t] - G[j + s, : j + t] @ g[t]
        col[j + t] = vv[t]
        G[: j + t + 1, j + t] = col
        G[j + t, : j + t + 1] = col
    Hm[:j, j - 1] += b[0] * g[0]
    Hm[j, j - 1] += b[0]
    C = [np.concatenate([g[t], [1.0]]) for t in range(m)]  # x_t = sum_r C[t][r] V_r in the finished basis
    for t in range(m - 1):
        col = np.zeros(n)
        col[: j + t + 2] += b[t + 1] * C[t + 1]
        col[: j + t + 1] += a[t] * C[t]
        if t:
            col[: j + t] += b[t] * C[t - 1]
        else:
            col[j - 1] += b[0]
        col -= Hm[:, : j + t] @ g[t]
        Hm[:, j + t] = col
    return e_old, e_in


def one_sweep_group_lanczos(H, n, m=4, seed=99, v0=None, tau=1e-14, chain="scaled"):
    """Returns (alpha, beta, V, stats); stats: groups, abandoned, e_old / e_in (per first step of a group), trips (the single steps'), G.
    chain: "scaled" - every chain vector is normalised before its product, as described above - or "unscaled": the device's default."""
    if chain not in ("scaled", "unscaled"):
        raise ValueError("chain must be 'scaled' or 'unscaled'")
    H = scipy.sparse.csr_matrix(H)
    M = H.shape[0]
    V = np.zeros((n, M))
    V[0] = proto.start_vector(M, seed, v0)
    alpha = np.zeros(n)
    bet = np.zeros(n)
    G = np.zeros((n, n))
    Hm = np.zeros((n, n))
    y = H @ V[0]
    alpha[0] = np.dot(y, V[0])
    r = y - alpha[0] * V[0]
    e_olds, e_ins, emax = np.zeros(n), np.zeros(n), np.zeros(n)
    trips = []
    abandoned = False
    groups = 0
    chat = np.zeros(0)

    def closing(j, b):  # one_sweep_pair_lanczos's
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
        if j >= 2 and j + m <= n:
            groups += 1
            # 1. the speculative chain
            a, b = np.zeros(m), np.zeros(m)
            X = np.zeros((m, M))
            w = (y - alpha[j - 1] * V[j - 1]) - bet[j - 1] * V[j - 2]
            if chain == "unscaled":
                # the chain in the units of z (one_sweep_quad_iter's default): the product runs on the unscaled z_t, both sums are taken
                # behind it, and x_t = z_t / b_t is formed by division wherever it is read - in the three-term pass and in the walk
                Z = np.zeros((m, M))
                Z[0] = w
                for t in range(m - 1):
                    yt = H @ Z[t]
                    nz = np.dot(Z[t], Z[t])
                    b[t] = np.sqrt(nz)
                    a[t] = np.dot(Z[t], yt) / nz
                    Z[t + 1] = (yt / b[t] - a[t] * (Z[t] / b[t])) - b[t] * (Z[t - 1] / b[t - 1] if t else V[j - 1])
                b[m - 1] = np.sqrt(np.dot(Z[m - 1], Z[m - 1]))
                for t in range(m):
                    X[t] = Z[t] / b[t]
            else:
                b[0] = np.sqrt(np.dot(w, w))
                X[0] = w / b[0]
                for t in range(m - 1):
                    yt = H @ X[t]
                    a[t] = np.dot(X[t], yt)
                    z = (yt - a[t] * X[t]) - b[t] * (X[t - 1] if t else V[j - 1])
                    b[t + 1] = np.sqrt(np.dot(z, z))
                    X[t + 1] = z / b[t + 1]
            # 2. the predictions
            g = group_predict(G, Hm, chat, a, b, j, m)
            # 3. the one walk over rows 0 .. j-1 and its epilogue
            D = [V[:j] @ X[t] for t in range(m)]
            Vn = np.zeros((m, M))
            mm = np.zeros((m, m))
            vv = np.zeros(m)
            for t in range(m):
                v = X[t] - g[t][:j] @ V[:j]
                for s in range(t):
                    v = v - g[t][j + s] * Vn[s]
                Vn[t] = v
                for s in range(t):
                    mm[s, t] = np.dot(Vn[s], X[t])
                vv[t] = np.dot(v, v)
            # 4. post
            V[j : j + m] = Vn
            e_old, e_in = group_post(G, Hm, g, D, mm, vv, a, b, j, m, n)
            e_olds[j], e_ins[j] = e_old, e_in
            emax[j : j + m] = max(e_old, e_in)
            if not (e_old <= tau and e_in <= tau):  # (a NaN fails both comparisons)
                abandoned = True
            alpha[j : j + m - 1] = a[: m - 1]
            bet[j : j + m] = b
            # 5. closing
            y, chat = closing(j + m - 1, b[m - 1])
            j += m
            continue
        if j == 0:
            nrm2 = np.dot(r, r)
            b1 = np.sqrt(nrm2)
            cs = nrm2 / (b1 * b1)
            u = r / b1
            v = 2 * u - cs * u
            col = np.array([np.dot(v, v)])
        else:  # the single fused form (one_sweep_fused_lanczos)
            w = y - alpha[j - 1] * V[j - 1]
            if j >= 2:
                w = w - bet[j - 1] * V[j - 2]
            t_ = chat @ V[:j]
            ut = 2 * w - (t_ + w)
            d = V[:j] @ w
            nrm2 = np.dot(w, w)
            b1 = np.sqrt(nrm2)
            dn, cn = d / b1, chat / b1
            emax[j] = np.abs(dn - cn).max()
            col = np.concatenate([dn - G[:j, :j] @ cn, [np.dot(ut, ut) / nrm2]])
            capp = cn.copy()
            if emax[j] > tau:
                trips.append(j)
                gg = col[:j].copy()
                ut = ut - (b1 * gg) @ V[:j]
                Gjj = G[:j, :j]
                col = np.concatenate([col[:j] - Gjj @ gg, [col[j] - 2.0 * gg @ col[:j] + gg @ Gjj @ gg]])
                capp = capp + gg
            v = ut / b1
            Hm[j, j - 1] += b1
            Hm[:j, j - 1] += b1 * capp
        bet[j] = b1
        V[j] = v
        G[: j + 1, j] = col
        G[j, : j + 1] = col
        y, chat = closing(j, b1)
        j += 1
    stats = {"emax": emax, "e_old": e_olds, "e_in": e_ins, "trips": trips, "G": G, "abandoned": abandoned, "groups": groups}
    return alpha, bet[1:], V, stats


def report(name, H, n, m, v0=None, chain="scaled"):
    a0, b0, V0 = proto.two_pass_lanczos(H, n, v0=v0)
    a1, b1, V1, st = one_sweep_group_lanczos(H, n, m, v0=v0, chain=chain)
    scale = np.abs(proto.tridiag_eigs(a0, b0)).max()
    orth = np.abs(V1 @ V1.T - np.eye(n)).max()
    orth0 = np.abs(V0 @ V0.T - np.eye(n)).max()
    return (f"| {name} | {n} | {m} | {st['e_old'].max():.1e} | {st['e_in'].max():.1e} | {orth:.1e} ({orth0:.1e}) | "
            f"{np.abs(a1 - a0).max() / scale:.1e} | {np.abs(b1 - b0).max() / scale:.1e} | {'abandoned' if st['abandoned'] else ''} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--chain", default="scaled", choices=["scaled", "unscaled"], help="unscaled: the chain in the units of z (the device's default)")
    args = ap.parse_args()
    print("| case | n | m | max e_old | max e_in | max\\|VVᵀ−I\\| (two-pass) | max\\|Δα\\|/scale | max\\|Δβ\\|/scale | |")
    print("|" + "---|" * 9)
    for m in sorted({2, args.m, 6}):
        print(report("lap2d 300 x 200", proto.lap2d(300, 200), 200, m, chain=args.chain), flush=True)
    for name, H, n, v0 in proto.fixtures():
        print(report(name, H, n, args.m, v0=v0, chain=args.chain), flush=True)


if __name__ == "__main__":
    main()
