"""lsmr piece by piece.  (GPU box; run by hand, not a test.)

    python tools/lsmr_probe.py [--nx 4000 --ny 2500 --dense 65536x4096 --reps 3 --tol 1e-8 --no-scipy --out FILE]      one JSON object

Two matrices: the edge-difference (gradient) operator ``G`` of the periodic ``nx x ny`` grid - ``2 nx ny x nx ny``, two entries a
row, ``G^T G`` = the periodic 5-point Laplacian, solved with ``damp = 0.1`` - and a dense random ``--dense`` matrix.  For each:

(a) ``parts_us``: the four parts of an iteration - the product ``A v``, ``k_lsmr_u``, the product ``A^T u``, ``k_lsmr_v`` with the
    three-term and the lagged update - device time by events (``lz_lsmr_step_time``: the mean of 20 launches behind a warm-up,
    repeated ``--reps`` times, median and spread).  ``u_bytes`` / ``v_bytes`` are the algorithmic bytes of the accounting in DESIGN.md
    section 8g (24 per padded row of ``b``'s length, 72 per padded row of ``x``'s) and ``*_frac_hbm_peak`` their rate over 8 TB/s.
(b) ``minres_step``: the yardstick - ``k_minres_step`` (72 B a row, the same shape) re-measured in the same run on a vector of
    ``x``'s length (the 5-point Laplacian of the same grid; the gradient workload only).
(c) ``iteration_us``: ``lz_lsmr_run`` of 64 steps as one chunk (all tolerances 0), host clock around the call, per step.
(d) ``solve``: ``lsmr`` to ``atol = btol = --tol`` at ``check_every`` = 8 / 32 / 128 on an open handle that holds the matrix already
    (``solve_seconds``) and once through ``lsmr`` itself with packing, upload and download (``end_to_end_seconds``).
(e) ``scipy_cpu``: ``scipy.sparse.linalg.lsmr`` on the same problem and tolerances on this machine's CPUs - a labelled baseline."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lanczos_amd import _capi, lsmr, synthetic  # noqa: E402
from lanczos_amd.eigsh import upload_matrix  # noqa: E402
from lanczos_amd.lsmr import DeviceLsmrBackend, solve  # noqa: E402
from lanczos_amd.svds import _pack  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def stats(ts):
    return {"median_us": float(np.median(ts)), "min_us": float(np.min(ts)), "max_us": float(np.max(ts))}


def gradient(nx, ny):
    """the edge-difference operator of the periodic nx x ny grid: row 2 i is x_right(i) - x_i, row 2 i + 1 is x_down(i) - x_i"""
    n = nx * ny
    idx = np.arange(n, dtype=np.int64)
    ix, iy = idx % nx, idx // nx
    right = iy * nx + (ix + 1) % nx
    down = ((iy + 1) % ny) * nx + ix
    cols = np.empty((n, 4), dtype=np.int32)
    cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3] = idx, right, idx, down
    vals = np.tile(np.array([-1.0, 1.0, -1.0, 1.0]), n)
    G = sp.csr_matrix((vals, cols.reshape(-1), np.arange(0, 4 * n + 1, 2, dtype=np.int32)), shape=(2 * n, n))
    G.sum_duplicates()
    G.sort_indices()
    return G


def minres_yardstick(nx, ny, reps):
    L = synthetic.laplacian_2d_5pt(nx, ny)
    n = nx * ny
    h = _capi.Handle(0)
    upload_matrix(h, L)
    plan = h.minres_info()
    b = np.random.default_rng(4).standard_normal(n)
    st = []
    for _ in range(reps):
        h.minres_begin(b, None, -0.05)
        h.minres_run(2, 0.0)
        st.append(h.minres_step_time(20)[1] * 1e3)
    step_bytes = float((72 if plan["scale_on_read"] else 80) * h.padded_rows(n))
    h.close()
    out = {"n": n, "step_us": stats(st), "step_bytes": step_bytes}
    out["step_frac_hbm_peak"] = step_bytes / (out["step_us"]["median_us"] * 1e-6) / HBM_PEAK
    return out


def probe(A, damp, tol, reps, scipy_too):
    M, N = A.shape
    rng = np.random.default_rng(4)
    b = rng.standard_normal(M)
    t = time.perf_counter()
    Aop, AopT, transposed = _pack(A)
    pack_seconds = time.perf_counter() - t
    h = _capi.Handle(0)
    t = time.perf_counter()
    if isinstance(Aop, np.ndarray):
        wide = not Aop.flags.c_contiguous
        h.gk_set_dense(AopT if wide else Aop, stored_transposed=wide)
        plan = "dense"
    else:
        h.gk_set_csr(Aop, AopT)
        plan = "csr"
    upload_seconds = time.perf_counter() - t
    out = {"shape": [M, N], "damp": damp, "tol": tol, "plan": plan, "transposed": bool(transposed), "pack_seconds": pack_seconds,
           "upload_seconds": upload_seconds, "own_launches_per_iteration": h.lsmr_info()["own_launches_per_iteration"]}
    parts = [[], [], [], []]
    for _ in range(reps):
        h.lsmr_begin(b, None, damp, transposed=transposed)
        h.lsmr_run(2, 0.0, 0.0, 0.0)
        for acc, ms in zip(parts, h.lsmr_step_time(20)):
            acc.append(ms * 1e3)
    names = ("product_av", "k_lsmr_u", "product_atu", "k_lsmr_v")
    out["parts_us"] = {name: stats(ts) for name, ts in zip(names, parts)}
    out["parts_sum_us"] = float(sum(np.median(ts) for ts in parts))
    out["u_bytes"], out["v_bytes"] = float(24 * h.padded_rows(M)), float(72 * h.padded_rows(N))
    out["u_frac_hbm_peak"] = out["u_bytes"] / (out["parts_us"]["k_lsmr_u"]["median_us"] * 1e-6) / HBM_PEAK
    out["v_frac_hbm_peak"] = out["v_bytes"] / (out["parts_us"]["k_lsmr_v"]["median_us"] * 1e-6) / HBM_PEAK
    ts = []
    for _ in range(reps + 1):
        h.lsmr_begin(b, None, damp, transposed=transposed)
        t = time.perf_counter()
        h.lsmr_run(64, 0.0, 0.0, 0.0)
        ts.append((time.perf_counter() - t) * 1e6 / 64)
    out["iteration_us"] = stats(ts[1:])
    out["solve"] = {}
    for check_every in (8, 32, 128):
        ts, info = [], {}
        for _ in range(reps):
            t = time.perf_counter()
            res = solve(DeviceLsmrBackend(h, transposed, plan), b, None, damp, tol, tol, 1e8, min(M, N), check_every, info=info)
            ts.append(time.perf_counter() - t)
        out["solve"][check_every] = {"solve_seconds": float(np.median(ts)), "min_seconds": float(np.min(ts)), "iterations": res[2],
                                     "chunks": info["chunks"], "istop": res[1]}
    h.close()
    t = time.perf_counter()
    x, istop, itn, normr, normar, normA, condA, normx = lsmr(A, b, damp, tol, tol)
    out["end_to_end_seconds"] = time.perf_counter() - t
    r = b - A @ x
    rbar = float(np.sqrt(r @ r + damp * damp * (x @ x)))
    out["result"] = {"istop": istop, "iterations": itn, "normr": normr, "normr_true": rbar, "normar": normar,
                     "normar_true": float(np.linalg.norm(A.T @ r - damp * damp * x)), "normA": normA, "condA": condA}
    if scipy_too:
        t = time.perf_counter()
        ref = sla.lsmr(A, b, damp=damp, atol=tol, btol=tol)
        sec = time.perf_counter() - t
        out["scipy_cpu"] = {"seconds": sec, "iterations": int(ref[2]), "istop": int(ref[1]),
                            "x_diff": float(np.linalg.norm(x - ref[0]) / np.linalg.norm(ref[0])),
                            "threads": int(os.environ.get("OMP_NUM_THREADS", 0))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4000)
    ap.add_argument("--ny", type=int, default=2500)
    ap.add_argument("--dense", default="65536x4096")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {}

    def save():
        text = json.dumps(out, indent=1)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return text

    out["minres_step"] = minres_yardstick(a.nx, a.ny, a.reps)
    save()
    G = gradient(a.nx, a.ny)
    out["gradient"] = probe(G, 0.1, a.tol, a.reps, not a.no_scipy)
    del G
    save()
    dm, dn = (int(v) for v in a.dense.split("x"))
    D = np.random.default_rng(7).standard_normal((dm, dn)) / np.sqrt(dm)
    out["dense"] = probe(D, 0.0, a.tol, a.reps, not a.no_scipy)
    print(save())


if __name__ == "__main__":
    main()
