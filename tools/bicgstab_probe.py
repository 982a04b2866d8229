"""bicgstab piece by piece.  (GPU box; run by hand, not a test.)

    python tools/bicgstab_probe.py [--nx 4000 --ny 2500 --dense 16384 --reps 3 --tol 1e-8 --no-scipy --no-lsmr --out FILE]      one JSON object

Two matrices: the periodic 5-point convection-diffusion stencil of the ``nx x ny`` grid (diagonal ``4 + shift``, west ``-1 - cx``,
east ``-1 + cx``, south ``-1 - cy``, north ``-1 + cy`` with ``cx = 0.6, cy = -0.3, shift = 0.05``; row-class coded on the device) and a
dense normal ``--dense`` matrix plus ``2 sqrt(n) I`` (the spectrum fills a disc of radius ``sqrt(n)``: with ``sqrt(n) I`` alone it
touches the origin and BiCGSTAB, SciPy's included, breaks down with -10).  For each:

(a) ``parts_us``: the two products and the four streaming passes of an iteration - device time by events (``lz_bicgstab_step_time``:
    the mean of 20 launches behind a warm-up, repeated ``--reps`` times, median and spread).  ``*_bytes`` are the algorithmic bytes
    of the accounting in DESIGN.md section 8h (32 / 24 / 8 / 56 per padded row) and ``*_frac_hbm_peak`` their rate over 8 TB/s.
(b) ``minres_step``: the yardstick - ``k_minres_step`` (72 B a row, the same shape) re-measured in the same run on the same length
    (the 5-point Laplacian of the same grid; the stencil workload only).
(c) ``iteration_us``: ``lz_bicgstab_run`` of 64 iterations as one chunk (``atol_eff = 0``), host clock around the call, per iteration.
(d) ``solve``: ``bicgstab`` to ``rtol = --tol`` at ``check_every`` = 8 / 32 / 128 on an open handle that holds the matrix already
    (``solve_seconds``) and once through ``bicgstab`` itself with packing, upload and download (``end_to_end_seconds``).
(e) two labelled baselines at the same tolerance: ``scipy_cpu`` - ``scipy.sparse.linalg.bicgstab`` on this machine's CPUs - and
    ``lsmr_gpu`` - this package's own ``lsmr`` on the same system (iterations, seconds, true residual)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lanczos_amd import _capi, bicgstab, lsmr, synthetic  # noqa: E402
from lanczos_amd.bicgstab import DeviceBicgstabBackend, solve  # noqa: E402
from lanczos_amd.eigsh import upload_matrix  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s
PASS_BYTES = {"k_bicgstab_p": 32, "k_bicgstab_s": 24, "k_bicgstab_tt": 8, "k_bicgstab_r": 56}


def note(text):
    print(f"[bicgstab_probe] {text}", file=sys.stderr, flush=True)


def stats(ts):
    return {"median_us": float(np.median(ts)), "min_us": float(np.min(ts)), "max_us": float(np.max(ts))}


def convdiff(nx, ny, cx=0.6, cy=-0.3, shift=0.05):
    n = nx * ny
    idx = np.arange(n, dtype=np.int32).reshape(nx, ny)
    cols = np.stack([idx, np.roll(idx, 1, 0), np.roll(idx, -1, 0), np.roll(idx, 1, 1), np.roll(idx, -1, 1)], axis=-1).reshape(n, 5)
    vals = np.tile(np.array([4.0 + shift, -1.0 - cx, -1.0 + cx, -1.0 - cy, -1.0 + cy]), (n, 1))
    order = np.argsort(cols, axis=1, kind="stable")
    cols, vals = np.take_along_axis(cols, order, 1), np.take_along_axis(vals, order, 1)
    return sp.csr_matrix((vals.reshape(-1), cols.reshape(-1), np.arange(0, 5 * n + 1, 5, dtype=np.int32)), shape=(n, n))


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


def probe(A, tol, reps, scipy_too, lsmr_too):
    n = A.shape[0]
    b = np.random.default_rng(4).standard_normal(n)
    atol_eff = tol * float(np.linalg.norm(b))
    h = _capi.Handle(0)
    t = time.perf_counter()
    upload_matrix(h, A)
    out = {"n": n, "tol": tol, "upload_seconds": time.perf_counter() - t, "plan": h.bicgstab_info()}
    if sp.issparse(A):
        out["coding"] = h.spmv_coding()[0]
    names = ("product_v", "product_t", "k_bicgstab_p", "k_bicgstab_s", "k_bicgstab_tt", "k_bicgstab_r")
    parts = [[] for _ in names]
    for _ in range(reps):
        h.bicgstab_begin(b)
        h.bicgstab_run(2, 0.0)
        for acc, ms in zip(parts, h.bicgstab_step_time(20)):
            acc.append(ms * 1e3)
    out["parts_us"] = {name: stats(ts) for name, ts in zip(names, parts)}
    note(f"n = {n}: parts measured")
    out["parts_sum_us"] = float(sum(np.median(ts) for ts in parts))
    pad = h.padded_rows(n)
    for name, per_row in PASS_BYTES.items():
        out[name + "_bytes"] = float(per_row * pad)
        out[name + "_frac_hbm_peak"] = per_row * pad / (out["parts_us"][name]["median_us"] * 1e-6) / HBM_PEAK
    ts = []
    for _ in range(reps + 1):
        h.bicgstab_begin(b)
        t = time.perf_counter()
        h.bicgstab_run(64, 0.0)
        ts.append((time.perf_counter() - t) * 1e6 / 64)
    out["iteration_us"] = stats(ts[1:])
    out["solve"] = {}
    for check_every in (8, 32, 128):
        ts, info = [], {}
        for _ in range(reps):
            t = time.perf_counter()
            x, code = solve(DeviceBicgstabBackend(h, n), b, None, atol_eff, 10 * n, check_every, info=info)
            ts.append(time.perf_counter() - t)
        out["solve"][check_every] = {"solve_seconds": float(np.median(ts)), "min_seconds": float(np.min(ts)), "iterations": info["iterations"],
                                     "products": info["products"], "chunks": info["chunks"], "code": code, "exit": info["exit"]}
        note(f"n = {n}: check_every {check_every}: {out['solve'][check_every]}")
    h.close()
    info = {}
    t = time.perf_counter()
    x, code = bicgstab(A, b, rtol=tol, info=info)
    out["end_to_end_seconds"] = time.perf_counter() - t
    out["result"] = {"code": code, "iterations": info["iterations"], "exit": info["exit"], "residual_norm_over_b": info["residual_norm"] / np.linalg.norm(b),
                     "true_residual_over_b": float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))}
    note(f"n = {n}: end to end {out['end_to_end_seconds']:.2f} s, {out['result']}")
    if lsmr_too:
        t = time.perf_counter()
        res = lsmr(A, b, atol=tol, btol=tol, maxiter=20 * n)
        out["lsmr_gpu"] = {"seconds": time.perf_counter() - t, "iterations": int(res[2]), "products": 2 * int(res[2]), "istop": int(res[1]),
                           "true_residual_over_b": float(np.linalg.norm(b - A @ res[0]) / np.linalg.norm(b))}
        note(f"n = {n}: lsmr {out['lsmr_gpu']}")
    if scipy_too:
        t = time.perf_counter()
        xs, code_s = sla.bicgstab(A, b, rtol=tol)
        out["scipy_cpu"] = {"seconds": time.perf_counter() - t, "code": int(code_s), "threads": int(os.environ.get("OMP_NUM_THREADS", 0)),
                            "true_residual_over_b": float(np.linalg.norm(b - A @ xs) / np.linalg.norm(b)),
                            "x_diff": float(np.linalg.norm(x - xs) / np.linalg.norm(xs))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4000)
    ap.add_argument("--ny", type=int, default=2500)
    ap.add_argument("--dense", type=int, default=16384)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-lsmr", action="store_true")
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
    out["convdiff"] = probe(convdiff(a.nx, a.ny), a.tol, a.reps, not a.no_scipy, not a.no_lsmr)
    save()
    n = a.dense
    D = np.random.default_rng(7).standard_normal((n, n)) + 2.0 * np.sqrt(n) * np.eye(n)
    out["dense"] = probe(D, a.tol, a.reps, not a.no_scipy, not a.no_lsmr)
    print(save())


if __name__ == "__main__":
    main()
