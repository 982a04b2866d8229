"""cg piece by piece.  (GPU box; run by hand, not a test.)

    python tools/cg_probe.py [--nx 4000 --ny 2500 --dense 16384 --reps 3 --tol 1e-8 --no-scipy --no-minres --out FILE]      one JSON object

Three matrices: ``laplacian`` - the periodic 5-point Laplacian of the ``nx x ny`` grid with diagonal 4.05, the system ``minres`` was
measured on (its Laplacian shifted by -0.05; row-class coded on the device) -, ``well`` - the same plus a potential
``10 ** uniform(-1, 3)``, four decades on the diagonal, solved without a preconditioner and with ``M="jacobi"`` - and ``dense`` - a
symmetric normal ``--dense`` matrix scaled to the spectrum ``[0.5, 2.5]``.  For each:

(a) ``parts_us``: the product and the two streaming passes of an iteration - device time by events (``lz_cg_step_time``: the mean of
    20 launches behind a warm-up, repeated ``--reps`` times, median and spread).  ``*_bytes`` are the algorithmic bytes of the
    accounting in DESIGN.md section 8j (24 / 40 per padded row, 32 / 48 with a preconditioner) and ``*_frac_hbm_peak`` their rate over
    8 TB/s.
(b) ``minres_step``: the yardstick - ``k_minres_step`` (72 B a row, the same shape) re-measured in the same run on the same length.
(c) ``iteration_us``: ``lz_cg_run`` of 64 iterations as one chunk (``atol_eff = 0``), host clock around the call, per iteration.
(d) ``solve``: ``cg`` to ``rtol = --tol`` at ``check_every`` = 8 / 32 / 128 on an open handle that holds the matrix already
    (``solve_seconds``) and once through ``cg`` itself with packing, upload and download (``end_to_end_seconds``).
(e) two labelled baselines at the same tolerance: ``minres_gpu`` - this package's own ``minres`` on the same system (iterations,
    seconds, true residual) - and ``scipy_cpu`` - ``scipy.sparse.linalg.cg`` with the same ``M`` on this machine's CPUs (skipped for
    the well without a preconditioner, whose thousands of iterations at this size take minutes there)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bicgstab_probe import minres_yardstick, stats  # noqa: E402

from lanczos_amd import _capi, cg, minres  # noqa: E402
from lanczos_amd.cg import DeviceCgBackend, solve  # noqa: E402
from lanczos_amd.eigsh import upload_matrix  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s
PASS_BYTES = {False: {"k_cg_r": 24, "k_cg_p": 40}, True: {"k_cg_r": 32, "k_cg_p": 48}}


def note(text):
    print(f"[cg_probe] {text}", file=sys.stderr, flush=True)


def laplacian(nx, ny, diag=4.05, potential=None):
    n = nx * ny
    idx = np.arange(n, dtype=np.int32).reshape(nx, ny)
    cols = np.stack([idx, np.roll(idx, 1, 0), np.roll(idx, -1, 0), np.roll(idx, 1, 1), np.roll(idx, -1, 1)], axis=-1).reshape(n, 5)
    vals = np.tile(np.array([diag, -1.0, -1.0, -1.0, -1.0]), (n, 1))
    if potential is not None:
        vals[:, 0] += potential
    order = np.argsort(cols, axis=1, kind="stable")
    cols, vals = np.take_along_axis(cols, order, 1), np.take_along_axis(vals, order, 1)
    return sp.csr_matrix((vals.reshape(-1), cols.reshape(-1), np.arange(0, 5 * n + 1, 5, dtype=np.int32)), shape=(n, n))


def probe(A, tol, reps, jacobi, scipy_too, minres_too):
    n = A.shape[0]
    b = np.random.default_rng(4).standard_normal(n)
    atol_eff = tol * float(np.linalg.norm(b))
    d = 1.0 / (A.diagonal() if sp.issparse(A) else np.diagonal(A)) if jacobi else None
    h = _capi.Handle(0)
    t = time.perf_counter()
    upload_matrix(h, A)
    out = {"n": n, "tol": tol, "preconditioner": "jacobi" if jacobi else None, "upload_seconds": time.perf_counter() - t, "spmv_plan": h.spmv_plan()}
    if sp.issparse(A):
        out["coding"] = h.spmv_coding()[0]
    names = ("product", "k_cg_r", "k_cg_p")
    parts = [[] for _ in names]
    for _ in range(reps):
        h.cg_begin(b, None, d)
        h.cg_run(2, 0.0)
        for acc, ms in zip(parts, h.cg_step_time(20)):
            acc.append(ms * 1e3)
    out["launches_per_iteration"] = h.cg_info()["launches_per_iteration"]
    out["parts_us"] = {name: stats(ts) for name, ts in zip(names, parts)}
    note(f"n = {n}: parts measured")
    out["parts_sum_us"] = float(sum(np.median(ts) for ts in parts))
    pad = h.padded_rows(n)
    for name, per_row in PASS_BYTES[jacobi].items():
        out[name + "_bytes"] = float(per_row * pad)
        out[name + "_frac_hbm_peak"] = per_row * pad / (out["parts_us"][name]["median_us"] * 1e-6) / HBM_PEAK
    ts = []
    for _ in range(reps + 1):
        h.cg_begin(b, None, d)
        t = time.perf_counter()
        h.cg_run(64, 0.0)
        ts.append((time.perf_counter() - t) * 1e6 / 64)
    out["iteration_us"] = stats(ts[1:])
    out["solve"] = {}
    for check_every in (8, 32, 128):
        ts, info = [], {}
        for _ in range(reps):
            t = time.perf_counter()
            x, code = solve(DeviceCgBackend(h, n), b, None, atol_eff, 10 * n, check_every, info=info, d=d)
            ts.append(time.perf_counter() - t)
        out["solve"][check_every] = {"solve_seconds": float(np.median(ts)), "min_seconds": float(np.min(ts)), "iterations": info["iterations"],
                                     "products": info["products"], "chunks": info["chunks"], "code": code, "exit": info["exit"]}
        note(f"n = {n}: check_every {check_every}: {out['solve'][check_every]}")
    h.close()
    info = {}
    t = time.perf_counter()
    x, code = cg(A, b, rtol=tol, M="jacobi" if jacobi else None, info=info)
    out["end_to_end_seconds"] = time.perf_counter() - t
    out["result"] = {"code": code, "iterations": info["iterations"], "exit": info["exit"], "indefinite_at": info["indefinite_at"],
                     "residual_norm_over_b": info["residual_norm"] / np.linalg.norm(b),
                     "true_residual_over_b": float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))}
    note(f"n = {n}: end to end {out['end_to_end_seconds']:.2f} s, {out['result']}")
    if minres_too:
        minfo = {}
        t = time.perf_counter()
        xm, cm = minres(A, b, rtol=tol, maxiter=10 * n, info=minfo)
        out["minres_gpu"] = {"seconds": time.perf_counter() - t, "code": int(cm), "iterations": minfo["iterations"],
                             "true_residual_over_b": float(np.linalg.norm(b - A @ xm) / np.linalg.norm(b))}
        note(f"n = {n}: minres {out['minres_gpu']}")
    if scipy_too:
        t = time.perf_counter()
        xs, code_s = sla.cg(A, b, rtol=tol, M=None if d is None else sp.diags(d))
        out["scipy_cpu"] = {"seconds": time.perf_counter() - t, "code": int(code_s), "threads": int(os.environ.get("OMP_NUM_THREADS", 0)),
                            "true_residual_over_b": float(np.linalg.norm(b - A @ xs) / np.linalg.norm(b)),
                            "x_diff": float(np.linalg.norm(x - xs) / np.linalg.norm(xs))}
        note(f"n = {n}: scipy {out['scipy_cpu']}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4000)
    ap.add_argument("--ny", type=int, default=2500)
    ap.add_argument("--dense", type=int, default=16384)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-minres", action="store_true")
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
    out["laplacian"] = probe(laplacian(a.nx, a.ny), a.tol, a.reps, False, not a.no_scipy, not a.no_minres)
    save()
    W = laplacian(a.nx, a.ny, 4.05, 10.0 ** np.random.default_rng(7).uniform(-1.0, 3.0, a.nx * a.ny))
    out["well"] = probe(W, a.tol, a.reps, False, False, not a.no_minres)
    save()
    out["well_jacobi"] = probe(W, a.tol, a.reps, True, not a.no_scipy, False)
    save()
    n = a.dense
    G = np.random.default_rng(7).standard_normal((n, n))
    D = (G + G.T) / (2.0 * np.sqrt(2.0 * n)) + 1.5 * np.eye(n)  # the semicircle of radius 1 about 1.5
    del G
    out["dense"] = probe(np.ascontiguousarray(D), a.tol, a.reps, False, not a.no_scipy, not a.no_minres)
    print(save())


if __name__ == "__main__":
    main()
