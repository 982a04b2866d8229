"""gmres piece by piece.  (GPU box; run by hand, not a test.)

    python tools/gmres_probe.py [--nx 4000 --ny 2500 --dense 16384 --reps 3 --tol 1e-8 --scipy-cycles 1 --no-scipy --out FILE]      one JSON object

Two matrices, the ``bicgstab`` probe's: the periodic 5-point convection-diffusion stencil of the ``nx x ny`` grid (``cx = 0.6,
cy = -0.3, shift = 0.05``; row-class coded on the device) and a dense normal ``--dense`` matrix plus ``2 sqrt(n) I``.  For each, at
``restart`` 20 and 40:

(a) ``parts_us[cols]`` at ``cols`` = 1, ``restart / 2`` and ``restart``: the product ``A V[cols - 1]``, the Gram-Schmidt step against
    ``cols`` rows (both passes), ``k_gmres_update``, ``launch_trl_cgs`` at the same row count - the bar: it moves the same
    ``(cols + 2) 8`` bytes a row - and ``k_gmres_residual`` (24 bytes a row); device time by events (``lz_gmres_step_time``: the mean of
    20 launches behind a warm-up, repeated ``--reps`` times, median and spread), the update's and the bar's rate over 8 TB/s.  (The
    state with ``cols == restart`` is measured on a basis one row longer, since the step that makes the last column ends the cycle.)
(b) ``minres_step``: the yardstick - ``k_minres_step`` (72 B a row) re-measured in the same run on the same length (stencil only).
(c) ``step_us``: ``lz_gmres_run`` of two whole cycles as one chunk (``atol_eff = 0``), host clock around the call, per inner step.
(d) ``solve``: to ``rtol = --tol`` at ``check_every`` = 4 / 8 / ``restart`` on an open handle that holds the matrix already, and once
    through ``gmres`` itself with packing, upload and download (``end_to_end_seconds``), with the true residual.
(e) two labelled baselines at the same tolerance: ``bicgstab_gpu`` - this package's own ``bicgstab`` on the same system - and
    ``scipy_cpu`` - ``scipy.sparse.linalg.gmres`` on this machine's CPUs (``OMP_NUM_THREADS`` threads); on the stencil it is cut off
    after ``--scipy-cycles`` cycles (a whole solve is hundreds of inner steps of modified Gram-Schmidt on 10^7 rows in NumPy) and reports seconds per inner step."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bicgstab_probe import convdiff, minres_yardstick, stats  # noqa: E402

from lanczos_amd import _capi, bicgstab, gmres  # noqa: E402
from lanczos_amd.eigsh import upload_matrix  # noqa: E402
from lanczos_amd.gmres import DeviceGmresBackend, solve  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s
NAMES = ("product", "gram_schmidt_step", "k_gmres_update", "launch_trl_cgs", "k_gmres_residual")


def note(text):
    print(f"[gmres_probe] {text}", file=sys.stderr, flush=True)


def parts(h, b, restart, cols, reps, pad):
    acc = [[] for _ in NAMES]
    for _ in range(reps):
        h.gmres_begin(restart if cols < restart else min(restart + 1, 128), b)
        st = h.gmres_run(cols, 0.0)
        assert st["cols"] == cols and not st["inner"] and not st["done"]
        for a, ms in zip(acc, h.gmres_step_time(20)):
            a.append(ms * 1e3)
    out = {name: stats(ts) for name, ts in zip(NAMES, acc)}
    moved = float((cols + 2) * 8 * pad)
    out["update_bytes"] = moved
    for name in ("k_gmres_update", "launch_trl_cgs"):
        out[name + "_frac_hbm_peak"] = moved / (out[name]["median_us"] * 1e-6) / HBM_PEAK
    out["k_gmres_residual_frac_hbm_peak"] = 24.0 * pad / (out["k_gmres_residual"]["median_us"] * 1e-6) / HBM_PEAK
    out["update_over_trl_cgs"] = out["k_gmres_update"]["median_us"] / out["launch_trl_cgs"]["median_us"]
    return out


def probe(out, save, A, tol, reps, scipy_cycles):
    n = A.shape[0]
    b = np.random.default_rng(4).standard_normal(n)
    bnorm = float(np.linalg.norm(b))
    atol_eff = tol * bnorm
    h = _capi.Handle(0)
    t = time.perf_counter()
    upload_matrix(h, A)
    out.update({"n": n, "tol": tol, "upload_seconds": time.perf_counter() - t, "plan": h.gmres_info()})
    if sp.issparse(A):
        out["coding"] = h.spmv_coding()[0]
    pad = h.padded_rows(n)
    for restart in (20, 40):
        r = out[f"restart_{restart}"] = {"parts_us": {}}
        for cols in (1, restart // 2, restart):
            r["parts_us"][cols] = parts(h, b, restart, cols, reps, pad)
        note(f"n = {n} restart {restart}: parts measured")
        ts = []
        for _ in range(reps + 1):
            h.gmres_begin(restart, b)
            t = time.perf_counter()
            h.gmres_run(2 * restart, 0.0)
            ts.append((time.perf_counter() - t) * 1e6 / (2 * restart))
        r["step_us"] = stats(ts[1:])
        r["solve"] = {}
        for check_every in (4, 8, restart):
            ts, info = [], {}
            for _ in range(reps):
                t = time.perf_counter()
                x, code = solve(DeviceGmresBackend(h, n), b, None, atol_eff, restart, 10 * n, check_every, bnorm=bnorm, info=info)
                ts.append(time.perf_counter() - t)
            r["solve"][check_every] = {"solve_seconds": float(np.median(ts)), "min_seconds": float(np.min(ts)), "max_seconds": float(np.max(ts)),
                                       "iterations": info["iterations"], "cycles": info["cycles"], "products": info["products"],
                                       "chunks": info["chunks"], "code": code, "exit": info["exit"],
                                       "true_residual_over_b": float(np.linalg.norm(b - A @ x) / bnorm)}
            note(f"n = {n} restart {restart}: check_every {check_every}: {r['solve'][check_every]}")
        save()
    h.close()
    info = {}
    t = time.perf_counter()
    x, code = gmres(A, b, rtol=tol, info=info)
    out["end_to_end_seconds"] = time.perf_counter() - t
    out["result"] = {"code": code, "iterations": info["iterations"], "cycles": info["cycles"], "exit": info["exit"],
                     "residual_norm_over_b": info["residual_norm"] / bnorm, "true_residual_over_b": float(np.linalg.norm(b - A @ x) / bnorm)}
    note(f"n = {n}: end to end {out['end_to_end_seconds']:.2f} s, {out['result']}")
    binfo = {}
    t = time.perf_counter()
    xb, cb = bicgstab(A, b, rtol=tol, info=binfo)
    out["bicgstab_gpu"] = {"seconds": time.perf_counter() - t, "code": cb, "iterations": binfo["iterations"], "products": binfo["products"],
                           "true_residual_over_b": float(np.linalg.norm(b - A @ xb) / bnorm)}
    note(f"n = {n}: bicgstab {out['bicgstab_gpu']}")
    save()
    if scipy_cycles is not None:
        pr = []
        t = time.perf_counter()
        xs, code_s = sla.gmres(A, b, rtol=tol, maxiter=scipy_cycles if scipy_cycles > 0 else None, callback=pr.append, callback_type="pr_norm")
        sec = time.perf_counter() - t
        out["scipy_cpu"] = {"seconds": sec, "code": int(code_s), "cut_off_after_cycles": scipy_cycles if scipy_cycles > 0 else None,
                            "inner_steps": len(pr), "seconds_per_inner_step": sec / max(len(pr), 1),
                            "threads": int(os.environ.get("OMP_NUM_THREADS", 0)),
                            "true_residual_over_b": float(np.linalg.norm(b - A @ xs) / bnorm)}
        note(f"n = {n}: scipy {out['scipy_cpu']}")
    save()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4000)
    ap.add_argument("--ny", type=int, default=2500)
    ap.add_argument("--dense", type=int, default=16384)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scipy-cycles", type=int, default=1)
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
    out["convdiff"] = {}
    probe(out["convdiff"], save, convdiff(a.nx, a.ny), a.tol, a.reps, None if a.no_scipy else a.scipy_cycles)
    n = a.dense
    D = np.random.default_rng(7).standard_normal((n, n)) + 2.0 * np.sqrt(n) * np.eye(n)
    out["dense"] = {}
    probe(out["dense"], save, D, a.tol, a.reps, None if a.no_scipy else 0)
    print(save())


if __name__ == "__main__":
    main()
