"""minres piece by piece.  (GPU box; run by hand, not a test.)

    python tools/minres_probe.py [--nx 4000 --ny 2500 --dense 16384 --reps 5 --rtol 1e-8 --out FILE]      one JSON object

Two matrices: the periodic 5-point Laplacian on ``nx x ny`` (default n = 1e7; its SpMV is the row-class coded stencil kernel, which
scales on read: plan S) and a dense random symmetric matrix of order ``--dense`` (plan U: the product runs on the un-normalised
residual).  Both are shifted to be positive definite.  For each:

(a) ``product_us`` / ``step_us``: one product of the plan and one ``k_minres_step`` with the three-term and the lagged update, device
    time by events (``lz_minres_step_time``: the mean of 20 launches behind a warm-up, repeated ``--reps`` times, median and spread).
    ``step_bytes`` are the algorithmic bytes of the accounting in DESIGN.md section 8f (72 per padded row for plan S, 80 for plan U)
    and ``step_frac_hbm_peak`` their rate over 8 TB/s.
(b) ``iteration_us``: ``lz_minres_run`` of 64 steps as one chunk (``rtol = 0``), host clock around the call, per step.
(c) ``solve``: ``minres`` to ``--rtol`` at ``check_every`` = 8 / 32 / 128 on an open handle that holds the matrix already, wall clock,
    median of ``--reps``; the iterations and the true residual.
(d) ``scipy_cpu``: ``scipy.sparse.linalg.minres`` on the same problem and ``rtol`` on this machine's CPUs - a labelled baseline, with its
    own (weaker) stopping rule: its iterations and true residual are beside its time."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lanczos_amd import _capi, synthetic  # noqa: E402
from lanczos_amd.eigsh import upload_matrix  # noqa: E402
from lanczos_amd.minres import DeviceMinresBackend, solve  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def stats(ts):
    return {"median_us": float(np.median(ts)), "min_us": float(np.min(ts)), "max_us": float(np.max(ts))}


def probe(A, S, n, shift, rtol, reps):
    """``A``: what goes to the device, ``S``: the same matrix for SciPy and the residuals"""
    rng = np.random.default_rng(4)
    b = rng.standard_normal(n)
    nb = np.linalg.norm(b)
    h = _capi.Handle(0)
    upload_matrix(h, A)
    plan = h.minres_info()
    out = {"n": n, "shift": shift, "rtol": rtol, "scale_on_read": plan["scale_on_read"], "launches_per_iteration": plan["launches_per_iteration"]}
    pt, st = [], []
    for _ in range(reps):
        h.minres_begin(b, None, shift)
        h.minres_run(2, 0.0)
        p, s = h.minres_step_time(20)
        pt.append(p * 1e3)
        st.append(s * 1e3)
    out["product_us"], out["step_us"] = stats(pt), stats(st)
    out["step_bytes"] = float((72 if plan["scale_on_read"] else 80) * h.padded_rows(n))
    out["step_frac_hbm_peak"] = out["step_bytes"] / (out["step_us"]["median_us"] * 1e-6) / HBM_PEAK
    ts = []
    for _ in range(reps + 1):
        h.minres_begin(b, None, shift)
        t = time.perf_counter()
        h.minres_run(64, 0.0)
        ts.append((time.perf_counter() - t) * 1e6 / 64)
    out["iteration_us"] = stats(ts[1:])
    out["solve"] = {}
    for check_every in (8, 32, 128):
        ts, info = [], {}
        for _ in range(reps):
            t = time.perf_counter()
            x, code = solve(DeviceMinresBackend(h, n), b, None, shift, rtol, 5 * n, check_every, info=info)
            ts.append(time.perf_counter() - t)
        res = float(np.linalg.norm(b - (S @ x - shift * x)) / nb)
        out["solve"][check_every] = {"seconds": float(np.median(ts)), "min_seconds": float(np.min(ts)), "iterations": info["iterations"],
                                     "chunks": info["chunks"], "info": code, "residual_over_b": res}
    h.close()
    it = [0]

    def count(_):
        it[0] += 1

    t = time.perf_counter()
    xs, code = sla.minres(S, b, shift=shift, rtol=rtol, callback=count)
    sec = time.perf_counter() - t
    out["scipy_cpu"] = {"seconds": sec, "iterations": it[0], "info": int(code), "residual_over_b": float(np.linalg.norm(b - (S @ xs - shift * xs)) / nb),
                        "threads": int(os.environ.get("OMP_NUM_THREADS", 0))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4000)
    ap.add_argument("--ny", type=int, default=2500)
    ap.add_argument("--dense", type=int, default=16384)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {}

    L = synthetic.laplacian_2d_5pt(a.nx, a.ny)
    S = sp.csr_matrix(L.to_scipy())
    # semi-definite either way round: a shift of 0.05 past the null end makes it definite, condition number about 160
    shift = -0.05 * float(np.sign(S[0, 0]))
    out["laplacian"] = probe(L, S, S.shape[0], shift, a.rtol, a.reps)
    del L, S

    nd = a.dense
    G = np.random.default_rng(7).standard_normal((nd, nd))
    D = (G + G.T) / np.sqrt(2.0 * nd)  # spectrum within about [-2, 2]
    del G
    out["dense"] = probe(D, D, nd, -2.1, a.rtol, a.reps)

    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
