"""eigsh on a complex Hermitian matrix against the real embedding of twice the order.  (GPU box; run by hand, not a test.)

The matrix is the Harper-Hofstadter Hamiltonian ``synthetic.hofstadter(Lx, Ly, 1/3, disorder=0.5)`` (default 2500 x 2000: n = 5e6, one
complex row of the basis is 1e7 doubles), ``k = 4``, ``which="SA"``, ``ncv = 36``, ``tol = 1e-8``, both runs bounded by ``--maxiter``
restart cycles; what converged is reported, not assumed.

    python tools/eigsh_complex_probe.py [--lx 2500 --ly 2000 --maxiter 30 --reps 5 --out FILE]      one JSON object

(a) ``extend_step_us``: one ``lz_ztrl_extend`` step at a full basis (``nb = ncv`` rows), second pass forced, and the same at smaller
    bases; the slope over ``nb`` is the cost of a row in two zdots and two zcgs walks (``64 n`` algorithmic bytes a complex row),
    reported as ``walks_frac_hbm_peak`` of 8 TB/s.  The two kernels one by one, and the product, come from the same program under
    ``rocprofv3 --kernel-trace --stats -- python tools/eigsh_complex_probe.py --steps-only`` (k_zdots, k_zcgs, k_zspmv_csr): a walk of
    ``nb`` rows moves ``16 n (nb + 1)`` (zdots) and ``16 n (nb + 2)`` (zcgs) bytes.
(c) ``residual_call_us``: ``lz_ztrl_residuals(1, ..)`` - one product, one difference-norm kernel and a synchronisation.
(d) ``embedding``: the same problem as the real symmetric ``[[R, -J], [J, R]]`` of order ``2 n`` through ``eigsh(block_size=2, k=8,
    ncv=2 ncv)`` - every eigenvalue twice, which is how a build without the complex path solves it.

Times are host wall clock around calls that end in a stream synchronisation: warm, ``--reps`` repetitions, median and spread."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import ArpackNoConvergence

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lanczos_amd import _capi, eigsh, synthetic  # noqa: E402
from lanczos_amd.eigsh import upload_complex_matrix  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def timed(fn, reps):
    fn()  # warm
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return {"median_us": float(np.median(ts)) * 1e6, "min_us": float(np.min(ts)) * 1e6, "max_us": float(np.max(ts)) * 1e6}


def steps(h, n, ncv, reps):
    """the last step of an extension (nb = m rows behind the product), second pass forced, for several m"""
    rng = np.random.default_rng(2)
    v0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h.set_options(_capi.FLAG_TRL_PASS2_ALWAYS)
    out = {}
    for m in sorted({4, 12, 20, 28, ncv}):
        h.ztrl_begin(m, v0)
        h.ztrl_extend(0, m)
        out[m] = timed(lambda: h.ztrl_extend(m - 1, m), reps)
    h.set_options(0)
    ms = np.array(sorted(out))
    slope, intercept = np.polyfit(ms, [out[m]["median_us"] for m in ms], 1)  # us per complex row in 2 zdots + 2 zcgs walks
    res = timed(lambda: h.ztrl_residuals(1, np.zeros(1)), reps)
    return {"extend_step_us": {int(m): out[m] for m in ms}, "us_per_row_two_passes": float(slope), "us_at_zero_rows": float(intercept),
            "walks_frac_hbm_peak": 64.0 * n / (slope * 1e-6) / HBM_PEAK, "residual_call_us": res}


def solve(fn, k):
    t = time.perf_counter()
    info = {}
    try:
        theta = fn(info)
        conv = len(theta)
    except ArpackNoConvergence as e:
        theta, conv, info = e.eigenvalues, len(e.eigenvalues), getattr(e, "info", {})
    return {"seconds": time.perf_counter() - t, "converged": int(conv), "wanted": k, "theta": [float(x) for x in np.atleast_1d(theta)],
            "cycles": info.get("cycles"), "matvecs": info.get("matvecs"),
            "residuals": [float(x) for x in info.get("residuals", [])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lx", type=int, default=2500)
    ap.add_argument("--ly", type=int, default=2000)
    ap.add_argument("--ncv", type=int, default=36)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    t = time.perf_counter()
    A = synthetic.hofstadter(a.lx, a.ly, 1 / 3, disorder=0.5)
    n = A.shape[0]
    out = {"n": n, "nnz": int(A.nnz), "ncv": a.ncv, "maxiter": a.maxiter, "build_s": time.perf_counter() - t}
    h = _capi.Handle(0)
    upload_complex_matrix(h, A)
    out.update(steps(h, n, a.ncv, a.reps))
    if not a.steps_only:
        k, tol = 4, 1e-8
        out["native"] = solve(lambda info: eigsh(A, k=k, which="SA", ncv=a.ncv, tol=tol, maxiter=a.maxiter, handle=h, info=info,
                                                 return_eigenvectors=False), k)
        h.close()
        R, J = A.real.tocsr(), A.imag.tocsr()
        R.eliminate_zeros()  # (the x-bonds have no imaginary part, the y-bonds at x = 0 mod 3 neither)
        J.eliminate_zeros()
        E =sp.bmat([[R, -J], [J, R]], format="csr")
        del R, J
        h = _capi.Handle(0)
        out["embedding"] = solve(lambda info: eigsh(E, k=2 * k, which="SA", ncv=2 * a.ncv, tol=tol, maxiter=a.maxiter, handle=h, info=info,
                                                    block_size=2, return_eigenvectors=False), 2 * k)
        out["native_over_embedding_seconds"] = out["native"]["seconds"] / out["embedding"]["seconds"]
        for key in ("native", "embedding"):
            if out[key]["cycles"]:
                out[key]["seconds_per_cycle"] = out[key]["seconds"] / out[key]["cycles"]
    h.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
