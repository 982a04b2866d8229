"""expm_multiply's mixed route (real matrix, Schroedinger time) piece by piece.  (GPU box; run by hand, not a test.)

    python tools/expm_probe.py [--nx 4000 --ny 2500 --dense 16384 --ncv 30 --reps 5 --out FILE]      one JSON object

Four matrices: the periodic 5-point Laplacian on ``nx x ny`` (default n = 1e7; its SpMV is the row-class coded stencil kernel), two
with rows of unequal length whose SpMV is the CSR-stream kernel - the real part of the ``gx x gy`` Hofstadter lattice with open
boundaries (n = 3e6, 4 entries in most rows) and a symmetric band of 33 entries per row (n = 1e6) - and a dense random symmetric matrix
of order ``--dense``.  For each:

(a) ``product_us``: the product of the real matrix with a planar complex vector in its forms, device time by events
    (``lz_expm_product_time``: the mean of 20 launches behind a warm-up, repeated ``--reps`` times, median and spread).  Laplacian:
    ``two_plane`` (k_spmv_csr_z2 on the plain CSR arrays), ``two_launch_coded`` (two launches of the coded stencil kernel: what the
    automatic rule runs there) and ``two_launch_uncoded`` (knob 17 = 1: two launches of the CSR-order fixed-K kernel).  Dense:
    ``two_plane`` (k_gemv_z2) and ``two_launch`` (k_gemv_dense twice).  ``bytes`` are the algorithmic bytes of the accounting in
    DESIGN.md section 8e and ``frac_hbm_peak`` their rate over 8 TB/s.
(b) ``step_us``: one ``lz_expm_extend`` step at a full basis (``ncv`` rows behind the product), host clock around a call that ends in
    a synchronisation; ``gram_schmidt_us`` is that minus the product of the automatic form.
(c) ``combine_us``: ``lz_expm_combine`` of ``ncv`` rows into 2 (the new state and one output) with the normalisation of row 0.
(d) ``run``: ``expm_multiply(a=-1j)`` to the time ``--t`` (chosen for about ten substeps at ``ncv = 30``), wall clock with the upload
    of the matrix, and the substeps it took."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lanczos_amd import _capi, expm_multiply, synthetic  # noqa: E402
from lanczos_amd.eigsh import upload_matrix  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def stats(ts):
    return {"median_us": float(np.median(ts)), "min_us": float(np.min(ts)), "max_us": float(np.max(ts))}


def host_timed(fn, reps):
    fn()  # warm
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e6)
    return stats(ts)


def product(h, reps, nbytes):
    out = stats([h.expm_product_time(20) * 1e3 for _ in range(reps)])
    out["bytes"] = float(nbytes)
    out["frac_hbm_peak"] = nbytes / (out["median_us"] * 1e-6) / HBM_PEAK
    out["form"] = h.expm_info()["product"]
    return out


def pieces(h, n, ncv, reps, forms, auto):
    """``forms``: {name: (form of ``expm_set_product``, algorithmic bytes)} for the matrix on the handle; ``auto``: the name the automatic rule runs"""
    rng = np.random.default_rng(2)
    v0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    out = {"product_us": {}}
    h.expm_begin(ncv, v0, True)
    for name, (knob, nbytes) in forms.items():
        h.expm_set_product(knob)
        out["product_us"][name] = product(h, reps, nbytes)
    h.expm_set_product(0)
    h.expm_extend(0, ncv)
    out["step_us"] = host_timed(lambda: h.expm_extend(ncv - 1, ncv), reps)
    out["gram_schmidt_us"] = out["step_us"]["median_us"] - out["product_us"][auto]["median_us"]
    C = rng.standard_normal((ncv, 2)) + 1j * rng.standard_normal((ncv, 2))

    def combine():
        h.expm_extend(0, 1)  # (keeps the rows finite and of order one; its time is taken off below)
        h.expm_combine(ncv, C)

    both = host_timed(combine, reps)
    first = host_timed(lambda: h.expm_extend(0, 1), reps)
    out["combine_us"] = {k: both[k] - first["median_us"] for k in both}
    return out


def run(A, n, t, ncv, tol):
    b = np.random.default_rng(3).standard_normal(n)
    info = {}
    t0 = time.perf_counter()
    out = expm_multiply(A, b, start=t, stop=t, num=1, a=-1j, ncv=ncv, tol=tol, info=info)
    sec = time.perf_counter() - t0
    nb = np.linalg.norm(b)
    return {"t": t, "tol": tol, "seconds_with_upload": sec, "substeps": info["substeps"], "matvecs": info["matvecs"], "product": info["product"],
            "err_est": info["err_est"], "norm_drift": float(abs(np.linalg.norm(out) - nb) / nb)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4000)
    ap.add_argument("--ny", type=int, default=2500)
    ap.add_argument("--dense", type=int, default=16384)
    ap.add_argument("--gx", type=int, default=2000)
    ap.add_argument("--gy", type=int, default=1500)
    ap.add_argument("--ncv", type=int, default=30)
    ap.add_argument("--t", type=float, default=25.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {"ncv": a.ncv}

    L = synthetic.laplacian_2d_5pt(a.nx, a.ny)
    n, nnz = L.shape[0], L.nnz
    lap = {"n": n, "nnz": nnz}
    # per row: 5 values + 5 indices + a row pointer, 2 vector reads (the gathers hit in cache) and 2 stores for both planes at once;
    # one launch of the real product: the same matrix stream, 1 read and 1 store; the coded stream is a byte per row
    two_plane = nnz * 12.0 + n * (4.0 + 32.0)
    uncoded = 2 * (nnz * 12.0 + n * (4.0 + 16.0))
    coded = 2 * n * (1.0 + 16.0)
    h = _capi.Handle(0)
    upload_matrix(h, L)
    lap["spmv_coding"] = list(h.spmv_coding())
    lap.update(pieces(h, n, a.ncv, a.reps, {"two_plane": (2, two_plane), "two_launch_coded": (1, coded)}, "two_launch_coded"))
    h.close()
    h = _capi.Handle(0)
    h.set_tuning(_capi.TUNE_FIXED_LAYOUT, 1)  # never ELL: the CSR-order fixed-K kernel
    upload_matrix(h, L)
    rng = np.random.default_rng(2)
    h.expm_begin(a.ncv, rng.standard_normal(n) + 1j * rng.standard_normal(n), True)
    h.expm_set_product(1)
    lap["product_us"]["two_launch_uncoded"] = product(h, a.reps, uncoded)
    h.expm_set_product(0)
    h.expm_product_time(1)
    lap["auto_without_coding"] = h.expm_info()["product"]  # what the automatic rule runs on the uncoded matrix
    h.close()
    lap["run"] = run(L, n, a.t, a.ncv, 1e-10)
    out["laplacian"] = lap

    # matrices with rows of unequal length, whose real SpMV is the CSR-stream kernel: the real part of a Hofstadter lattice with open
    # boundaries (about 4 entries per row) and a symmetric band with 33 entries per row
    import scipy.sparse as sp

    H = sp.csr_matrix(synthetic.hofstadter(a.gx, a.gy, 1 / 8).real)
    rng = np.random.default_rng(5)
    nb = a.gx * a.gy // 3
    offs = list(range(1, 17))
    B = sp.diags([rng.standard_normal(nb - o) for o in offs], offs, format="csr")
    B = sp.csr_matrix(B + B.T + sp.diags(rng.standard_normal(nb)))
    for name, M in (("hofstadter_real", H), ("band33", B)):
        M.sort_indices()
        gn, gnnz = M.shape[0], M.nnz
        rec = {"n": gn, "nnz": int(gnnz)}
        h = _capi.Handle(0)
        upload_matrix(h, M)
        rec["group"] = h.expm_info()["group"]
        rec["spmv_plan"] = h.spmv_plan()
        forms = {"two_plane": (2, gnnz * 12.0 + gn * (4.0 + 32.0)), "two_launch": (1, 2 * (gnnz * 12.0 + gn * (4.0 + 16.0)))}
        h.expm_set_product(0)
        h.expm_begin(a.ncv, rng.standard_normal(gn) + 1j * rng.standard_normal(gn), True)
        h.expm_product_time(1)
        auto = {"two-plane": "two_plane", "two-launch": "two_launch"}[h.expm_info()["product"]]
        rec["auto"] = auto
        rec.update(pieces(h, gn, a.ncv, a.reps, forms, auto))
        h.close()
        out[name] = rec

    # the two forms on symmetric bands of 3 .. 65 entries per row (about 3.2e7 entries each; the end rows are shorter, so the real SpMV
    # is the CSR-stream kernel): where the group kernel of 2 .. 64 lanes per row stops paying
    sweep = {}
    for per_row in (3, 5, 9, 17, 33, 65):
        ns = 32_000_000 // per_row
        offs = list(range(1, per_row // 2 + 1))
        M = sp.diags([rng.standard_normal(ns - o) for o in offs], offs, format="csr")
        M = sp.csr_matrix(M + M.T + sp.diags(rng.standard_normal(ns)))
        M.sort_indices()
        h = _capi.Handle(0)
        upload_matrix(h, M)
        h.expm_begin(2, rng.standard_normal(ns) + 1j * rng.standard_normal(ns), True)
        rec = {"n": ns, "nnz": int(M.nnz), "group": h.expm_info()["group"], "spmv_plan": h.spmv_plan()}
        for name, knob, nbytes in (("two_plane", 2, M.nnz * 12.0 + ns * 36.0), ("two_launch", 1, 2 * (M.nnz * 12.0 + ns * 20.0))):
            h.expm_set_product(knob)
            rec[name] = product(h, a.reps, nbytes)
        rec["two_launch_over_two_plane"] = rec["two_launch"]["median_us"] / rec["two_plane"]["median_us"]
        h.close()
        sweep[per_row] = rec
    out["band_sweep"] = sweep

    nd = a.dense
    G = np.random.default_rng(7).standard_normal((nd, nd))
    D = (G + G.T) / np.sqrt(2.0 * nd)  # spectrum within about [-2, 2]
    del G
    den = {"n": nd}
    h = _capi.Handle(0)
    upload_matrix(h, D)
    den.update(pieces(h, nd, a.ncv, a.reps, {"two_plane": (2, 8.0 * nd * nd), "two_launch": (1, 16.0 * nd * nd)}, "two_plane"))
    h.close()
    den["run"] = run(D, nd, a.t * 4.0, a.ncv, 1e-10)
    out["dense"] = den

    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
