"""What every correct Lanczos run with full re-orthogonalisation satisfies, whatever its length: beyond the stable prefix the
coefficients of a long run are not determined by the arithmetic (tests/test_gpu_one_sweep*.py compare a prefix only), so the long
runs (tests/test_one_sweep_long_host.py, tests/test_gpu_one_sweep_long.py) are held to these instead.  NumPy / SciPy float64 from
the fetched alpha, beta, basis rows V (n x M), the residual r entering step n and the test's own CSR matrix:

  orth = max |V V^T - I|                         and the first row j with max_{i <= j} |(V V^T - I)[j, i]| above the bar
  rel  = max |A V^T - V^T T - r e_{n-1}^T|       T tridiagonal from alpha and beta[:n-1]; and the first column above the bar
  ritz = the three smallest and the three largest eigenvalues of T against those of the dense A (n >= 258 on the inputs below:
         at n = 129 the extremes have not converged, 8.7e-12 in the CPU prototype against 6.5e-15 at n = 258)

and the inputs of the long runs: periodic Laplacians with perturbed off-diagonal values (the unperturbed ones have highly
degenerate spectra, their Krylov spaces run out long before n = 1000)."""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse

from lanczos_amd import synthetic

ORTH_BAR = 1e-13   # the project's bar on max |V V^T - I| (tests/test_gpu_one_sweep*.py)
COEF_BAR = 1e-12   # the project's coefficient bar, in units of the spectral scale
RITZ_MIN_N = 258


def perturbed(L, kind, amp, seed=5):
    """_perturbed_5pt of tests/test_gpu_one_sweep_fused.py on any fixed-width matrix: the off-diagonal entries changed on their own
    pattern, "values": L + amp (P + P^T), "asym": L + amp (P - P^T), P uniform in [-1, 1) from default_rng(seed)."""
    L = scipy.sparse.csr_matrix(L)
    width = np.diff(L.indptr)
    off = L.copy()
    off.setdiag(0.0)
    off.eliminate_zeros()
    P = off.copy()
    P.data = np.random.default_rng(seed).uniform(-1.0, 1.0, size=P.nnz)
    H = (L + amp * (P + P.T)) if kind == "values" else (L + amp * (P - P.T))
    H = H.tocsr()
    H.sort_indices()
    assert np.array_equal(np.diff(H.indptr), width) and np.all(width == width[0])
    return H


@functools.lru_cache(maxsize=None)
def long_matrix(name):
    if name == "values_48x40":    # 1920 rows, five entries per row
        return perturbed(synthetic.laplacian_2d_5pt(48, 40).to_scipy(), "values", 1e-3)
    if name == "values7_13x12x11":  # 1716 rows, seven entries per row
        return perturbed(synthetic.laplacian_3d_7pt(13, 12, 11).to_scipy(), "values", 1e-3)
    if name == "asym_48x40":      # a prediction that assumes A = A^T misses by ~1e-9 at every step
        return perturbed(synthetic.laplacian_2d_5pt(48, 40).to_scipy(), "asym", 1e-9)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def dense_spectrum(name):
    """eigvalsh of the dense matrix, once per input"""
    return np.linalg.eigvalsh(long_matrix(name).toarray())


def _first_above(per_index, bar):
    hit = np.flatnonzero(~(per_index <= bar))  # (a NaN is above every bar)
    return int(hit[0]) if hit.size else None


def orthogonality(V, bar=ORTH_BAR):
    """(max |V V^T - I|, the first row j whose own part of it - the entries against rows i <= j - exceeds `bar`, or None)"""
    V = np.asarray(V, dtype=np.float64)
    E = np.abs(np.tril(V @ V.T - np.eye(V.shape[0])))
    per_row = np.where(np.isnan(E).any(axis=1), np.nan, E.max(axis=1))
    return (float(per_row.max()) if not np.isnan(per_row).any() else float("nan")), _first_above(per_row, bar)


def relation_residual(A, alpha, beta, V, r):
    """per column j the max |A v_j - beta_{j-1} v_{j-1} - alpha_j v_j - beta_j v_{j+1}|, the last column with r (the residual entering
    step n) in the place of beta_{n-1} v_n"""
    alpha, beta, V = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64), np.asarray(V, dtype=np.float64)
    n = V.shape[0]
    assert alpha.shape == (n,) and beta.shape[0] >= n - 1 and np.shape(r) == (V.shape[1],)
    b = beta[: n - 1]
    R = (scipy.sparse.csr_matrix(A) @ V.T).T - alpha[:, None] * V  # row j: column j of the relation
    R[1:] -= b[:, None] * V[:-1]
    R[:-1] -= b[:, None] * V[1:]
    R[-1] -= np.asarray(r, dtype=np.float64)
    return np.abs(R).max(axis=1)


def ritz_extremes(alpha, beta, spectrum, k=3):
    """max difference of the k smallest and the k largest eigenvalues of T and of A"""
    n = len(alpha)
    if not (np.isfinite(alpha).all() and np.isfinite(np.asarray(beta)[: n - 1]).all()):
        return float("nan")
    theta = scipy.linalg.eigvalsh_tridiagonal(np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)[: n - 1])
    return float(max(np.abs(theta[:k] - spectrum[:k]).max(), np.abs(theta[-k:] - spectrum[-k:]).max()))


def invariants(A, alpha, beta, V, r, spectrum, rel_bar=None):
    """dict(orth, orth_row, rel, rel_col, per_col, ritz, scale).  `spectrum`: the ascending eigenvalues of the dense A; scale = max |lambda|.
    rel_col is the first column above `rel_bar` (default: 1e-13 of the scale, which a correct run stays a hundred times under);
    ritz is None below RITZ_MIN_N steps."""
    scale = float(np.abs(spectrum).max())
    orth, orth_row = orthogonality(V)
    per_col = relation_residual(A, alpha, beta, V, r)
    rel = float(per_col.max()) if not np.isnan(per_col).any() else float("nan")
    rel_col = _first_above(per_col, 1e-13 * scale if rel_bar is None else rel_bar)
    ritz = ritz_extremes(alpha, beta, spectrum) if len(alpha) >= RITZ_MIN_N else None
    return dict(orth=orth, orth_row=orth_row, rel=rel, rel_col=rel_col, per_col=per_col, ritz=ritz, scale=scale)


def describe(inv):
    ritz = "-" if inv["ritz"] is None else f"{inv['ritz']:.1e}"
    return f"orth {inv['orth']:.1e} rel {inv['rel']:.1e} ritz {ritz} (scale {inv['scale']:.2f})"


def assert_invariants(inv, ref_rel, what):
    """orth under the project's bar, rel within 4x of the six-launch (or two-pass) run's on the same input and n - the margin is for
    another summation order; a wrong coefficient shows at its own size -, ritz within 1e-12 of the scale"""
    assert inv["orth"] < ORTH_BAR, f"{what}: max |V V^T - I| = {inv['orth']:.2e}, first at row {inv['orth_row']}"
    first = _first_above(inv["per_col"], 4.0 * ref_rel)
    assert inv["rel"] <= 4.0 * ref_rel, f"{what}: relation residual {inv['rel']:.2e} against {ref_rel:.2e} of the reference, first at column {first}"
    if inv["ritz"] is not None:
        assert inv["ritz"] <= COEF_BAR * inv["scale"], f"{what}: extreme Ritz values off by {inv['ritz']:.2e}"
