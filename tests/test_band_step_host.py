"""The cases of the band extension step (``lz_trl_extend_band``) and, without a GPU, what makes them worth running: for every case the
longdouble reference's bounds (tests/band_reference.py) are small against ``|w|``, the second block pass is large where the rows are
skewed (a dropped, doubled or misplaced pass shows) and vanishes where they are orthonormal, a float64 restatement of the device's
order of operations lies within the bounds, and four planted errors in that restatement do not.
tests/test_gpu_band_step.py imports ``BAND_CASES``, ``inputs`` and ``errors``.

Matrix and rows are those of tests/test_arnoldi_step_host.py (``matrix``, ``make_rows``): ``orth`` rows are orthonormal, ``skew`` rows are
``M Q`` and are not, so the second pass has coefficients of a few hundredths of ``|w|`` to find.  ``thin`` (rows drawn on ``1 / thin`` of
the positions before they are made orthonormal) is set per shape so that the cap below holds from the reference alone.

``NumpyBackend.extend_band`` is held to the bounds on ``orth`` rows only.  It projects on the old and the new rows in one pass, which on
rows that are not orthonormal is another operator than the device's block passes followed by the tail: for ``skew`` rows it is not
expected within the bounds and is not tested.
"""
import collections
import functools

import numpy as np
import pytest
from arnoldi_reference import padded
from band_reference import extension, worst
from test_arnoldi_step_host import make_rows, matrix

from lanczos_amd.eigsh import NumpyBackend

Case = collections.namedtuple("Case", "n k m b kind thin", defaults=(1,))
CAP = 1e-8  # of |w|: every bound of every step (the Arnoldi step's is 1e-9; the band step adds the two tail passes over dense new rows)
WIDTHS = (2, 3, 4, 5, 6, 7, 8)
LONG = 262145  # pads to 262176, one padding unit past rows_pad / 2 >= 256 * 2 * 256: the first row length of k_trl_band_update<B, 2, 4>
LDS_K = (120, 121, 127)  # b = 8, m = 128: r0 = 128 (65 536 bytes of LDS, the last launch without the attribute), 129 (nb = 7), 135 (nb = 1)
SECOND_TRIP = [(1048609, 1, 5, 4, "orth", 64), (524289, 0, 8, 8, "orth", 64)]  # NG = 1: 1025 slices of 1024; NG = 2: 1025 of 512


def _cases():
    out = []
    for b in WIDTHS:  # a. every width, one full batch, ragged row tiles (r0 = 13)
        out += [Case(1501, 13 - b, 13, b, "skew"), Case(1501, 13 - b, 13, b, "orth")]
    for b in WIDTHS:  # b. every width at the first long-row length of the update kernel
        out.append(Case(LONG, 13 - b, 13, b, "skew", 32))
    for r0 in (7, 8, 9, 16, 17):  # c. tile edges of the dots walk: T = 2, eight rows per trip, clamped duplicates
        out += [Case(257, r0 - 3, r0, 3, "skew"), Case(257, r0 - 5, r0, 5, "skew")]
    out += [Case(40, 0, 2, 2, "skew"), Case(257, 0, 8, 8, "skew")]  # d. three of four waves idle; one exact tile, no clamp
    for k in LDS_K:  # e. LDS at and past 64 KiB
        out.append(Case(1501, k, 128, 8, "skew", 16))
    out.append(Case(1501, 121, 128, 8, "orth", 16))
    for k, m, b in ((3, 20, 6), (2, 12, 7), (4, 12, 3)):  # f. several batches in one call, a short last one (stale work vectors swept along)
        out.append(Case(1501, k, m, b, "skew"))
    out += [Case(*c) for c in SECOND_TRIP]  # g. the persistent second trip, its slice the ragged last one
    assert len(set(out)) == len(out)
    return out


BAND_CASES = _cases()
PLANT_CASES = [Case(1501, 13 - b, 13, b, "skew") for b in (5, 7)]


def case_id(c):
    return f"{c.n}-k{c.k}-m{c.m}-b{c.b}-{c.kind}" + (f"-thin{c.thin}" if c.thin > 1 else "")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """``(A, rows)`` of a case, computed once and never changed: the ``k + b`` rows the call starts from"""
    A = matrix(case.n)
    rows = make_rows(A, case.k + case.b, case.kind, 1, case.thin)
    rows.setflags(write=False)
    return A, rows


def restate(A, rows, k, m, b, plant=None):
    """the device's order in float64: per batch the products into the ``b`` work vectors (a short last batch sweeps the stale ones
    along), two block passes of all ``b`` against ``V[:r0]``, then per step the two tail passes and ``v = w / |w|``.  ``plant``: one of
    ``PLANTS``.  Returns ``(proj, beta, V)``."""
    n = A.shape[0]
    V = np.zeros((m + b, n))
    V[: k + b] = rows
    proj, beta, W = np.zeros((m, m + b)), np.zeros(m), np.zeros((b, n))
    for j in range(k, m, b):
        nb, r0 = min(b, m - j), j + b
        for i in range(nb):
            W[i] = A @ V[j + i]
        for _ in range(1 if plant == "pass 2 dropped" else 2):
            C = V[:r0] @ W.T  # (r0, b)
            if plant == "columns swapped":
                C[:, [1, 2]] = C[:, [2, 1]]
            if plant == "row r0 - 1 left out":
                C[r0 - 1] = 0.0
            U = C.T @ V[:r0]
            if plant == "update of the last vector skipped":
                U[b - 1] = 0.0
            W -= U
            proj[j: j + nb, :r0] += C.T[:nb]
        for i in range(nb):
            for _ in range(2 if i else 0):
                c = V[r0: r0 + i] @ W[i]
                W[i] -= c @ V[r0: r0 + i]
                proj[j + i, r0: r0 + i] += c
            beta[j + i] = np.linalg.norm(W[i])
            V[r0 + i] = W[i] / beta[j + i]
    return proj, beta, V


PLANTS = ("pass 2 dropped", "columns swapped", "update of the last vector skipped", "row r0 - 1 left out")


def errors(case, ref, proj, beta, V):
    """error over bound of ``proj[k:]``, ``beta[k:]`` and the new rows against a reference evaluated on ``V``"""
    k, n = case.k, case.n
    return {"proj": worst(np.abs(proj[k:] - ref["proj"][k:]), ref["e_proj"][k:]), "beta": worst(np.abs(beta[k:] - ref["beta"][k:]), ref["e_beta"][k:]),
            "v": worst(np.abs(V[k + case.b:, :n] - ref["rows"]), ref["e_v"])}


def figures(case, ref):
    """the bounds over ``|w|`` (worst step) and the smallest and largest ``max|c2| / |w|`` over the steps"""
    k, wn = case.k, ref["w_norm"][case.k:]
    c2 = ref["c2"][k:] / wn
    return (f"{case_id(case):34s} e_proj/|w| {(ref['e_proj'][k:].max(axis=1) / wn).max():.2e} e_beta/|w| {(ref['e_beta'][k:] / wn).max():.2e} "
            f"|e_v|beta/|w| {(np.linalg.norm(ref['e_v'], axis=1) * ref['beta'][k:] / wn).max():.2e} max|c2|/|w| {c2.min():.2e} .. {c2.max():.2e}")


@functools.lru_cache(maxsize=None)
def restated(case):
    """``(proj, beta, V, ref)``: the float64 restatement of a case and the reference evaluated on its basis"""
    A, rows = inputs(case)
    proj, beta, V = restate(A, rows, case.k, case.m, case.b)
    return proj, beta, V, extension(A, V, case.k, case.m, case.b)


def test_the_cases_cover_the_edges():
    cs = BAND_CASES
    assert 40 <= len(cs) <= 50
    for kind in ("skew", "orth"):
        assert {c.b for c in cs if (c.n, c.k + c.b, c.m, c.kind) == (1501, 13, 13, kind)} == set(WIDTHS)
    assert {c.b for c in cs if (c.n, c.k + c.b, c.m, c.kind) == (LONG, 13, 13, "skew")} == set(WIDTHS)
    assert LONG % 32 and padded(LONG) // 2 >= 256 * 2 * 256 > (padded(LONG) - 64) // 2  # (256 lanes x 2 positions x 256 CUs)
    for b in (3, 5):
        assert {c.m for c in cs if c.n == 257 and c.b == b and c.m == c.k + b} >= {7, 8, 9, 16, 17}
    assert Case(40, 0, 2, 2, "skew") in cs and Case(257, 0, 8, 8, "skew") in cs
    assert {c.k for c in cs if (c.n, c.m, c.b, c.kind) == (1501, 128, 8, "skew")} == set(LDS_K)
    assert Case(1501, 121, 128, 8, "orth", 16) in cs
    for k in LDS_K:  # the dots kernel's LDS: 8 (b L + 4 run), L = 512 max(1, 10 / b), run = (r0 b + 15) & ~15
        lds = 8 * (8 * 512 + 4 * ((((k + 8) * 8) + 15) & ~15))
        assert (lds > 65536) == (k > 120) and (k > 120 or lds == 65536)
    assert {(c.k, c.m, c.b) for c in cs if c.n == 1501 and (c.m - c.k) > c.b} == {(3, 20, 6), (2, 12, 7), (4, 12, 3)}
    assert all((c.m - c.k) % c.b for c in cs if c.n == 1501 and (c.m - c.k) > c.b)  # a short last batch
    for n, k, m, b, kind, _ in SECOND_TRIP:  # 1025 slices on a grid of at most 1024 blocks, the last slice ragged
        L = 512 * max(1, 10 // b)
        pad = padded(n)
        assert -(-pad // L) == 1025 and 0 < pad - 1024 * L < L and Case(n, k, m, b, kind, 64) in cs
    assert {c.b <= 4 for c in cs if c.n in (1048609, 524289)} == {True, False}  # NG = 1 and NG = 2
    assert all(c in cs for c in PLANT_CASES)


@pytest.mark.parametrize("case", BAND_CASES, ids=case_id)
def test_case_is_decisive_and_float64_meets_the_bounds(case):
    A, rows = inputs(case)
    proj, beta, V, ref = restated(case)
    print(figures(case, ref))
    k = case.k
    wn = ref["w_norm"][k:]
    # the bounds are not vacuous
    assert np.all(ref["e_proj"][k:].max(axis=1) <= CAP * wn) and np.all(ref["e_beta"][k:] <= CAP * wn)
    assert np.all(np.linalg.norm(ref["e_v"], axis=1) * ref["beta"][k:] <= CAP * wn)
    # a dropped, doubled or misplaced second pass shows / the rows are orthonormal
    if case.kind == "skew":
        assert np.all(ref["c2"][k:] >= 1e-2 * wn)
    else:
        assert np.all(ref["c2"][k:] <= 1e-12 * wn)
    # float64 in the device's order lies within the bounds
    err = errors(case, ref, proj, beta, V)
    print("  restatement error / bound: " + " ".join(f"{key} {v:.2e}" for key, v in err.items()))
    assert all(v <= 1.0 for v in err.values()), err
    assert all(not proj[j, j + case.b:].any() for j in range(k, case.m))
    if case.kind == "orth":  # and so does the NumPy backend, in its own order
        be = NumpyBackend(A, block_size=case.b)
        be.V = np.zeros((case.m + case.b, case.n))
        be.V[: k + case.b] = rows
        pr, bt = be.extend_band(k, case.m)
        err = errors(case, extension(A, be.V, k, case.m, case.b), pr, bt, be.V)
        print("  numpy error / bound:       " + " ".join(f"{key} {v:.2e}" for key, v in err.items()))
        assert all(v <= 1.0 for v in err.values()), err


@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("case", PLANT_CASES, ids=case_id)
def test_a_planted_error_leaves_the_bounds(case, plant):
    A, rows = inputs(case)
    proj, beta, V = restate(A, rows, case.k, case.m, case.b, plant)
    err = errors(case, extension(A, V, case.k, case.m, case.b), proj, beta, V)
    print(f"{case_id(case)} {plant}: " + " ".join(f"{key} {v:.2e}" for key, v in err.items()))
    assert max(err.values()) > 1.0
