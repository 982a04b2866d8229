"""The cases of the single-vector extension step (``lz_trl_extend`` as an Arnoldi step) and, without a GPU, what makes them worth
running: for every case ``NumpyBackend.extend`` lies within the longdouble reference's bounds (tests/arnoldi_reference.py), the DGKS
gate is decided far from its edge, the bounds are small against ``|w|`` and, where the second pass runs, its coefficients are large
enough that a dropped or doubled pass shows.  tests/test_gpu_arnoldi_step.py imports ``STEP_CASES`` and ``reference``.

Matrix: ``n`` rows of six standard normal entries at random columns plus a diagonal in ``[0.6, 1]`` - non-symmetric, ``|A x|^2`` about
``6.65 |x|^2`` of which ``x . A x`` takes about a tenth.  Rows, ``nb`` of length ``n``, the last one ``x`` (the step is ``w = A x``):

- ``orth``: orthonormal.  They are drawn at random with the part along ``w`` damped, so that all rows but ``x`` together hold about
  ``min((nb - 1) / n, 0.08)`` of ``|w|^2`` whatever ``nb / n`` is (random rows hold ``(nb - 1) / n``, which at ``nb = 128``, ``n = 257``
  puts the gate's ratio on its edge); every coefficient stays generic, none vanishes.  The gate stays closed (ratio about 0.8).
- ``near``: the same, then row 0 replaced by ``normalise(w + 0.05 g)``, ``|g|`` about ``|w|``, and not re-orthogonalised: pass 1
  subtracts ``w`` once through row 0 and its parts along the other rows once more, the gate opens (ratio about 0.2) and pass 2's
  coefficients on rows ``1 ..`` are about minus pass 1's.
- ``skew``: ``M Q`` with ``Q`` the ``orth`` rows and ``M = I + 0.3 G / sqrt(nb)`` in all rows but the last, which stays ``x``: not
  orthonormal.  Pass 1 leaves at least the part of ``w`` outside the span, so the gate stays closed at every ``nb``; the forced run
  differs from the gated one by exactly ``c2``.

``thin``.  The bounds take every error at its worst sign, so through two passes they grow like ``nb^2 n_pad eps`` times three factors
``|row_i| . |row_j|`` (0.64 for dense Gaussian rows) and pass ``1e-9 |w|`` at ``nb = 128`` and from ``n = 20001`` on.  At those shapes
each row is drawn on a random ``1 / thin`` of the positions before it is made orthonormal (every position is still held by many
rows, every row still reaches every block of a walk), which shrinks those factors and nothing else.
"""
import collections
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from arnoldi_reference import step, worst

from lanczos_amd.eigsh import NumpyBackend

Case = collections.namedtuple("Case", "n nb kind force dense seed thin", defaults=(1,))
CAPTURE = 0.08  # the share of |w|^2 that the rows other than x hold (at most)
THREE_KINDS = [(257, 9), (1501, 17), (5121, 128)]  # shapes that run orth, near, skew gated and skew forced (on the device: on both Q^T w plans)


def _thin(n, nb):
    return {(257, 127): 2, (257, 128): 2, (20001, 9): 2, (5121, 128): 16}.get((n, nb), 1)


def _cases():
    out = []
    for nb in (2, 3, 7, 8, 9, 15, 16, 17, 33, 64, 65, 127, 128):  # the 8-row tiles of the Q^T w walk, 16 and 4 rows in flight, m's limits
        out.append(Case(257, nb, "near", False, False, 1, _thin(257, nb)))
    for n in (33, 255, 256, 1501, 5121, 20001):  # the padding's edges, more than one block, several slices
        out.append(Case(n, 9, "near", False, False, 1, _thin(n, 9)))
    for n, nb in THREE_KINDS:
        t = _thin(n, nb)
        out += [Case(n, nb, "orth", False, False, 1, t), Case(n, nb, "skew", False, False, 1, t), Case(n, nb, "skew", True, False, 1, t)]
    out += [Case(1501, 17, "near", False, False, 1), Case(5121, 128, "near", False, False, 1, _thin(5121, 128))]
    out += [Case(257, 8, "skew", False, False, 1), Case(257, 8, "skew", True, False, 1)]
    for nb in (4, 5):  # the first row length of k_trl_cgs<4, 4>: one pass, and both (a near row 0 alone costs n_pad eps |w| there)
        out += [Case(524289, nb, "orth", False, False, 1), Case(524289, nb, "skew", True, False, 1, 8)]
    for n, nb in ((33, 9), (257, 9), (1501, 17)):  # the dense product under the same step
        out += [Case(n, nb, "near", False, True, 1), Case(n, nb, "skew", True, True, 1)]
    assert len({c[:5] for c in out}) == len(out)
    return out


STEP_CASES = _cases()


def case_id(c):
    return f"{c.n}-{c.nb}-{c.kind}" + ("-forced" if c.force else "") + ("-dense" if c.dense else "") + (f"-thin{c.thin}" if c.thin > 1 else "")


@functools.lru_cache(maxsize=None)
def matrix(n):
    rng = np.random.default_rng(1000 + n)
    r = np.repeat(np.arange(n), 6)
    A = sp.csr_matrix((rng.standard_normal(6 * n), (r, rng.integers(0, n, 6 * n))), shape=(n, n)) + sp.diags(rng.uniform(0.6, 1.0, n))
    A = A.tocsr()
    A.sort_indices()
    assert abs(A - A.T).max() > 0.1
    return A


def make_rows(A, nb, kind, seed, thin=1, coupling=0.3):
    """the ``(nb, n)`` float64 rows of a case (see the module docstring)"""
    n = A.shape[0]
    rng = np.random.default_rng([seed, n, nb])

    def draw(count):
        G = rng.standard_normal((count, n))
        return G if thin == 1 else G * (rng.random((count, n)) * thin < 1.0)

    x = draw(1)[0]
    x /= np.linalg.norm(x)
    w = A @ x
    wp = w - np.dot(x, w) * x
    wp /= np.linalg.norm(wp)
    G = draw(nb - 1)
    s = min(1.0, np.sqrt(CAPTURE * n / (nb - 1)))
    G -= (1.0 - s) * np.outer(G @ wp, wp)
    Q = np.linalg.qr(np.vstack([x, G]).T)[0].T  # row 0 is x up to its sign, the others are orthonormal to it
    rows = np.vstack([Q[1:], x])
    if kind == "near":
        g = rng.standard_normal(n) * (np.linalg.norm(w) / np.sqrt(n))
        u = w + 0.05 * g
        rows[0] = u / np.linalg.norm(u)
    elif kind == "skew":
        M = np.eye(nb) + coupling * rng.standard_normal((nb, nb)) / np.sqrt(nb)
        M[nb - 1] = 0.0
        M[nb - 1, nb - 1] = 1.0  # the last row stays x: the step is the same product
        rows = M @ rows
    else:
        assert kind == "orth"
    return np.ascontiguousarray(rows)


@functools.lru_cache(maxsize=None)
def reference(case):
    """``(A, rows, ref)`` of a case, computed once and never changed: ``A`` as the device gets it (CSR, or its dense copy)"""
    A = matrix(case.n)
    rows = make_rows(A, case.nb, case.kind, case.seed, case.thin)
    if case.dense:
        A = A.toarray()
    ref = step(A, rows, case.force)
    for a in (rows, ref["c1"], ref["c2"], ref["v"], ref["e_proj"], ref["e_v"]):
        a.setflags(write=False)
    return A, rows, ref


def figures(case, ref):
    return (f"{case_id(case):28s} ratio {ref['ratio']:.3f} pass2 {int(ref['pass2'])} max|c2|/|w| {np.abs(ref['c2']).max() / ref['w_norm']:.2e} "
            f"e_proj/|w| {ref['e_proj'].max() / ref['w_norm']:.2e} e_beta/|w| {ref['e_beta'] / ref['w_norm']:.2e} "
            f"|e_v|/|w| {np.linalg.norm(ref['e_v']) / ref['w_norm']:.2e}")


def test_the_cases_cover_the_edges():
    assert 35 <= len(STEP_CASES) <= 50
    assert {c.nb for c in STEP_CASES if c.n == 257} >= {2, 3, 7, 8, 9, 15, 16, 17, 33, 64, 65, 127, 128}
    assert {c.n for c in STEP_CASES if c.nb == 9} >= {33, 255, 256, 257, 1501, 5121, 20001}
    assert {c.nb for c in STEP_CASES if c.n == 524289} == {4, 5}
    for shape in THREE_KINDS:
        assert {(c.kind, c.force) for c in STEP_CASES if (c.n, c.nb) == shape and not c.dense} == {("orth", False), ("near", False), ("skew", False), ("skew", True)}


@pytest.mark.parametrize("case", STEP_CASES, ids=case_id)
def test_case_is_decisive_and_numpy_meets_the_bounds(case):
    A, rows, ref = reference(case)
    print(figures(case, ref))
    wn = ref["w_norm"]
    # the gate is decided far from its edge, from the reference alone
    assert ref["ratio"] <= 0.25 or ref["ratio"] >= 0.75
    assert ref["pass2"] == (case.kind == "near" or case.force)
    # the bounds are not vacuous
    assert ref["e_proj"].max() <= 1e-9 * wn and ref["e_beta"] <= 1e-9 * wn and np.linalg.norm(ref["e_v"]) <= 1e-9 * wn
    # a dropped (or doubled) second pass shows
    if ref["pass2"]:
        assert np.abs(ref["c2"]).max() >= 1e-2 * wn
    else:
        assert not ref["c2"].any()
    # float64 in another order lies within the bounds
    be = NumpyBackend(A, force_second_pass=case.force)
    be.V = np.zeros((case.nb + 1, case.n))
    be.V[: case.nb] = rows
    proj, beta = be.extend(case.nb - 1, case.nb)
    err = {"proj": worst(np.abs(proj[case.nb - 1, : case.nb] - (ref["c1"] + ref["c2"])), ref["e_proj"]),
           "beta": worst(abs(beta[case.nb - 1] - ref["beta"]), ref["e_beta"]), "v": worst(np.abs(be.V[case.nb] - ref["v"]), ref["e_v"])}
    print("  numpy error / bound: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert all(v <= 1.0 for v in err.values())


def test_skew_runs_differ_by_the_second_pass():
    """the gated and the forced ``skew`` run of a shape share their rows: same ``c1``, and ``c2`` only where forced"""
    for n, nb in THREE_KINDS + [(257, 8)]:
        t = _thin(n, nb)
        gated, forced = reference(Case(n, nb, "skew", False, False, 1, t)), reference(Case(n, nb, "skew", True, False, 1, t))
        assert np.array_equal(gated[1], forced[1]) and np.array_equal(gated[2]["c1"], forced[2]["c1"])
        assert not gated[2]["pass2"] and forced[2]["pass2"]
