"""One call of ``lz_trl_extend_band`` in ``np.longdouble``, with first-order error bounds for a float64 device.

``extension`` follows the device batch by batch (``j = k, k + b, ...``, ``nb = min(b, m - j)``, ``r0 = j + b``).  Step ``i < nb`` of a
batch is ``w = A V[j + i]``, two ungated classical Gram-Schmidt passes against ``V[:r0]`` (the block passes: the device does them for all
``b`` work vectors in one walk, which is the same operation per vector), for ``i > 0`` two more against the ``i`` rows the batch has made
so far (the tail), then ``beta = |r|``, ``v = r / beta``.  Every quantity carries the absolute bound that ``arnoldi_reference`` derives
for the same operations - a product row, a dot product over the padded length, a Gram-Schmidt update, a norm, a quotient - and the
passes are that module's ``_pass``.

The basis is taken **as it stands after the call**: rows ``0 .. k + b - 1`` are the inputs, the rows above are what the implementation
under test produced, and each new row is checked against what follows from ``A`` and the float64 rows below it *as given*.  Row
``r0 + i`` is a function of ``A``, the old rows and the new rows below it, so the check is complete; carrying the new rows' own bounds
through the tail instead (every error at its worst sign) compounds them by about a factor seven per tail stage, to ``4e-6 |w|`` at
``b = 7``, where conditioning on the produced rows leaves ``1e-10 |w|``.

A plain module: no fixtures, nothing collected from it.
"""
import numpy as np
from arnoldi_reference import EPS, LD, _abs_matvec, _pass, matvec, padded, worst

__all__ = ["extension", "worst"]


def extension(A, V, k, m, b):
    """``V``: the ``(m + b, n)`` float64 basis after ``extend_band(k, m)``.  Returns a dict: ``proj`` (``m x (m + b)``), ``beta`` (``m``) and
    ``rows`` (the expected rows ``k + b .. m + b - 1``) in float64, their bounds ``e_proj``, ``e_beta``, ``e_v`` of the same shapes, and per
    step ``w_norm`` and ``c2`` (``max|c2|`` of the second block pass), both of length ``m`` and zero below ``k``."""
    V = np.asarray(V, dtype=np.float64)
    assert V.shape[0] == m + b and 0 <= k < m
    n = V.shape[1]
    n_pad = padded(n)
    VL = V.astype(LD)
    f = np.float64
    out = {"proj": np.zeros((m, m + b)), "e_proj": np.zeros((m, m + b)), "beta": np.zeros(m), "e_beta": np.zeros(m),
           "rows": np.zeros((m - k, n)), "e_v": np.zeros((m - k, n)), "w_norm": np.zeros(m), "c2": np.zeros(m)}
    for j in range(k, m, b):
        nb, r0 = min(b, m - j), j + b
        old = VL[:r0]
        for i in range(nb):
            s = j + i
            w = matvec(A, VL[s])
            aw, terms = _abs_matvec(A, V[s])
            e_w = terms * EPS * aw
            c1, r, e_c1, e_r = _pass(old, w, e_w, n_pad)
            c2, r, e_c2, e_r = _pass(old, r, e_r, n_pad)
            out["proj"][s, :r0], out["e_proj"][s, :r0] = (c1 + c2).astype(f), (e_c1 + e_c2).astype(f)
            if i > 0:  # the tail: the rows this batch has made so far, exact float64 inputs
                new = VL[r0: r0 + i]
                d1, r, e_d1, e_r = _pass(new, r, e_r, n_pad)
                d2, r, e_d2, e_r = _pass(new, r, e_r, n_pad)
                out["proj"][s, r0: r0 + i], out["e_proj"][s, r0: r0 + i] = (d1 + d2).astype(f), (e_d1 + e_d2).astype(f)
            beta = np.sqrt(np.dot(r, r))
            e_beta = np.sqrt(np.dot(e_r, e_r)) + n_pad * EPS * beta
            out["beta"][s], out["e_beta"][s] = float(beta), float(e_beta)
            out["rows"][s - k] = (r / beta).astype(f)
            out["e_v"][s - k] = ((e_r + np.abs(r) * (e_beta / beta + 2 * EPS)) / beta).astype(f)
            out["w_norm"][s] = float(np.sqrt(np.dot(w, w)))
            out["c2"][s] = float(np.abs(c2).max())
    return out
