"""The two-pass re-orthogonalisation sweep in longdouble, its forward bounds, a NumPy replay of pass 2, a Python restatement of
the launch-time plan, and the list of step cases (tests/test_reorth_host.py checks all of this without a device,
tests/test_gpu_reorth_step.py runs the cases through lz_step_reorth).

The sweep (lz_reorth.hip; step_reorth in lz_loops.hip):  c = V[0:nrows] . w,  V[j] = 2 w - sum_i c_i V_i  with
  mode 0  w = V[j] as stored;
  mode 1  w = r / beta, beta = sqrt(|r|^2), stored to V[j] before pass 1 dots it;
  mode 2  (LZ_FLAG_FUSED_NORM, nrows == j + 1) pass 1 dots the raw r, k_fused_prepare turns the sums into beta = sqrt(r.r),
          c_i = (V_i . r) / beta, c_j = (r.r) / (beta beta), and pass 2 forms w = r / beta itself.

Coefficient bound  |c_dev - c_ref| <= gamma_K sum|V_i||w|,  gamma_K = K u / (1 - K u), u = 2^-53.  K is the largest number of
roundings on any path from a product to the result, read from the kernels' summation tree, one line per stage:

  4x4x4 MFMA family (k_qtw_mfma4), rows i != j
    per-lane chain + MFMA contraction: a wave owns L/4 elements and walks them 32 per step, two MFMAs per step; an MFMA adds four
        products to the accumulator in an order the code does not show: any order of five terms is at most 4 additions deep, a
        product at most one rounding more (none if the unit fuses) -> 5 for the first MFMA, 4 for each further one:
        1 + 4 * 2 * (L / 128) = L / 16 + 1
    cross-lane steps: the four 64-byte chunks of a row, __shfl_xor 4 and 8                                     + 2
    the four waves: ((k0 + k1) + k2) + k3                                                                      + 3
    second stage over the P = G runs (k_final_rows_t): a lane's strided chain, at most ceil(G / 128) additions,
        (a0 + a1) + (a2 + a3), then 128 partial sums added in order                                            + ceil(G / 128) + 2 + 128
  row j (its coefficient is w . w from the LDS image, qtw_stage_w): a lane's fma chain over the slice, L / 256 roundings, wave_sum
        6, the four waves 3, the same second stage: never more than the line above (L >= 512).
  VALU family (k_qtw_valu, k_final_rows)
    per-lane fma chain over the slice: two per double2, L / 512 double2 per lane                               L / 256
    wave_sum (six shuffle steps) and the four wave sums added in order                                         + 6 + 4
    second stage (k_final_rows): a lane's chain over the G partials, then block_sum                            + ceil(G / 256) + 6 + 4
  Adding an exact zero rounds nothing, and any summation order of rows_pad products is covered by the classical
  K = rows_pad + nrows: coef_K returns the smaller of the two, both are valid.
  mode 2: c_i = fl(raw_i / b), b = fl(sqrt(rr)), rr = r.r(1 + theta_K): b = beta (1 + theta_(K+1)), so raw_i / b is off by at most
        gamma_K + gamma_(K+2) of sum|V_i||r| / beta, and c_j = rr / (b b) by gamma_(3K+4): K_fused = 3 K + 4 for every coefficient.
  beta of modes 1 and 2 (k_three_term's |r|^2: grid-stride fma chain, block_sum, final_sum_1024; or pass 1's self term): the
        classical K = rows_pad covers either tree; the square root halves the relative error and rounds once: gamma_(rows_pad+1).

Row: given the device's own c (and beta) pass 2 is float64 NumPy, bit for bit - every arm adds c_k V_k to a running sum that
starts at 0.0 in ascending k, products and sums rounded separately (-ffp-contract=off), then 2 w - sum.  That holds for all arms:
k_update, the k_update_slice<P, RU> instantiations (RU rows are LOADED together, the additions stay in row order) and k_update_elem
(its two register buffers alternate loads, add(k, q[0]) always precedes add(k + 32, q[1])).  No arm needs the longdouble row;
row_bound is used on the host only, to show what the bound can see.
"""
import collections
import functools
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TPB, NUM_CU, PAD = 256, 256, 32  # kTPB, kNumCU, kPadDoubles (lz_internal.h)
QTW_MAX_L = 5120                 # kQtwMaxL
FLAG_VALU, FLAG_FUSED, FLAG_PARTIAL, FLAG_ONE_REDUCE = 4, 16, 64, 256


def gamma(K):
    return K * U / (1.0 - K * U)


def padded(rows):
    return (rows + PAD - 1) // PAD * PAD


# ------------------------------------------------------------------------------------------------ the sweep in longdouble
Sweep = collections.namedtuple("Sweep", "beta w c c_mag row row_mag")


def sweep_reference(V, j, nrows, r=None, mode=0, beta=None):
    """The exact sweep of rows V[0:nrows] (float64 in, longdouble out).  beta: the device's own beta (mode 1: the row the
    device dots is the float64 quotient r / beta it stored); None: beta = |r| in longdouble.  Returns
    Sweep(beta, w, c, c_mag = sum|V_i||w| per coefficient, row, row_mag = |2 w| + sum|c_i||V_i| per element)."""
    Vl = np.array(V[:nrows], dtype=LD)
    b = None
    if mode == 0:
        w = Vl[j].copy()
    else:
        rl = np.asarray(r, dtype=LD)
        b = np.sqrt(np.sum(rl * rl))
        w = rl / b if beta is None else np.asarray(np.asarray(r, dtype=np.float64) / np.float64(beta), dtype=LD)
        Vl[j] = w
    aV, aw = np.abs(Vl), np.abs(w)
    c = Vl @ w
    return Sweep(b, w, c, aV @ aw, LD(2) * w - c @ Vl, LD(2) * aw + np.abs(c) @ aV)


def numpy_sweep(V, j, nrows):
    """the float64 expression of the reference implementation (docstring of test_reorth_matches_numpy)"""
    c = np.sum(V[j] * V[:nrows], axis=1)
    return c, 2 * V[j] - np.sum(c[:, None] * V[:nrows], axis=0)


def replay_row(V, j, nrows, c, w):
    """pass 2 as every arm evaluates it, from the device's coefficients; w: V[j] (mode 0) or the float64 r / beta"""
    t = np.zeros_like(w)
    for k in range(nrows):
        t = t + c[k] * (w if k == j else V[k])
    return 2.0 * w - t


def row_bound(ref, V, j, nrows, K):
    """|row - ref.row| of a float64 pass 2 on float64 coefficients that are within gamma_K c_mag of ref.c"""
    aV = np.abs(np.array(V[:nrows], dtype=LD))
    aV[j] = np.abs(ref.w)
    return gamma(nrows + 2) * ref.row_mag + (gamma(K) * ref.c_mag) @ aV


# ------------------------------------------------------------------------------------------------ the plan
Plan = collections.namedtuple("Plan", "L G family variant R tile Y lds arm P P_rule")


def qtw_ldp(nrows):
    return (nrows + 15) & ~15


def qtw_room(flags, nrows_max):
    ncol = 2 if flags & FLAG_ONE_REDUCE else 1
    return 155 * 1024 // ncol - (TPB // 64) * qtw_ldp(nrows_max + (2 if ncol == 2 else 0)) * 8


def _balance(G):
    g = G / NUM_CU
    return g / math.ceil(g)


def plan_qtw(length, flags, tune, nrows_max):
    """(L, G, family) of plan_qtw: family 2 = 4x4x4 MFMA, 0 = VALU"""
    target = tune.get(0, 0)
    L = 512
    if target > 0:
        L = (target + 511) // 512 * 512
    else:
        best, found = -1.0, False
        lmax = QTW_MAX_L // 2 if flags & FLAG_ONE_REDUCE else QTW_MAX_L
        room = qtw_room(flags, nrows_max)
        if int(room / 8) < lmax:
            lmax = max(512, int(int(room / 8) / 512) * 512)
        cand = lmax
        while cand >= 1024 and not found:
            G = (length + cand - 1) // cand
            if G >= 480:
                bal = _balance(G)
                if bal >= 0.93:
                    L, found = cand, True
                elif bal * cand / (cand + 48) > best:
                    best, L = bal * cand / (cand + 48), cand
            cand -= 512
    L = min(L, QTW_MAX_L)
    G = (length + L - 1) // L
    family = 0 if flags & FLAG_VALU else 2
    if family == 2 and qtw_room(flags, nrows_max) < L * 8:
        family = 0
    return L, G, family


def auto_p(span):
    """positions per lane by launch_update's balance rule: (P, "balanced" when a candidate reached 0.93, else "best")"""
    best, P = -1.0, 2
    for cand in (16, 8, 4, 2):
        bal = _balance((span + TPB * cand - 1) // (TPB * cand))
        if bal >= 0.93:
            return cand, "balanced"
        if bal > best:
            best, P = bal, cand
    return P, "best"


def update_arm(rows_pad, nrows, fused, knob8=0):
    """(name, P, rule) of the pass-2 kernel launch_update picks for a whole row (no gate, no position range)"""
    span = rows_pad // 2
    if not fused and knob8 == 1:
        return "update<cached>", 0, "knob"
    if knob8 == 2:
        return "update<nt>", 0, "knob"
    P, rule = (8, "knob") if knob8 == 3 else (4, "knob") if knob8 == 4 else auto_p(span)
    if knob8 == 6 or (knob8 == 0 and P == 16 and span > 16384):
        return "slice<16,1>", 16, "knob" if knob8 == 6 else rule
    if knob8 == 0 and span <= 4096 and fused and nrows > 64:
        return "elem", 0, "threshold"
    if (knob8 == 0 and span <= 16384) or knob8 == 5:
        return "slice<1,32>", 1, "knob" if knob8 == 5 else "threshold"
    if P == 8:
        return "slice<8,2>", 8, rule
    if P == 4:
        return "slice<4,4>", 4, rule
    return "slice<2,8>", 2, rule  # (P == 2, and P == 16 where the 16-position arm's own conditions do not hold)


def step_mode(flags, scale, j, nrows):
    """the pass-1 mode step_reorth launches"""
    if scale and flags & FLAG_FUSED and not flags & FLAG_PARTIAL and nrows == j + 1:
        return 2
    return 1 if scale else 0


def plan(rows_pad, flags, tune, nrows_max, nrows=None, mode=0):
    """plan_qtw, qtw_room, qtw_ldp, launch_qtw_t and launch_update restated.  tune: {knob: value}.  nrows, mode: the call (default: a
    mode-0 call on nrows_max - 2 rows, the cases' allocation).  Returns Plan(L, G, family, variant, R = rows per VALU trip, tile =
    rows per MFMA tile, Y = row split, lds = dynamic LDS bytes of pass 1, arm, P, P_rule of pass 2)."""
    nrows = nrows_max - 2 if nrows is None else nrows
    L, G, family = plan_qtw(rows_pad, flags, tune, nrows_max)
    variant = tune.get(1, 0)
    Y, R, tile = 1, 0, 0
    if family == 2:
        ncol = 2 if mode == 3 else 1
        ldp = qtw_ldp(nrows + 2 if mode == 3 else nrows)
        lds = ncol * (L * 8 + (TPB // 64) * ldp * 8)
        tile = {10: 16, 11: 32, 13: 8}.get(variant, 8)
        if mode in (2, 4) and G <= 64 and nrows > 8:
            Y = max(1, min(256 // G, (nrows + 7) // 8))
    else:
        lds = L * 8
        R = {1: 4, 7: 8}.get(variant, 8 if nrows > 4 else 4)
    arm, P, rule = update_arm(rows_pad, nrows, mode == 2, tune.get(8, 0))
    return Plan(L, G, family, variant, R, tile, Y, lds, arm, P, rule)


def coef_K(p, rows_pad, nrows, mode):
    """K of the coefficient bound for a call planned as p (module docstring)"""
    if p.family == 2:
        tree = (p.L // 16 + 1) + 2 + 3 + (-(-p.G // 128) + 2 + 128)
    else:
        tree = p.L // 256 + 6 + 4 + (-(-p.G // 256) + 6 + 4)
    K = min(tree, rows_pad + nrows)
    return 3 * K + 4 if mode == 2 else K


def beta_K(rows_pad):
    return rows_pad + 1


# ------------------------------------------------------------------------------------------------ the step cases
# claim: what the id says about the branch, every entry asserted against plan() (host and device)
Case = collections.namedtuple("Case", "id M nrows j mode flags knobs claim")
MODE_NAME = {0: "stored", 1: "scaled", 2: "fused"}


def _case(sec, what, M, nrows, j, mode, flags=0, knobs=(), **claim):
    flags |= FLAG_FUSED if mode == 2 else 0
    what = what.replace("<", "").replace(">", "").replace(",", "x")  # slice<8,2> -> slice8x2
    return Case(f"{sec}-{what}-M{M}-n{nrows}-j{j}-{MODE_NAME[mode]}", M, nrows, j, mode, flags, tuple(knobs), claim)


def _uniq(seq):
    return list(dict.fromkeys(seq))


def _slices():
    out = []
    for L in (512, 1024, 2560, 5120):
        for M in _uniq([31, 33, 512, 513, L, L + 1, L + 32, L + 33, 2 * L - 31, 3 * L + 130]):
            G = -(-padded(M) // L)
            for mode in (0, 1, 2):
                for j in (0, 5, 10):
                    nrows = j + 1 if mode == 2 else 11  # the fused call is the in-loop shape: row j is the newest
                    Y = 2 if mode == 2 and nrows == 11 else 1
                    out.append(_case("a", f"L{L}-G{G}-Y{Y}", M, nrows, j, mode, 0, [(0, L)], L=L, G=G, family=2, Y=Y, arm="slice<1,32>"))
    return out


def _tile_rows(t):
    return _uniq([1, 2, 3, 4, 5, t - 1, t, t + 1, 2 * t + 3])


def _tile_js(nrows):
    return _uniq([j for j in (0, 1, nrows // 2 if nrows >= 3 else 0, nrows - 1) if j < nrows])


def _tiles():
    out = []
    for knob1, t in ((0, 8), (10, 16), (11, 32), (13, 8)):
        for nrows in _tile_rows(t):
            for j in _tile_js(nrows):
                out.append(_case("b", f"mfma-k{knob1}-tile{t}", 1300, nrows, j, 0, 0, [(0, 512), (1, knob1)], L=512, G=3, family=2, variant=knob1, tile=t))
    for knob1, t in ((0, 8), (1, 4), (7, 8)):
        for nrows in _tile_rows(t):
            R = (8 if nrows > 4 else 4) if knob1 == 0 else t
            for j in _tile_js(nrows):
                out.append(_case("b", f"valu-k{knob1}-R{R}", 1300, nrows, j, 0, FLAG_VALU, [(0, 512), (1, knob1)], L=512, G=3, family=0, variant=knob1, R=R))
    return out


def _row_split():
    out = []
    for G, nrows, Y in ((1, 9, 2), (1, 200, 25), (2, 17, 3), (64, 9, 2), (64, 40, 4), (65, 40, 1)):
        out.append(_case("c", f"G{G}-Y{Y}", 512 * G - 7, nrows, nrows - 1, 2, 0, [(0, 512)], L=512, G=G, family=2, Y=Y))
    return out


def _big_lds():
    return [_case("d", "lds66560-Y100", 5120 + 96, 800, 799, 2, 0, [(0, 5120)], L=5120, G=2, family=2, Y=100, lds=66560, arm="elem"),
            _case("d", "valu-fallback", 1056, 4098, 2049, 0, 0, [(0, 5120)], L=5120, G=1, family=0, R=8, arm="slice<1,32>")]


UNFUSED_ARM = {1: "update<cached>", 2: "update<nt>", 3: "slice<8,2>", 4: "slice<4,4>", 5: "slice<1,32>", 6: "slice<16,1>"}
FUSED_ARM = dict(UNFUSED_ARM)
FUSED_ARM[1] = "slice<2,8>"  # knob 8 = 1 is not honoured with the fused residual and switches the short-vector rules off: automatic P


def first_balanced(cand):
    """the smallest rows_pad whose whole row the automatic rule gives `cand` positions per lane because its block count is balanced"""
    rows_pad = padded(2 * (238 * TPB * cand + 1))  # G = 239 blocks: 239 / 256 >= 0.93 > 238 / 256
    while update_arm(rows_pad, 3, False)[1:] != (cand, "balanced"):
        rows_pad += PAD
    assert update_arm(rows_pad - PAD, 3, False)[2] == "best"
    return rows_pad


def _update_arms():
    out = []
    for knob8 in (1, 2, 3, 4, 5, 6):
        for M in (33, 4099, 40000):
            for nrows in (1, 7, 33, 70):
                out.append(_case("e", f"k{knob8}-{UNFUSED_ARM[knob8]}", M, nrows, nrows // 2, 0, 0, [(8, knob8)], arm=UNFUSED_ARM[knob8]))
                out.append(_case("e", f"k{knob8}-{FUSED_ARM[knob8]}", M, nrows, nrows - 1, 2, 0, [(8, knob8)], arm=FUSED_ARM[knob8]))
    # the automatic rule at its thresholds.  A row is padded to 32 doubles, so the spans are multiples of 16 positions: the first span
    # above 4096 is 4112, above 16384 it is 16400.
    for M, nrows, arm in ((8192, 64, "slice<1,32>"), (8192, 65, "elem"), (8193, 64, "slice<1,32>"), (8193, 65, "slice<1,32>")):
        out.append(_case("e", f"auto-pos{padded(M) // 2}-{arm}", M, nrows, nrows - 1, 2, arm=arm))
    for M, arm in ((32768, "slice<1,32>"), (32769, "slice<2,8>")):
        for mode in (0, 2):
            out.append(_case("e", f"auto-pos{padded(M) // 2}-{arm}", M, 3, 2, mode, arm=arm))
    # automatic P: the first balanced row length of each P and the row length below it (same P or a neighbour by the best-balance rule)
    for cand in (2, 4, 8, 16):
        first = first_balanced(cand)
        for rows_pad in (first, first - PAD):
            arm, P, rule = update_arm(rows_pad, 3, False)
            for mode in (0, 2):
                out.append(_case("e", f"auto-P{P}-{rule}-{arm}", rows_pad - PAD + 1, 3, 2, mode, arm=arm, P=P, P_rule=rule))
    return out


def _second_stage():
    out = []
    for flags, fam in ((0, 2), (FLAG_VALU, 0)):
        for G in (1, 2):
            for nrows in (1, 7, 8, 9, 16, 17):
                out.append(_case("f", f"G{G}-family{fam}", 512 * G - 5, nrows, nrows // 2, 0, flags, [(0, 512)], L=512, G=G, family=fam))
        out.append(_case("f", f"G3824-family{fam}", 512 * 3824 - 5, 3, 1, 0, flags, [(0, 512)], L=512, G=3824, family=fam))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _slices() + _tiles() + _row_split() + _big_lds() + _update_arms() + _second_stage()
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


def case_plan(case):
    return plan(padded(case.M), case.flags, dict(case.knobs), case.nrows + 2, case.nrows, case.mode)


def assert_claim(case):
    p = case_plan(case)
    for key, want in case.claim.items():
        assert getattr(p, key) == want, f"{case.id}: plan() gives {key} = {getattr(p, key)}, the id says {want}"
    return p


def case_inputs(case):
    """(V, r): nrows rows of standard_normal / sqrt(M) and two NaN rows behind them; r standard normal where the mode reads it, NaN
    where it must stay untouched.  Row j of a scaling mode is written before it is read: large finite values that would show."""
    rng = np.random.default_rng([case.M, case.nrows, case.j, case.mode])
    V = np.full((case.nrows + 2, case.M), np.nan)
    V[: case.nrows] = rng.standard_normal((case.nrows, case.M)) / np.sqrt(case.M)
    if case.mode == 0:
        return V, np.full(case.M, np.nan)
    V[case.j] = 1e3 * rng.standard_normal(case.M)
    return V, rng.standard_normal(case.M)


# ------------------------------------------------------------------------------------------------ the run loops (tests/test_gpu_reorth_loops.py)
def lanczos_longdouble(A, n, v0):
    """oracle/lanczos_ref.execute_lanczos (full sweep over rows 0..j at every step, the reference's quirks included) in longdouble
    on the float64 matrix A (SciPy CSR without empty rows, or a dense array) from the float64 start vector v0 as given."""
    if hasattr(A, "indptr"):
        data, idx, starts = np.asarray(A.data, dtype=LD), A.indices, A.indptr[:-1]
        assert np.all(np.diff(A.indptr) > 0)
        mul = lambda x: np.add.reduceat(data * x[idx], starts)
    else:
        Al = np.asarray(A, dtype=LD)
        mul = lambda x: Al @ x
    M = A.shape[0]
    V = np.zeros((n, M), dtype=LD)
    V[0] = np.asarray(v0, dtype=LD)
    alpha, beta = np.zeros(n, dtype=LD), np.zeros(n - 1, dtype=LD)
    r = mul(V[0])
    alpha[0] = r @ V[0]
    r = r - alpha[0] * V[0]
    for j in range(n):
        beta[j - 1] = np.sqrt(r @ r)
        V[j] = r / beta[j - 1]
        c = V[: j + 1] @ V[j]
        V[j] = 2 * V[j] - c @ V[: j + 1]
        r = mul(V[j])
        alpha[j] = V[j] @ r
        r = r - V[j] * alpha[j] - V[j - 1] * beta[j - 1]
    return alpha, beta, V


def expected_engine(flags, knob1, knob15, G):
    """choose_loop (lz_loops.hip) on one rank for the flags and knobs the loop tests use"""
    default_kernels = knob1 == 0 and not flags & FLAG_VALU
    if flags & FLAG_ONE_REDUCE and not flags & FLAG_PARTIAL and not flags & FLAG_VALU:
        return "one-reduce"
    if flags & FLAG_PARTIAL and default_kernels:
        return "partial-one-reduce" if flags & FLAG_ONE_REDUCE else "partial-device"
    if knob15 or not flags & FLAG_FUSED or flags & FLAG_PARTIAL or not default_kernels:
        return "kernels"
    return "fused" if G <= 8 else "three-term-fused"
