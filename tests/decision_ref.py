"""numpy restatement of the kernels that DECIDE (csrc/decide.hip): the two-stage gate (gate_begin / gate_flag / gate_widen_* /
gate_recheck / round_counts), the conditioning guard (x8_guard_begin / _flag / _fix), the gate's softmax (gate_finish,
switch_finish) and the routing helpers (route, scatter3, stat_max_export / _import, mask_empty_queries), with the counter blocks
as plain Python lists and numpy arrays.

What fp32 IEEE arithmetic pins is stated in np.float32, operation by operation, and is compared BIT FOR BIT: the top-2 margin,
the comparisons with tau_eff / lower / upper, widen * max_margin_err, the pair error |(k_a - k_e) - (l_a - l_e)|, the round
counts, the tau_eff sequence and the max-as-bits words.  None of these holds a multiply followed by an add, so the compiler's
freedom to contract a * b + c does not reach them.  The rest is stated in fp64 and compared under a bound:
  PROB_REL  softmax probabilities: an exp of ~1 ulp, a sum of <= 8 terms, a division -- 2^-20 relative (tests/test_gpu_layers.py)
  SUM_REL   sum_sq_pair_err: <= 8 fp32 roundings per row (pe * pe + sq, contracted or not), fp64 adds in any order -- 2^-20 relative
  DN_REL    max_dn: three squared differences and a square root -- 2^-21 relative
Flag lists and routing lists are filled with atomics: a list is predicted as a SET, a round of it only by its size.

The restatement states the INTENDED behaviour: a row with any non-finite logit (NaN, +inf, -inf) is flagged by the filter pass
and left out of the widening passes; in the recheck a pair (a, e) whose error is not finite adds nothing to max_margin_err, to
the squared sum or to `pairs`."""
import numpy as np

F32 = np.float32
MAX_EXPERTS, MAX_ROUNDS = 8, 24                       # NESTI_MAX_EXPERTS; csrc/host.h: kMaxCascadeRounds
FC_ROUND_COUNTS, FC_TAU_EFF, FC_WIDEN_UPPER, FC_WIDEN_COUNT, FC_WIDEN_ROUNDS = 8, 40, 41, 48, 56   # int32 words of fcounts
PROB_REL, SUM_REL, DN_REL = 2.0 ** -20, 2.0 ** -20, 2.0 ** -21
GRID = 2.0 ** -10                                     # crafted logits are pairwise equal or at least this far apart


def f32_bits(x):
    return int(np.asarray(x, F32).reshape(1).view(np.uint32)[0])


def bits_f32(w):
    return np.asarray([int(w) & 0xFFFFFFFF], np.uint32).view(F32)[0]


def new_cstat(max_err=0.0):
    """[0] queries [1] rechecked [2] changed [3] max_margin_err bits [4] the squared sum (a float here) [5] pairs [6] widened
    [7] widen events."""
    return [0, 0, 0, f32_bits(max_err), 0.0, 0, 0, 0]


def round_counts(counts, cap, n_rounds):
    """out[i * n_rounds + r] = clamp(counts[i] - r * cap, 0, cap)"""
    return np.asarray([max(0, min(cap, int(c) - r * cap)) for c in counts for r in range(n_rounds)], np.int32)


def top2_margin(l):
    """(margin [B] f32 -- the loop of top2_margin, row-parallel -- , nonfinite [B])"""
    l = np.asarray(l, F32)
    mx = np.full(l.shape[0], -np.inf, F32)
    second = mx.copy()
    with np.errstate(invalid="ignore"):
        for e in range(l.shape[1]):
            gt = l[:, e] > mx
            second = np.where(gt, mx, np.fmax(second, l[:, e]))     # fmaxf skips a NaN
            mx = np.where(gt, l[:, e], mx)
        margin = (mx - second).astype(F32)
    return margin, ~np.isfinite(l).all(axis=1)


def softmax64(l):
    """The kernels' softmax in fp64: max with fmaxf (NaNs skipped), exp(l - max), / sum.  A NaN or +inf logit, or a row of -inf,
    makes the whole row NaN."""
    l = np.asarray(l, F32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.fmax.reduce(l, axis=1, initial=-np.inf)
        ex = np.exp(l - mx[:, None])
        return ex / ex.sum(axis=1, keepdims=True)


def arg_max(l):
    """First-index arg-max of the fp32 probabilities, read off the logits: entries that are equal or >= GRID apart order
    their probabilities the same way (e^GRID - 1 ~ 1e-3 against 2^-20); a row of NaN probabilities never passes `pr > pb`
    and keeps index 0."""
    l = np.asarray(l, F32)
    poisoned = np.isnan(softmax64(l)).any(axis=1)
    with np.errstate(invalid="ignore"):
        return np.where(poisoned, 0, np.argmax(np.where(np.isnan(l), -np.inf, l), axis=1)).astype(np.int32)


def probs_error(got, want):
    """Largest |got - want| / max(want, 1e-30); inf when the NaN patterns differ."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - want[ok]) / np.maximum(want[ok], 1e-30)).max())


def lists_of(expert, E):
    """Routing lists as sets: list e = the rows with expert e (rows outside 0 .. E - 1 are in no list)."""
    expert = np.asarray(expert)
    return [set(np.nonzero(expert == e)[0].tolist()) for e in range(E)]


# ---- the two-stage gate -------------------------------------------------------------------------------------------------
def gate_flag(logits, tau, widen, cstat, fcounts, cap, n_rounds, rstat=None):
    """gate_begin + gate_flag + round_counts on logits [B, E].  Updates cstat and fcounts (int32 [128]) in place and returns
    dict(probs fp64, expert, flags set, tau_eff f32)."""
    l = np.asarray(logits, F32)
    B = l.shape[0]
    tau_eff = F32(tau) if rstat is not None else np.fmax(F32(tau), F32(widen) * bits_f32(cstat[3]))
    margin, nonfinite = top2_margin(l)
    with np.errstate(invalid="ignore"):
        flag = nonfinite | ~(margin >= tau_eff)
    fcounts[0] = int(flag.sum())
    fcounts[FC_WIDEN_COUNT] = 0
    fcounts.view(F32)[FC_TAU_EFF] = tau_eff
    fcounts[FC_ROUND_COUNTS:FC_ROUND_COUNTS + n_rounds] = round_counts([fcounts[0]], cap, n_rounds)
    cstat[0] += B
    cstat[1] += int(flag.sum())
    return {"probs": softmax64(l), "expert": arg_max(l), "flags": set(np.nonzero(flag)[0].tolist()), "tau_eff": tau_eff}


def gate_widen(keep, E, widen, cstat, fcounts, cap, n_rounds):
    """gate_widen_begin + gate_widen + gate_widen_end on the kept logits [B, >= E].  Returns the set of rows in the band."""
    k = np.asarray(keep, F32)[:, :E]
    fv = fcounts.view(F32)
    lower = fv[FC_TAU_EFF]
    upper = F32(widen) * bits_f32(cstat[3])
    fv[FC_WIDEN_UPPER] = upper
    rows = set()
    if upper > lower:
        margin, nonfinite = top2_margin(k)
        with np.errstate(invalid="ignore"):
            rows = set(np.nonzero(~nonfinite & (margin >= lower) & (margin < upper))[0].tolist())
        fv[FC_TAU_EFF] = upper
    n = len(rows)
    fcounts[FC_WIDEN_COUNT] = n
    fcounts[FC_WIDEN_ROUNDS:FC_WIDEN_ROUNDS + n_rounds] = round_counts([n], cap, n_rounds)
    cstat[1] += n
    cstat[6] += n
    cstat[7] += 1 if n else 0
    return rows


def pair_errors(keep_rows, exact_rows, a):
    """pe [n, E] f32 = |(k_a - k_e) - (l_a - l_e)|, operation by operation"""
    k, l = np.asarray(keep_rows, F32), np.asarray(exact_rows, F32)
    r = np.arange(len(a))
    with np.errstate(invalid="ignore"):
        d16 = (k[r, a][:, None] - k).astype(F32)
        return np.abs((d16 - (l[r, a][:, None] - l).astype(F32)).astype(F32))


def gate_recheck(exact, rows, keep, expert, cstat, fcounts, widen, rstat=None):
    """gate_recheck on the listed `rows` (any order): exact [B, E] holds the second gate's logits of every row, keep [B, >= E]
    the kept ones, expert [B] the filter's arg-max (updated in place).  Returns the rows' probabilities in fp64, [len(rows), E]."""
    rows = np.asarray(sorted(rows), np.int64)
    l = np.asarray(exact, F32)[rows]
    E = l.shape[1]
    if len(rows) == 0:
        return np.zeros((0, E))
    a = np.asarray(expert)[rows].astype(np.int64)
    pe = pair_errors(np.asarray(keep, F32)[rows, :E], l, a)
    fin = np.isfinite(pe)
    pz = np.where(fin, pe, F32(0))
    err = pz.max(axis=1)
    best = arg_max(l)
    expert[rows] = best
    cstat[2] += int((best != a).sum())
    cstat[3] = max(cstat[3], f32_bits(err.max()))
    cstat[4] += float((pz.astype(np.float64) ** 2).sum())
    cstat[5] += int((fin & (np.arange(E)[None, :] != a[:, None])).sum())
    if rstat is not None:
        rstat[0] += int((F32(widen) * err > fcounts.view(F32)[FC_TAU_EFF]).sum())
    return softmax64(l)


def gate_cascade(filt, exact, tau, widen, passes, cstat, rstat=None):
    """The host sequence of model.hip: gate_cascade over one batch whose rows fit one round: the filter pass's logits `filt` and
    the exact gate's logits `exact` of every row (a routed row does not depend on its place in a list).  Returns (probs fp64,
    expert, decided-twice mask)."""
    B, E = filt.shape
    fcounts = np.zeros(128, np.int32)
    keep = np.zeros((B, MAX_EXPERTS), F32)
    keep[:, :E] = filt
    r = gate_flag(filt, tau, widen, cstat, fcounts, B, 1, rstat)
    probs, expert = r["probs"].copy(), r["expert"].copy()
    twice = np.zeros(B, bool)
    rows = r["flags"]
    for p in range(1 if rstat is not None else passes + 1):
        if p >= 1:
            rows = gate_widen(keep, E, widen, cstat, fcounts, B, 1)
        idx = sorted(rows)
        probs[idx] = gate_recheck(exact, rows, keep, expert, cstat, fcounts, widen, rstat)
        twice[idx] = True
    return probs, expert, twice


# ---- the conditioning guard --------------------------------------------------------------------------------------------
def x8_guard_begin(pass_, thr, scale, B, gstat, slot, rstat=None):
    """gstat: [0] queries [1] re-evaluated [2] max_dn bits [3] dropped; slot: f32 [2], the |n| band"""
    hi = F32(thr) if rstat is not None else np.fmax(F32(thr), F32(scale) * bits_f32(gstat[2]))
    if pass_ == 0:
        slot[0], slot[1] = F32(0), hi
        gstat[0] += B
    else:
        slot[0], slot[1] = slot[1], np.fmax(hi, slot[1])


def x8_guard_flag(rows, normals, slot, cap, gstat):
    """rows: the live part of one routing list.  Returns (the rows in the band or with a NaN norm -- fp64 norm; the band edges are
    midpoints between norms >= 2^-10 relative apart --, the listed count min(cap, .)); the device count is the set's size."""
    n = np.asarray(normals, F32).astype(np.float64)[list(rows)]
    r = np.sqrt((n * n).sum(axis=1))
    with np.errstate(invalid="ignore"):
        hit = np.isnan(r) | ((r >= float(slot[0])) & (r < float(slot[1])))
    band = set(np.asarray(list(rows))[hit].tolist())
    gstat[3] += max(0, len(band) - cap)
    return band, min(cap, len(band))


def x8_guard_fix(src_rows, listed, normals, gstat, thr, scale, rstat=None):
    """src_rows[j] replaces normals[listed[j]] (in place); returns max_dn in fp64 (0 when nothing finite and positive was measured),
    to be compared within DN_REL; gstat[2] is left to the caller.  The rstat[1] decision scale * dn > thr must be clear of
    DN_REL (asserted)."""
    src, listed = np.asarray(src_rows, F32), list(listed)
    gstat[1] += len(listed)
    if not listed:
        return 0.0
    old = np.asarray(normals, F32)[listed].astype(np.float64)
    dn = np.sqrt(((src[:, :3].astype(np.float64) - old) ** 2).sum(axis=1))
    normals[listed] = src[:, :3]
    ok = np.isfinite(dn)
    if rstat is not None and ok.any():
        x = float(scale) * dn[ok]
        assert (np.abs(x - float(thr)) > 8 * DN_REL * float(thr)).all(), "crafted |dn| too close to the violation threshold"
        rstat[1] += int((x > float(thr)).sum())
    return float(dn[ok & (dn > 0)].max()) if (ok & (dn > 0)).any() else 0.0


# ---- the rest -----------------------------------------------------------------------------------------------------------
def stat_max_import(word, values):
    """word = max(word, bits of every v with 0 < v < inf) (NaN compares false)"""
    for v in np.asarray(values, F32):
        if v > 0 and v < np.inf:
            word = max(word, f32_bits(v))
    return word


def switch_finish(noise, threshold):
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(noise, F32) < F32(threshold), 0, 1).astype(np.int32)     # NaN -> tower 1


def mask_empty(n_eff, normals, expert, probs):
    empty = ~(np.asarray(n_eff) > 0).any(axis=1)
    normals[empty] = 0
    if expert is not None:
        expert[empty] = -1
    if probs is not None:
        probs[empty] = 0
    return empty


# ---- crafted inputs -------------------------------------------------------------------------------------------------------
TAU_X = F32(0.3125)      # the threshold the "margin exactly tau" rows are built for (on the grid)
LSTRIDE = 64


def crafted_logits(B, E, seed):
    """([B, LSTRIDE] f32 with garbage -- NaN, inf, huge -- in the columns >= E, {name: row} of the fixed rows).  Random rows: entries
    on the grid k * GRID, |k| <= 4096, so pairwise equal or >= GRID apart (ties are frequent: 1 in 4 entries repeats another)."""
    rng = np.random.default_rng(seed)
    full = np.empty((B, LSTRIDE), F32)
    g = rng.integers(0, 4, size=full.shape)
    full[:] = np.choose(g, [np.nan, np.inf, 3e38, -7.0]).astype(F32)
    k = rng.integers(-4096, 4097, size=(B, E))
    rep = rng.random((B, E)) < 0.25
    for e in range(1, E):
        k[:, e] = np.where(rep[:, e], k[np.arange(B), rng.integers(0, e, size=B)], k[:, e])
    full[:, :E] = (k * GRID).astype(F32)
    low = (-(np.arange(E) + 2.0)).astype(F32)              # -2, -3, ...: a background below every crafted entry
    fixed = {}

    def row(name, vals):
        fixed[name] = (7 + 23 * len(fixed)) % B if len(fixed) % 2 else B - 1 - (5 * len(fixed)) % 44   # both blocks, the last wave
        full[fixed[name], :E] = np.asarray(vals, F32)

    def with_(pairs):
        v = low.copy()
        for i, x in pairs:
            v[i] = x
        return v

    row("all_equal", np.full(E, 0.75))
    row("pm80", with_([(0, 80.0)] + ([(E - 1, -80.0)] if E > 1 else [])))
    row("one_nan", with_([(0, 3.0), (E - 1, np.nan)]) if E > 1 else [np.nan])
    row("all_nan", np.full(E, np.nan))
    row("one_pinf", with_([(E // 2, np.inf)]))
    row("one_ninf", with_([(0, 2.0), (E - 1, -np.inf)]) if E > 1 else [-np.inf])
    if E >= 2:
        row("two_pinf", with_([(0, np.inf), (E - 1, np.inf)]))
        row("pinf_and_nan", with_([(0, np.nan), (E - 1, np.inf)]))
        row("margin_eq_tau", with_([(1, TAU_X), (0, 0.0)]))
        row("margin_below_tau", with_([(1, np.nextafter(TAU_X, F32(0))), (0, 0.0)]))
        row("margin_above_tau", with_([(0, np.nextafter(TAU_X, F32(1))), (1, 0.0)]))
    if E >= 3:
        row("ninf_close", with_([(0, 1.0), (1, 0.5), (E - 1, -np.inf)]))     # a finite top-2 margin inside the widening bands
    if E >= 4:
        row("tie_0_3", with_([(0, 1.5), (3, 1.5), (1, 1.0)]))
    if E >= 7:
        row("tie_5_6", with_([(5, 0.25), (6, 0.25), (0, -0.5)]))
    assert len(set(fixed.values())) == len(fixed)
    return full, fixed


def crafted_exact(filt, E, fixed, seed):
    """The second gate's logits [B, E] for crafted_logits' rows: the filter's plus k * 2^-12, |k| <= 64 (a quarter of the rows: 0);
    finite on the filter's non-finite rows except all_nan (the exact gate sees a NaN too) and two_pinf (+inf), and NaN / +inf on one
    row each whose filter logits are finite."""
    rng = np.random.default_rng(seed + 1)
    B = filt.shape[0]
    d = rng.integers(-64, 65, size=(B, E)) * 2.0 ** -12
    d[rng.random(B) < 0.25] = 0
    x = (filt[:, :E].astype(np.float64) + d).astype(F32)
    bad = ~np.isfinite(x).all(axis=1)
    x[bad] = (rng.integers(-4096, 4097, size=(int(bad.sum()), E)) * GRID).astype(F32)
    extra = {}
    if "all_nan" in fixed:
        x[fixed["all_nan"], E - 1] = np.nan
    if "two_pinf" in fixed:
        x[fixed["two_pinf"], 0] = np.inf
    # ... on rows the filter flags at TAU_X (a tie or a small margin), so that the recheck meets them
    margin, _ = top2_margin(filt[:, :E])
    free = [b for b in range(B) if b not in fixed.values() and (E == 1 or margin[b] <= TAU_X / 2)]
    assert len(free) >= 2
    extra["exact_nan"], extra["exact_pinf"] = free[1], free[-1]
    x[extra["exact_nan"], 0] = np.nan
    x[extra["exact_pinf"], E - 1] = np.inf
    return x, extra


def margin_midpoint(margins, fraction):
    """A threshold strictly between two neighbouring distinct finite margins, about `fraction` of the way up the sorted list"""
    m = np.unique(np.asarray(margins, F32)[np.isfinite(margins)])
    assert len(m) >= 2
    i = min(max(int(fraction * len(m)), 1), len(m) - 1)
    t = F32((np.float64(m[i - 1]) + np.float64(m[i])) / 2)
    assert m[i - 1] < t < m[i]
    return t


def crafted_normals(B, seed):
    """(normals [B, 3] f32, norms fp64 sorted ascending with their rows): row norms 2^-12 * 1.01^i in random directions -- neighbours
    1 % apart, far more than 2^-10 --, plus one NaN row and one zero row (returned apart)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(B, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    order = rng.permutation(B)
    want = np.empty(B)
    want[order] = 2.0 ** -12 * 1.01 ** np.arange(B)
    n = (d * want[:, None]).astype(F32)
    nan_row, zero_row = int(order[B // 3]), int(order[B // 2])
    n[nan_row] = [0.1, np.nan, 0.2]
    n[zero_row] = 0
    return n, nan_row, zero_row


def norms64(normals):
    n = np.asarray(normals, F32).astype(np.float64)
    return np.sqrt((n * n).sum(axis=1))
