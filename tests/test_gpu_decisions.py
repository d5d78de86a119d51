"""The kernels that DECIDE (csrc/decide.hip) against tests/decision_ref.py, the numpy restatement of each.

Part A: every launcher alone through nesti_debug_decision_step, on crafted caller buffers: B = 300 rows (two 256-thread blocks,
the last wave with 44 live lanes), logits of stride 64 with garbage beyond column E, E in {1, 2, 7, 8}, entries pairwise equal or
>= 2^-10 apart so that no tolerance touches a decision, and the fixed rows of decision_ref.crafted_logits (exact ties, margins on
and one ulp around the threshold, NaN / +inf / -inf, exp underflow).  Every output buffer is pre-filled, so a stray write shows.
Decisions, counts, thresholds and max-as-bits words are compared exactly; probabilities, the squared sum and max_dn under the bounds
decision_ref states.  Lists filled with atomics are compared as sets.

Part B: the host sequence of the two-stage gate through the product at B = 37: the filter's and the exact gate's logits come from
stepping the gating net launch by launch (layer_ref.TowerChecker), the restatement predicts nesti_gate_forward's outputs and every
field of nesti_model_cascade_stats.  Two biases of the synthetic gate's last layer are moved so that widening passes find rows."""
import ctypes
import math

import numpy as np
import pytest
import torch

import decision_ref as R

pytestmark = pytest.mark.gpu

B = 300
ES = (1, 2, 7, 8)
CAP, ROUNDS = 16, 19                  # ceil(300 / 16): the rounds partition a list longer than one cap
WIDEN = 1.5


# ---- plumbing -------------------------------------------------------------------------------------------------------------
class Dev:
    """Caller buffers on the device and one call per launcher."""

    def __init__(self, device):
        from nesti_net_amd import _lib
        self.L, self.lib, self.device = _lib, _lib.load(), device
        self.ops = {n: i for i, n in enumerate(_lib.DECISION_OPS)}

    def put(self, a):
        return torch.as_tensor(np.ascontiguousarray(a), device=self.device)

    def full(self, shape, value, dtype):
        return torch.full(shape, value, dtype=dtype, device=self.device)

    def counters(self, words):
        """8 x uint64 from a decision_ref block ([4] may be a float: the double's bits)"""
        w = np.zeros(8, np.uint64)
        for i, v in enumerate(words):
            w[i] = np.asarray([v], np.float64).view(np.uint64)[0] if isinstance(v, float) else v
        return self.put(w.view(np.int64))

    def step(self, op, rc=0, **kw):
        a = self.L.CDebugDecision()
        for k, v in kw.items():
            setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
        got = self.lib.nesti_debug_decision_step(self.ops[op], ctypes.byref(a),
                                                 ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        torch.cuda.synchronize(self.device)
        if rc == 0:
            self.L.check(got, "nesti_debug_decision_step(%s)" % op)
        else:
            assert got != 0
        return got


def host(t):
    return t.cpu().numpy()


def words(t):
    return [int(v) for v in host(t).view(np.uint64)]


def dbl(word):
    return float(np.asarray([word], np.uint64).view(np.float64)[0])


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def dev(gpu_device):
    return Dev(gpu_device)


@pytest.fixture(scope="module", params=ES)
def rows(request):
    E = request.param
    full, fixed = R.crafted_logits(B, E, seed=E)
    exact, extra = R.crafted_exact(full, E, fixed, seed=E)
    margin, nonfinite = R.top2_margin(full[:, :E])
    return E, full, fixed, exact, extra, margin, nonfinite


CSTAT0 = [10, 20, 30, 0, 2.5, 40, 50, 60]     # preset counters: the kernels ADD to them


def _cstat(err):
    c = list(CSTAT0)
    c[3] = R.f32_bits(err)
    return c


def _flag_buffers(dev, E):
    return {"probs": dev.full((B, E), -3.0, torch.float32), "expert": dev.full((B,), -7, torch.int32),
            "keep": dev.full((B, R.MAX_EXPERTS), 123.0, torch.float32), "fcounts": dev.full((128,), 0x5A5A5A5A, torch.int32),
            "flag_list": dev.full((B,), -1, torch.int32)}


def _run_flag(dev, full, E, tau, err, with_rstat, probs=True):
    """launch_gate_flag on fresh buffers -> (buffers, reference result, reference cstat, reference fcounts)"""
    buf = _flag_buffers(dev, E)
    cst = _cstat(err)
    buf["cstat"] = dev.counters(cst)
    buf["rstat"] = dev.counters([7, 8, 0, 0, 0, 0, 0, 0]) if with_rstat else None
    dev.step("gate_flag", logits=dev.put(full), lstride=R.LSTRIDE, B=B, E=E, tau=tau, widen=WIDEN, cap=CAP, n_rounds=ROUNDS,
             probs=buf["probs"] if probs else None, expert=buf["expert"], keep=buf["keep"], fcounts=buf["fcounts"],
             flag_list=buf["flag_list"], cstat=buf["cstat"], rstat=buf["rstat"] if with_rstat else None)
    fc = np.full(128, 0x5A5A5A5A, np.int32)
    ref = R.gate_flag(full[:, :E], tau, WIDEN, cst, fc, CAP, ROUNDS, rstat=[7, 8] if with_rstat else None)
    return buf, ref, cst, fc


def _check_list(lst, n, want, what):
    lst = host(lst)
    assert sorted(lst[:n].tolist()) == sorted(want), "%s: the list is not the predicted set" % what
    assert (lst[n:] == -1).all(), "%s: entries beyond the count were written" % what


def _check_cstat(got_words, want, what):
    for i in (0, 1, 2, 3, 5, 6, 7):
        assert got_words[i] == want[i], "%s: cstat[%d] = %d, predicted %d" % (what, i, got_words[i], want[i])


# ---- part A: the two-stage gate -------------------------------------------------------------------------------------------
def test_gate_flag(dev, rows):
    E, full, fixed, exact, extra, margin, nonfinite = rows
    taus = [0.0, float(R.TAU_X), 1e30] + ([float(R.margin_midpoint(margin[~nonfinite], 1 / 3))] if E > 1 else [])
    for tau in taus:
        for err in (0.0, 0.5):                       # 1.5 x 0.5 > every tau but 1e30: the threshold follows the measured error
            for with_rstat in (False, True):
                what = "gate_flag E=%d tau=%g err=%g rstat=%s" % (E, tau, err, with_rstat)
                buf, ref, cst, fc = _run_flag(dev, full, E, tau, err, with_rstat)
                got_n = int(host(buf["fcounts"])[0])
                assert 0 <= got_n <= B
                for name, b in fixed.items():
                    assert (b in host(buf["flag_list"])[:got_n]) == (b in ref["flags"]), \
                        "%s: row %s is %sflagged" % (what, name, "not " if b in ref["flags"] else "")
                assert np.array_equal(host(buf["fcounts"]), fc), what + ": fcounts (flag count, round counts, tau_eff bits, untouched words)"
                want_tau = np.float32(tau) if with_rstat else max(np.float32(tau), np.float32(WIDEN) * np.float32(err))
                assert host(buf["fcounts"]).view(np.float32)[R.FC_TAU_EFF] == want_tau
                n = int(fc[0])
                _check_list(buf["flag_list"], n, ref["flags"], what)
                assert np.array_equal(host(buf["expert"]), ref["expert"]), what + ": expert"
                perr = R.probs_error(host(buf["probs"]), ref["probs"])
                print(what, "flags", n, "probs rel err %.3g" % perr)
                assert perr <= R.PROB_REL, what + ": probabilities"
                k = host(buf["keep"])
                assert np.array_equal(bits(k[:, :E]), bits(full[:, :E])) and (k[:, E:] == 123.0).all(), what + ": keep"
                w = words(buf["cstat"])
                _check_cstat(w, cst, what)
                assert dbl(w[4]) == 2.5
                if with_rstat:
                    assert words(buf["rstat"])[:2] == [7, 8]
    buf, ref, cst, fc = _run_flag(dev, full, E, 0.25, 0.0, False, probs=False)      # probs is optional
    assert np.array_equal(host(buf["expert"]), ref["expert"]) and (host(buf["probs"]) == -3.0).all()


def _upper_on_a_margin(margin, nonfinite):
    """(err, upper): upper = 1.5 x err in fp32 lands exactly on the margin of an existing row above TAU_X"""
    k = np.round(margin[~nonfinite & np.isfinite(margin)].astype(np.float64) / R.GRID).astype(np.int64)
    k = np.unique(k[(k % 3 == 0) & (k * R.GRID > 2 * float(R.TAU_X))])
    assert len(k), "no crafted margin is a multiple of 3 x 2^-10"
    upper = np.float32(k[0] * R.GRID)
    err = np.float32(float(upper) / 1.5)
    assert np.float32(WIDEN) * err == upper
    return err, upper


def test_gate_widen(dev, rows):
    E, full, fixed, exact, extra, margin, nonfinite = rows
    keep = np.full((B, R.MAX_EXPERTS), 123.0, np.float32)
    keep[:, :E] = full[:, :E]
    cases = [(float(R.TAU_X), 0.5), (0.75, 0.5), (0.75, 0.25), (0.0, 2.0)]       # (lower, err): the 2nd and 3rd have upper <= lower
    if E > 1:
        err, upper = _upper_on_a_margin(margin, nonfinite)
        cases.append((float(R.TAU_X), float(err)))
    for lower, err in cases:
        what = "gate_widen E=%d lower=%g err=%g" % (E, lower, err)
        fc = np.full(128, 0x5A5A5A5A, np.int32)
        fc.view(np.float32)[R.FC_TAU_EFF] = lower
        cst = _cstat(err)
        d_fc, d_list, d_cstat = dev.put(fc), dev.full((B,), -1, torch.int32), dev.counters(cst)
        dev.step("gate_widen", keep=dev.put(keep), B=B, E=E, widen=WIDEN, fcounts=d_fc, flag_list=d_list, cap=CAP, n_rounds=ROUNDS,
                 cstat=d_cstat)
        want = R.gate_widen(keep, E, WIDEN, cst, fc, CAP, ROUNDS)
        assert np.array_equal(host(d_fc), fc), what + ": fcounts (upper, count, round counts, tau_eff)"
        _check_list(d_list, len(want), want, what)
        w = words(d_cstat)
        _check_cstat(w, cst, what)
        assert dbl(w[4]) == 2.5
        got = set(host(d_list)[:len(want)].tolist())
        if 1.5 * err <= lower:
            assert not got and host(d_fc).view(np.float32)[R.FC_TAU_EFF] == np.float32(lower)
        elif E > 1:
            assert not got & set(np.nonzero(nonfinite)[0].tolist()), what + ": a row with a non-finite logit was widened"
            if "ninf_close" in fixed and lower <= 0.5:
                assert margin[fixed["ninf_close"]] == 0.5 < 1.5 * err, "the -inf row's finite margin lies in the band"
            if lower == float(R.TAU_X):
                assert fixed["margin_eq_tau"] in got and fixed["margin_above_tau"] in got and fixed["margin_below_tau"] not in got
        print(what, "rows", len(want))
    if E > 1:
        on_upper = set(np.nonzero(~nonfinite & (margin == upper))[0].tolist())
        assert on_upper and not on_upper & got, "a row with margin exactly `upper` belongs to the NEXT band"


@pytest.mark.parametrize("with_rstat", [False, True])
def test_gate_recheck(dev, rows, with_rstat):
    """All 19 rounds of the filter's flag list: full rounds (count = cap), the partial one, the empty ones."""
    E, full, fixed, exact, extra, margin, nonfinite = rows
    tau = float(R.TAU_X)
    buf, ref, cst, fc = _run_flag(dev, full, E, tau, 0.0, with_rstat)
    fc = host(buf["fcounts"]).copy()               # the rounds are the DEVICE's (test_gate_flag compares them with the prediction)
    n = int(fc[0])
    lst = host(buf["flag_list"])
    assert 0 <= n <= B and len(set(lst[:n].tolist())) == n and ((0 <= lst[:n]) & (lst[:n] < B)).all()
    xfull = np.full((B, R.LSTRIDE), np.nan, np.float32)
    xfull[:, :E] = exact
    d_exact = dev.put(xfull)
    p0, e0 = host(buf["probs"]).copy(), host(buf["expert"]).copy()
    keep = host(buf["keep"])
    expert = e0.copy()
    rstat = [7, 8] if with_rstat else None
    probs_ref = {}
    counts_seen = set()
    for r in range(ROUNDS):
        seg = buf["flag_list"][r * CAP:(r + 1) * CAP]
        count = int(fc[R.FC_ROUND_COUNTS + r])
        counts_seen.add(count)
        compact = d_exact[seg.long().clamp_min(0)].contiguous()       # the second gate's logits, gathered through the device's list
        before = words(buf["cstat"])
        dev.step("gate_recheck", logits=compact, lstride=R.LSTRIDE, flag_list=seg, count_ptr=buf["fcounts"][R.FC_ROUND_COUNTS + r:],
                 cap=CAP, E=E, keep=buf["keep"], probs=buf["probs"], expert=buf["expert"], cstat=buf["cstat"], fcounts=buf["fcounts"],
                 widen=WIDEN, rstat=buf["rstat"] if with_rstat else None)
        listed = lst[r * CAP:r * CAP + count].tolist()
        p = R.gate_recheck(exact, listed, keep, expert, cst, fc, WIDEN, rstat)
        probs_ref.update(zip(sorted(listed), p))
        if count == 0:
            assert words(buf["cstat"]) == before, "an empty round changed the counters"
    if E > 1:
        assert counts_seen >= {0, CAP} and any(0 < c < CAP for c in counts_seen)
    w = words(buf["cstat"])
    what = "gate_recheck E=%d" % E
    print(what, "rows", n, "max_margin_err %.6g" % R.bits_f32(w[3]), "sum %.9g (predicted %.9g)" % (dbl(w[4]), cst[4]), "pairs", w[5],
          "changed", w[2] - 30)
    assert math.isfinite(dbl(w[4])), what + ": sum_sq_pair_err is not finite (a non-finite pair error was summed)"
    assert math.isfinite(float(R.bits_f32(w[3]))), what + ": max_margin_err is not finite"
    assert set(lst[:n].tolist()) == ref["flags"], what + ": the filter's flag list is not the predicted set"
    for name in ("one_nan", "all_nan", "one_pinf", "two_pinf", "one_ninf", "pinf_and_nan", "ninf_close"):
        assert name not in fixed or fixed[name] in ref["flags"]
    assert E == 1 or {extra["exact_nan"], extra["exact_pinf"]} <= ref["flags"]
    _check_cstat(w, cst, what)
    assert abs(dbl(w[4]) - cst[4]) <= R.SUM_REL * cst[4], what + ": sum_sq_pair_err"
    if with_rstat:
        assert words(buf["rstat"])[:2] == rstat, what + ": gate_violations"
        assert rstat[0] > 7 or E <= 2          # E >= 7: the one_ninf row's finite pairs are units apart
    listed = np.zeros(B, bool)
    listed[lst[:n]] = True
    got_p, got_e = host(buf["probs"]), host(buf["expert"])
    assert np.array_equal(got_e, expert), what + ": expert"
    assert np.array_equal(bits(got_p[~listed]), bits(p0[~listed])) and np.array_equal(got_e[~listed], e0[~listed]), \
        what + ": rows outside the list were touched"
    want_p = np.stack([probs_ref[b] for b in sorted(probs_ref)]) if probs_ref else np.zeros((0, E))
    perr = R.probs_error(got_p[sorted(probs_ref)], want_p)
    assert perr <= R.PROB_REL, what + ": probabilities of the listed rows (%.3g)" % perr
    assert np.array_equal(host(buf["fcounts"]), fc) and np.array_equal(bits(host(buf["keep"])), bits(keep))


def test_gate_finish_and_route(dev, rows):
    E, full, fixed, exact, extra, margin, nonfinite = rows
    d_logits = dev.put(full)
    probs, expert = dev.full((B, E), -3.0, torch.float32), dev.full((B,), -7, torch.int32)
    counts, lists = dev.full((R.MAX_EXPERTS,), 99, torch.int32), dev.full((E, B), -1, torch.int32)
    dev.step("gate_finish", logits=d_logits, lstride=R.LSTRIDE, B=B, E=E, probs=probs, expert=expert, counts=counts, lists=lists)
    want_e, want_p = R.arg_max(full[:, :E]), R.softmax64(full[:, :E])
    assert np.array_equal(host(expert), want_e)
    assert R.probs_error(host(probs), want_p) <= R.PROB_REL
    sets = R.lists_of(want_e, E)
    c = host(counts)
    assert c[:E].tolist() == [len(s) for s in sets] and (c[E:] == 99).all()
    for e in range(E):
        _check_list(lists[e], len(sets[e]), sets[e], "gate_finish list %d" % e)
    # every output is optional
    e2 = dev.full((B,), -7, torch.int32)
    dev.step("gate_finish", logits=d_logits, lstride=R.LSTRIDE, B=B, E=E, expert=e2)
    assert np.array_equal(host(e2), want_e)
    p2 = dev.full((B, E), -3.0, torch.float32)
    dev.step("gate_finish", logits=d_logits, lstride=R.LSTRIDE, B=B, E=E, probs=p2)
    assert np.array_equal(bits(host(p2)), bits(host(probs)))
    # route: a caller-supplied assignment with rows outside 0 .. E - 1, which are in no list
    rng = np.random.default_rng(E)
    ex = rng.integers(-1, E + 1, size=B).astype(np.int32)
    counts, lists = dev.full((R.MAX_EXPERTS,), 99, torch.int32), dev.full((E, B), -1, torch.int32)
    dev.step("route", expert=dev.put(ex), B=B, E=E, counts=counts, lists=lists)
    sets = R.lists_of(ex, E)
    assert (ex == -1).any() and (ex == E).any() and sum(len(s) for s in sets) < B
    assert host(counts)[:E].tolist() == [len(s) for s in sets] and (host(counts)[E:] == 99).all()
    for e in range(E):
        _check_list(lists[e], len(sets[e]), sets[e], "route list %d" % e)


def test_switch_finish(dev):
    thr = np.float32(0.015)
    rng = np.random.default_rng(2)
    full = np.full((B, R.LSTRIDE), np.nan, np.float32)
    full[:, 0] = (thr + rng.integers(-200, 201, size=B) * np.float32(2.0 ** -14)).astype(np.float32)
    full[[3, 257]] = thr                                     # exactly at the threshold: tower 1
    full[[4, 299], 0] = np.nextafter(thr, np.float32(0))
    full[[5, 270], 0] = np.nan                               # a NaN noise estimate: tower 1
    full[[6, 280], 0] = [np.inf, -np.inf]
    probs, expert = dev.full((B,), -3.0, torch.float32), dev.full((B,), -7, torch.int32)
    counts, lists = dev.full((4,), 99, torch.int32), dev.full((2, B), -1, torch.int32)
    dev.step("switch_finish", logits=dev.put(full), lstride=R.LSTRIDE, B=B, thr=float(thr), probs=probs, expert=expert, counts=counts,
             lists=lists)
    want = R.switch_finish(full[:, 0], thr)
    assert want[[3, 257, 5, 270, 6]].tolist() == [1] * 5 and want[[4, 299, 280]].tolist() == [0] * 3
    assert np.array_equal(host(expert), want) and np.array_equal(bits(host(probs)), bits(full[:, 0]))
    sets = R.lists_of(want, 2)
    assert host(counts).tolist() == [len(sets[0]), len(sets[1]), 99, 99]
    for t in range(2):
        _check_list(lists[t], len(sets[t]), sets[t], "switch_finish list %d" % t)
    e2 = dev.full((B,), -7, torch.int32)
    dev.step("switch_finish", logits=dev.put(full), lstride=R.LSTRIDE, B=B, thr=float(thr), expert=e2)
    assert np.array_equal(host(e2), want)


def test_scatter3(dev):
    rng = np.random.default_rng(4)
    N, cap, stride = 400, 300, 5
    src = rng.normal(size=(cap, stride)).astype(np.float32)
    src[7, 1] = np.nan
    index = rng.permutation(N)[:cap].astype(np.int32)
    base = rng.normal(size=(N, 3)).astype(np.float32)
    d_src, d_idx, d_cnt = dev.put(src), dev.put(index), dev.put(np.asarray([261, 0, 1000], np.int32))
    for use_idx in (True, False):
        for cnt_at in (None, 0, 1, 2):                        # no count pointer; 261 (a partial second block); 0; beyond the cap
            out = dev.put(base)
            dev.step("scatter3", src=d_src, sstride=stride, index=d_idx if use_idx else None,
                     count_ptr=d_cnt[cnt_at:] if cnt_at is not None else None, cap=cap, normals=out)
            n = cap if cnt_at is None else min(cap, [261, 0, 1000][cnt_at])
            want = base.copy()
            want[index[:n] if use_idx else np.arange(n)] = src[:n, :3]
            assert np.array_equal(bits(host(out)), bits(want)), "scatter3 index=%s count=%s" % (use_idx, cnt_at)


def test_round_counts(dev):
    counts = np.asarray([0, 1, 15, 16, 17, 383, 384, 1000], np.int32)
    out = dev.full((8 * 24 + 8,), -1, torch.int32)
    dev.step("round_counts", counts=dev.put(counts), n_lists=8, cap=16, n_rounds=24, round_out=out)
    assert np.array_equal(host(out)[:192], R.round_counts(counts, 16, 24)) and (host(out)[192:] == -1).all()
    big = dev.full((11 * 24,), -1, torch.int32)
    dev.step("round_counts", rc=1, counts=dev.put(np.zeros(11, np.int32)), n_lists=11, cap=16, n_rounds=24, round_out=big)
    assert dev.lib.nesti_last_error().decode() == "round_counts: too many lists x rounds" and (host(big) == -1).all()


def test_stat_max_import_export(dev):
    den = np.float32(1e-40)
    vals = np.asarray([np.nan, np.inf, -1.0, 0.0, den, 0.5, 3.25, 1e-3, -np.inf, 3.2499998], np.float32)
    for start, src in ((0, vals), (0, vals[:5]), (R.f32_bits(7.0), vals), (R.f32_bits(1e-3), vals[:5]), (0, vals[:4])):
        word = dev.counters([5, start, 6])            # the word between two others
        dev.step("stat_max_import", word=word[1:], src=dev.put(src), B=len(src))
        want = R.stat_max_import(start, src)
        assert words(word)[:3] == [5, want, 6], "stat_max_import from %#x" % start
        dst = dev.full((3,), -3.0, torch.float32)
        dev.step("stat_max_export", word=word[1:], dst=dst[1:])
        assert host(dst).view(np.uint32).tolist() == [R.f32_bits(-3.0), want, R.f32_bits(-3.0)]
    # more than one block of inputs
    many = np.abs(np.random.default_rng(1).normal(size=B)).astype(np.float32)
    word = dev.counters([0])
    dev.step("stat_max_import", word=word, src=dev.put(many), B=B)
    assert words(word)[0] == R.f32_bits(many.max())


@pytest.mark.parametrize("with_gate", [True, False])
def test_mask_empty_queries(dev, with_gate):
    rng = np.random.default_rng(6)
    M, S, E = 300, 3, 7
    n_eff = rng.integers(0, 3, size=(M, S)).astype(np.int32) * (rng.random((M, 1)) < 0.8)
    n_eff = n_eff.astype(np.int32)
    n_eff[[0, 255, 256, 299]] = 0
    n_eff[[1, 298]] = [[0, 0, 1], [1, 0, 0]]
    normals = rng.normal(size=(M, 3)).astype(np.float32)
    expert = rng.integers(0, E, size=M).astype(np.int32)
    probs = rng.random((M, E)).astype(np.float32)
    d_n, d_e, d_p = dev.put(normals), dev.put(expert), dev.put(probs)
    d_neff = dev.put(n_eff)
    rc = dev.lib.nesti_mask_empty_queries(dev.L.ptr(d_neff), M, S, dev.L.ptr(d_n), dev.L.ptr(d_e) if with_gate else None,
                                          dev.L.ptr(d_p) if with_gate else None, E,
                                          ctypes.c_void_p(torch.cuda.current_stream(dev.device).cuda_stream))
    dev.L.check(rc, "nesti_mask_empty_queries")
    torch.cuda.synchronize()
    empty = R.mask_empty(n_eff, normals, expert if with_gate else None, probs if with_gate else None)
    assert empty[[0, 255, 256, 299]].all() and not empty[[1, 298]].any() and 20 < empty.sum() < 150
    assert np.array_equal(bits(host(d_n)), bits(normals)) and np.array_equal(host(d_e), expert) and np.array_equal(bits(host(d_p)), bits(probs))


# ---- part A: the conditioning guard ----------------------------------------------------------------------------------------
def _midpoint(s, i):
    """fp32 midpoint of the sorted norms s[i - 1] < s[i]: at least 2^-9 relative away from both"""
    t = np.float32((s[i - 1] + s[i]) / 2)
    assert s[i - 1] * (1 + 2.0 ** -9) < t < s[i] * (1 - 2.0 ** -9)
    return t


def _clear(edge, s):
    assert (np.abs(s / float(edge) - 1) > 2.0 ** -10).all(), "a crafted band edge sits on a norm"


@pytest.mark.parametrize("with_rstat", [False, True])
def test_x8_guard(dev, with_rstat):
    E = 7
    normals, nan_row, zero_row = R.crafted_normals(B, 9)
    r = R.norms64(normals)
    s = np.sort(r[np.isfinite(r) & (r > 0)])
    rng = np.random.default_rng(10)
    ex = rng.integers(0, E, size=B)
    sets = R.lists_of(ex, E)
    lists = np.full((E, B), -1, np.int32)
    for e in range(E):
        lists[e, :len(sets[e])] = rng.permutation(sorted(sets[e]))
    d_lists, d_counts = dev.put(lists), dev.put(np.asarray([len(x) for x in sets] + [0], np.int32))
    d_normals = dev.put(normals)
    scale = 4.0
    thr = _midpoint(s, 40)                                           # the frozen threshold: 40 norms (and the zero row) below it
    dn0 = np.float32(float(s[70]) * 1.004 / scale)                   # what was measured asks for more: 71 norms below scale x dn0
    hi_meas = np.float32(scale) * dn0
    _clear(hi_meas, s)
    gst = [100, 200, R.f32_bits(dn0), 300]
    rst = [7, 8] if with_rstat else None
    d_gstat, d_rstat = dev.counters(gst), dev.counters(rst) if with_rstat else None
    d_slot = dev.full((4,), -3.0, torch.float32)
    slot = np.full(2, -3.0, np.float32)
    # pass 0: [0, max(thr, scale x max_dn)) -- in reproducible form [0, thr) whatever was measured
    dev.step("x8_guard_begin", pass_=0, thr=float(thr), scale=scale, B=B, gstat=d_gstat, slot=d_slot, rstat=d_rstat)
    R.x8_guard_begin(0, thr, scale, B, gst, slot, rst)
    assert slot[1] == (thr if with_rstat else hi_meas) and slot[0] == 0
    assert np.array_equal(bits(host(d_slot)), bits(np.concatenate([slot, [-3.0, -3.0]]).astype(np.float32))) and words(d_gstat)[:4] == gst
    glist, gcount = dev.full((E, B), -1, torch.int32), dev.full((E + 1,), 99, torch.int32)

    def flag_all(cap):
        total = set()
        for e in range(E):
            dev.step("x8_guard_flag", lists=d_lists[e], count_ptr=d_counts[e:], B=B, normals=d_normals, slot=d_slot, glist=glist[e],
                     gcount=gcount[e:], cap=cap, gstat=d_gstat)
            band, listed = R.x8_guard_flag(sets[e], normals, slot, cap, gst)
            assert int(host(gcount)[e]) == len(band), "x8_guard_flag list %d: count" % e
            got = host(glist[e])
            assert len(set(got[:listed].tolist())) == listed and set(got[:listed].tolist()) <= band and (got[cap:] == -1).all()
            if cap >= len(band):
                _check_list(glist[e], listed, band, "x8_guard_flag list %d" % e)
            total |= band
        assert words(d_gstat)[:4] == gst and int(host(gcount)[E]) == 99
        return total

    total = flag_all(B)                                              # cap larger than any band
    assert zero_row in total and nan_row in total and len(total) == int((s < float(slot[1])).sum()) + 2 >= 42
    # pass 1 after a larger measurement: [old upper end, max(scale x max_dn, old upper end)); pass 1 never takes rstat
    dn1 = np.float32(float(s[110]) * 1.004 / scale)
    _clear(np.float32(scale) * dn1, s)
    gst[2] = R.f32_bits(dn1)
    d_gstat = dev.counters(gst)
    dev.step("x8_guard_begin", pass_=1, thr=float(thr), scale=scale, B=B, gstat=d_gstat, slot=d_slot)
    R.x8_guard_begin(1, thr, scale, B, gst, slot)
    assert np.array_equal(bits(host(d_slot)[:2]), bits(slot)) and slot[0] > 0 and words(d_gstat)[:4] == gst
    glist.fill_(-1)
    total1 = flag_all(B)
    assert zero_row not in total1 and nan_row in total1 and not (total1 & total) - {nan_row}
    assert len(total1) == int(((s >= float(slot[0])) & (s < float(slot[1]))).sum()) + 1 >= 30
    # a full list: 9 rows in the band (8 norms and the NaN row), room for 4
    every = dev.put(np.arange(B, dtype=np.int32))
    lo, hi = _midpoint(s, 150), _midpoint(s, 158)
    d_slot2 = dev.put(np.asarray([lo, hi], np.float32))
    g4, c4 = dev.full((16,), -1, torch.int32), dev.full((2,), 99, torch.int32)
    dev.step("x8_guard_flag", lists=every, count_ptr=dev.put(np.asarray([B], np.int32)), B=B, normals=d_normals, slot=d_slot2, glist=g4,
             gcount=c4, cap=4, gstat=d_gstat)
    band, listed = R.x8_guard_flag(range(B), normals, np.asarray([lo, hi], np.float32), 4, gst)
    assert len(band) == 9 and listed == 4 and host(c4).tolist() == [9, 99]
    got = host(g4)
    assert len(set(got[:4].tolist())) == 4 and set(got[:4].tolist()) <= band and (got[4:] == -1).all()
    assert words(d_gstat)[:4] == gst and gst[3] == 305
    # an empty list (count 0), and a count above count_cap
    dev.step("x8_guard_flag", lists=every, count_ptr=d_counts[E:], B=B, normals=d_normals, slot=d_slot2, glist=g4, gcount=c4, cap=4,
             gstat=d_gstat)
    assert host(c4).tolist() == [0, 99] and words(d_gstat)[:4] == gst
    g9, c9 = dev.full((16,), -1, torch.int32), dev.full((2,), 99, torch.int32)
    dev.step("x8_guard_flag", lists=every, count_ptr=dev.put(np.asarray([10 * B], np.int32)), B=B, normals=d_normals, slot=d_slot2, glist=g9,
             gcount=c9, cap=16, gstat=d_gstat)
    _check_list(g9, 9, band, "x8_guard_flag, count above count_cap")
    # ---- fix: the listed rows take the replacement's bits and measure |dn| ---------------------------------------------------
    listed_rows = host(g9)[:9].tolist()
    stride = 5
    src = np.full((16, stride), 77.0, np.float32)
    step_ = rng.normal(size=(9, 3))
    step_ /= np.linalg.norm(step_, axis=1, keepdims=True)
    size = float(s[158]) * np.asarray([0.0, 0.5, 1, 2, 3, 4, 5, 6, 7.5])      # one row is replaced by itself: |dn| = 0
    old = normals[listed_rows].astype(np.float64)
    src[:9, :3] = np.where(np.isnan(old), 0.25, old + step_ * size[:, None]).astype(np.float32)
    fix_thr = np.float32(scale * float(s[158]) * 4.5)                # rows with |dn| of 5, 6 and 7.5 x violate
    for cap, count in ((16, 9), (6, 9), (16, 0)):
        nrm = normals.copy()
        d_n = dev.put(nrm)
        g = [100, 200, R.f32_bits(np.float32(float(s[158]) * (0.75 if cap == 16 else 100))), 300]
        rs = [7, 8] if with_rstat else None
        d_g, d_r = dev.counters(g), dev.counters(rs) if with_rstat else None
        dev.step("x8_guard_fix", src=dev.put(src), sstride=stride, glist=g9, gcount=dev.put(np.asarray([count], np.int32)), cap=cap,
                 normals=d_n, gstat=d_g, thr=float(fix_thr), scale=scale, rstat=d_r)
        n = min(cap, count)
        max_dn = R.x8_guard_fix(src[:n], listed_rows[:n], nrm, g, fix_thr, scale, rs)
        assert np.array_equal(bits(host(d_n)), bits(nrm)), "x8_guard_fix cap %d count %d: normals" % (cap, count)
        w = words(d_g)
        assert [w[0], w[1], w[3]] == [g[0], g[1], g[3]]
        old_max = float(R.bits_f32(g[2]))
        got_max = float(R.bits_f32(w[2]))
        if max_dn > old_max * (1 + 2 * R.DN_REL):
            print("x8_guard_fix max_dn", got_max, "predicted", max_dn)
            assert abs(got_max - max_dn) <= R.DN_REL * max_dn
        else:
            assert w[2] == g[2]
        if with_rstat:
            assert words(d_r)[:2] == rs
        if (cap, count) == (16, 9):
            assert max_dn > old_max and (not with_rstat or rs[1] > 8) and g[1] == 209


# ---- part B: the host sequence through the product ----------------------------------------------------------------------------
NB = 37


@pytest.fixture(scope="module")
def product(gpu_device):
    """The model at 37 golden patches, the filter's and the exact gate's logits of every row stepped launch by launch."""
    from conftest import golden_patch_files, load_golden_patches
    import layer_ref
    from nesti_net_amd import weights
    from nesti_net_amd.config import NestiConfig
    from nesti_net_amd.model import NestiNet
    cfg = NestiConfig()
    W = weights.synthetic_weights(cfg)
    pts, neff = [], []
    for p in golden_patch_files():
        g = load_golden_patches(p)
        if g["points"].shape[1] == 3 * 512 and g["n_eff"].shape[1] == 3:
            pts.append(g["points"])
            neff.append(g["n_eff"])
    pts, neff = np.concatenate(pts)[:NB], np.concatenate(neff)[:NB]
    pts, neff = torch.as_tensor(pts, device=gpu_device), torch.as_tensor(neff, device=gpu_device)
    E = cfg.n_experts

    def stepped(W, passes):
        net = NestiNet(cfg, W, dtype="f16x3c", device=gpu_device, max_batch=NB)
        mups = net.mups(pts, neff)
        out = []
        for fast in passes:
            t = layer_ref.TowerChecker(net.lib, net, W, "f16x3", -1, NB, mups, fast=fast)
            t.run(check=False)
            out.append(t.output()[:, :E].cpu().numpy().copy())
        return [net, mups] + out

    # On these 37 rows the synthetic gate's smallest margins (~0.1) lie far above 1.5 x the filter's error (~0.05): no threshold
    # would make a widening pass find a row.  Two biases of the gate's last layer are therefore moved so that two rows get the
    # filter margins 2^-9 and 2^-8 -- the runner-up of each is lifted, every other weight stays; what the passes then compute is
    # stepped again and the restatement predicts the calls from those logits alone
    filt0 = stepped(W, (1,))[2]
    order = np.argsort(-filt0, axis=1, kind="stable")
    m0 = filt0[np.arange(NB), order[:, 0]] - filt0[np.arange(NB), order[:, 1]]
    r0 = int(np.argmin(m0))
    ok = [r for r in np.argsort(m0) if r != r0 and order[r, 1] != order[r0, 1] and order[r, 1] != order[r0, 0]
          and order[r0, 1] != order[r, 0]]
    assert ok, "no second row whose runner-up can be lifted independently"
    r1 = int(ok[0])
    W2 = dict(W)
    bias = np.array(W["fc4noise/biases"], np.float32)
    bias[order[r0, 1]] += m0[r0] - np.float32(2.0 ** -9)
    bias[order[r1, 1]] += m0[r1] - np.float32(2.0 ** -8)
    W2["fc4noise/biases"] = bias
    return stepped(W2, (1, 0))


def _raw_stats(net, reset=False):
    from nesti_net_amd import _lib
    st = _lib.CCascadeStats()
    _lib.check(net.lib.nesti_model_cascade_stats(net._handle, ctypes.byref(st), int(reset), net._stream(None)), "nesti_model_cascade_stats")
    return st


def _check_call(net, mups, filt, exact, tau, cstat, rstat, what):
    """One nesti_gate_forward against the restatement continued from `cstat`"""
    probs, expert = net.gate(mups)
    st = _raw_stats(net)
    want_p, want_e, twice = R.gate_cascade(filt, exact, tau, WIDEN, 3, cstat, rstat)
    m = R.bits_f32(cstat[3])
    print(what, "tau %.6g" % tau, "rechecked", cstat[1], "widened", cstat[6], "events", cstat[7], "max_margin_err %.6g" % m,
          "sum %.9g (device %.9g)" % (cstat[4], st.sum_sq_pair_err))
    assert np.array_equal(host(expert), want_e), what + ": expert"
    perr = R.probs_error(host(probs), want_p)
    assert perr <= R.PROB_REL, what + ": probabilities (%.3g)" % perr
    got = [st.queries, st.rechecked, st.changed, R.f32_bits(st.max_margin_err), st.pairs, st.widened, st.widen_events]
    assert got == [cstat[i] for i in (0, 1, 2, 3, 5, 6, 7)], what + ": queries, rechecked, changed, max_margin_err bits, pairs, widened, widen_events"
    assert abs(st.sum_sq_pair_err - cstat[4]) <= R.SUM_REL * cstat[4], what + ": sum_sq_pair_err"
    assert R.f32_bits(st.tau) == R.f32_bits(tau)
    tau_eff = np.float32(tau) if rstat is not None else max(np.float32(tau), np.float32(WIDEN) * m)
    assert R.f32_bits(st.tau_eff) == R.f32_bits(tau_eff), what + ": tau_eff"
    return twice


def _product_taus(filt, exact):
    margin, nonfinite = R.top2_margin(filt)
    assert not nonfinite.any()
    third = float(R.margin_midpoint(margin, 1 / 3))
    # a threshold below the error its own rows measure, so that widening passes run: the lowest midpoint of the sorted margins
    # for which the restatement predicts one (the rows below it must exist, or nothing is measured at all)
    m = np.unique(margin)
    for i in range(1, len(m)):
        small = float(np.float32((np.float64(m[i - 1]) + np.float64(m[i])) / 2))
        c = R.new_cstat()
        R.gate_cascade(filt, exact, small, WIDEN, 3, c)
        if m[i - 1] < small < m[i] and c[6] > 0:
            return margin, [0.0, 1e30, third, small], True
    return margin, [0.0, 1e30, third, float(R.margin_midpoint(margin, 0.1))], False


def test_product_gate_sequence(product):
    net, mups, filt, exact = product
    net.set_reproducible(False)
    margin, taus, widens = _product_taus(filt, exact)
    widened = False
    for tau in taus:
        net.set_gate_margin(tau)
        net.cascade_stats(reset=True)
        cstat = R.new_cstat()
        twice = _check_call(net, mups, filt, exact, tau, cstat, None, "first call")
        first = (cstat[1], cstat[6], cstat[7])
        widened |= cstat[6] > 0
        if tau == 0.0:
            assert cstat[1] == 0 and not twice.any()
        if tau == 1e30:
            assert cstat[1] == NB and cstat[5] == NB * (filt.shape[1] - 1)
        # a second call without reset starts from the raised threshold
        _check_call(net, mups, filt, exact, tau, cstat, None, "second call")
        assert cstat[0] == 2 * NB and cstat[1] - first[0] >= first[0]
        if first[1] and first[2] < 3:                # converged: the second call's first list already covers the band
            assert cstat[6] == first[1], "the second call widened again"
    assert widens and widened, "no threshold between two filter margins makes a widening pass run on these 37 rows"
    assert 8 <= int((margin < np.float32(taus[2])).sum()) <= 16


def test_product_gate_sequence_reproducible(product):
    net, mups, filt, exact = product
    margin, taus, widens = _product_taus(filt, exact)
    net.set_reproducible(True)
    try:
        for tau in taus:
            net.set_gate_margin(tau)
            net.reproducible_stats(reset=True)
            cstat, rstat = R.new_cstat(), [0] * 8
            for call in ("first call", "second call"):
                twice = _check_call(net, mups, filt, exact, tau, cstat, rstat, "reproducible, " + call)
                assert np.array_equal(twice, margin < np.float32(tau))
                rs = net.reproducible_stats()
                assert rs["gate_violations"] == rstat[0] and rs["on"] and cstat[6] == 0 and cstat[7] == 0
                assert R.f32_bits(rs["max_margin_err"]) == cstat[3]
            if tau == taus[3] and widens:
                assert rstat[0] > 0, "the threshold below the smallest error counted no violation"
    finally:
        net.set_reproducible(False)
        net.cascade_stats(reset=True)
