"""Host-only checks of tests/decision_ref.py, the numpy restatement the GPU tests of the deciding kernels compare against
(tests/test_gpu_decisions.py): it agrees with a brute-force fp64 evaluation, row by row in plain Python, on the crafted rows -- whose
entries lie on a grid where the fp32 operations are exact, the three off-grid threshold rows apart --, and the refusals of
nesti_debug_decision_step, all of which return before any device call."""
import ctypes
import math

import numpy as np
import pytest

import decision_ref as R

B = 300
ES = (1, 2, 7, 8)


def _brute_row(l):
    """(nonfinite, margin) of one row in Python floats"""
    l = [float(v) for v in l]
    if not all(math.isfinite(v) for v in l):
        return True, None
    s = sorted(l, reverse=True)
    return False, (s[0] - s[1]) if len(s) > 1 else math.inf


def _brute_expert(l):
    l = [float(v) for v in l]
    if any(math.isnan(v) or v == math.inf for v in l) or all(v == -math.inf for v in l):
        return 0
    return l.index(max(l))


@pytest.mark.parametrize("E", ES)
def test_margins_flags_and_arg_max_agree_with_brute_force(E):
    full, fixed = R.crafted_logits(B, E, seed=E)
    l = full[:, :E]
    margin, nonfinite = R.top2_margin(l)
    taus = [0.0, float(R.TAU_X), 1e30] + ([float(R.margin_midpoint(margin[~nonfinite], 1 / 3))] if E > 1 else [])
    for tau in taus:
        for err in (0.0, 0.5):
            cstat, fc = R.new_cstat(err), np.zeros(128, np.int32)
            r = R.gate_flag(l, tau, 1.5, cstat, fc, 16, 19)
            tau_eff = max(tau, 1.5 * err)
            assert float(r["tau_eff"]) == float(np.float32(tau_eff))
            want = set()
            for b in range(B):
                bad, m = _brute_row(l[b])
                if not bad:
                    assert float(margin[b]) == pytest.approx(m, rel=2.0 ** -23, abs=0) or (m == math.inf and margin[b] == np.inf)
                assert bad == bool(nonfinite[b])
                if bad or not (float(margin[b]) >= float(np.float32(tau_eff))):
                    want.add(b)
                assert int(r["expert"][b]) == _brute_expert(l[b])
            assert r["flags"] == want
            assert fc[0] == len(want) and cstat[0] == B and cstat[1] == len(want)
            rc = fc[R.FC_ROUND_COUNTS:R.FC_ROUND_COUNTS + 19]
            assert rc.sum() == len(want) and all(0 <= c <= 16 for c in rc) and list(rc) == sorted(rc, reverse=True)
    # what the fixed rows are there for
    for name in ("one_nan", "all_nan", "one_pinf", "one_ninf", "two_pinf", "pinf_and_nan", "ninf_close"):
        if name in fixed:
            assert nonfinite[fixed[name]]
    if E >= 2:
        assert margin[fixed["margin_eq_tau"]] == R.TAU_X
        assert margin[fixed["margin_below_tau"]] == np.nextafter(R.TAU_X, np.float32(0))
        assert margin[fixed["margin_above_tau"]] == np.nextafter(R.TAU_X, np.float32(1))
        r = R.gate_flag(l, R.TAU_X, 1.5, R.new_cstat(), np.zeros(128, np.int32), 16, 19)
        assert fixed["margin_below_tau"] in r["flags"] and not {fixed["margin_eq_tau"], fixed["margin_above_tau"]} & r["flags"]
        assert margin[fixed["all_equal"]] == 0 and r["expert"][fixed["all_equal"]] == 0
    if E >= 7:
        assert margin[fixed["tie_0_3"]] == 0 and r["expert"][fixed["tie_0_3"]] == 0
        assert margin[fixed["tie_5_6"]] == 0 and r["expert"][fixed["tie_5_6"]] == 5


@pytest.mark.parametrize("E", ES)
def test_softmax_agrees_with_brute_force(E):
    full, fixed = R.crafted_logits(B, E, seed=E)
    p = R.softmax64(full[:, :E])
    for b in range(B):
        l = [float(v) for v in full[b, :E]]
        if any(math.isnan(v) or v == math.inf for v in l) or all(v == -math.inf for v in l):
            assert np.isnan(p[b]).all()
            continue
        mx = max(l)
        ex = [math.exp(v - mx) for v in l]
        assert p[b] == pytest.approx(np.asarray(ex) / math.fsum(ex), rel=1e-14, abs=0)
    if E > 1:
        assert p[fixed["pm80"], E - 1] < 1e-60 and p[fixed["pm80"], 0] == pytest.approx(1.0)
    assert R.probs_error(p, p) == 0 and R.probs_error(np.where(np.isnan(p), 0, p), p) == float("inf")


@pytest.mark.parametrize("E", ES)
def test_recheck_and_widen_agree_with_brute_force(E):
    full, fixed = R.crafted_logits(B, E, seed=E)
    l = full[:, :E]
    exact, extra = R.crafted_exact(full, E, fixed, seed=E)
    keep = np.zeros((B, R.MAX_EXPERTS), np.float32)
    keep[:, :E] = l
    cstat, fc = R.new_cstat(), np.zeros(128, np.int32)
    tau = float(R.TAU_X)
    r = R.gate_flag(l, tau, 1.5, cstat, fc, 16, 19)
    expert = r["expert"].copy()
    R.gate_recheck(exact, r["flags"], keep, expert, cstat, fc, 1.5)
    # brute force over the flagged rows
    mx, sq, pairs, changed = 0.0, 0.0, 0, 0
    for b in sorted(r["flags"]):
        a = int(r["expert"][b])
        for e in range(E):
            pe = abs((float(l[b, a]) - float(l[b, e])) - (float(exact[b, a]) - float(exact[b, e])))
            if math.isfinite(pe):
                mx, sq, pairs = max(mx, pe), sq + pe * pe, pairs + (e != a)
        changed += _brute_expert(exact[b]) != a
        assert int(expert[b]) == _brute_expert(exact[b])
    assert float(R.bits_f32(cstat[3])) == pytest.approx(mx, rel=2.0 ** -22, abs=0)
    assert cstat[4] == pytest.approx(sq, rel=2.0 ** -21, abs=0) and math.isfinite(cstat[4])
    assert cstat[5] == pairs and cstat[2] == changed
    if E > 1:
        assert 0 < pairs < (E - 1) * len(r["flags"]), "the non-finite rows must cost some pairs and not all"
    # one widening pass: the band [tau_eff, 1.5 x max error) among the rows with finite logits
    cstat[3] = R.f32_bits(0.5)
    before = cstat[1]
    rows = R.gate_widen(keep, E, 1.5, cstat, fc, 16, 19)
    want = set()
    for b in range(B):
        bad, m = _brute_row(l[b])
        if not bad and tau <= float(np.float32(m)) < 0.75:
            want.add(b)
    assert rows == want and not rows & r["flags"] and cstat[1] == before + len(rows) and cstat[6] == len(rows)
    assert float(fc.view(np.float32)[R.FC_TAU_EFF]) == 0.75 and cstat[7] == (1 if rows else 0)
    if E > 1:
        assert fixed["margin_eq_tau"] in rows
    # a second pass finds the band empty: upper <= lower
    assert R.gate_widen(keep, E, 1.5, cstat, fc, 16, 19) == set() and fc[R.FC_WIDEN_COUNT] == 0
    assert float(fc.view(np.float32)[R.FC_TAU_EFF]) == 0.75


def test_cascade_sequence_on_crafted_rows():
    """gate_cascade = flag, recheck, up to three widening passes each followed by its recheck; in reproducible form one pass and
    counted violations."""
    E = 7
    full, fixed = R.crafted_logits(B, E, seed=3)
    exact, _ = R.crafted_exact(full, E, fixed, seed=3)
    cstat = R.new_cstat()
    probs, expert, twice = R.gate_cascade(full[:, :E], exact, 2.0 ** -8, 1.5, 3, cstat)
    m = float(R.bits_f32(cstat[3]))
    assert cstat[0] == B and cstat[1] == int(twice.sum()) and cstat[6] > 0 and 1 <= cstat[7] <= 3 and m > 2.0 ** -8 / 1.5
    margin, nonfinite = R.top2_margin(full[:, :E])
    if cstat[7] < 3:
        assert (twice == (nonfinite | (margin < np.float32(1.5) * np.float32(m)))).all()
    assert np.array_equal(expert[twice], R.arg_max(exact)[twice]) and np.array_equal(expert[~twice], R.arg_max(full[:, :E])[~twice])
    rstat, c2 = [0] * 8, R.new_cstat()
    _, _, twice2 = R.gate_cascade(full[:, :E], exact, 2.0 ** -8, 1.5, 3, c2, rstat)
    assert c2[6] == 0 and c2[7] == 0 and (twice2 == (nonfinite | (margin < np.float32(2.0 ** -8)))).all() and rstat[0] > 0


def test_round_counts_max_words_switch_and_guard():
    assert list(R.round_counts([0, 5, 16, 17, 300], 16, 3)) == [0, 0, 0, 5, 0, 0, 16, 0, 0, 16, 1, 0, 16, 16, 16]
    den = np.float32(1e-40)
    vals = np.asarray([np.nan, np.inf, -1.0, 0.0, den, 0.5, 3.25, 1e-3], np.float32)
    assert R.stat_max_import(0, vals) == R.f32_bits(3.25) and R.stat_max_import(0, vals[:5]) == R.f32_bits(den) > 0
    assert R.stat_max_import(R.f32_bits(7.0), vals) == R.f32_bits(7.0)
    assert list(R.switch_finish([0.014, 0.015, np.nan, 0.016, -1.0], 0.015)) == [0, 1, 1, 1, 0]
    n, nan_row, zero_row = R.crafted_normals(B, 5)
    r = R.norms64(n)
    s = np.sort(r[np.isfinite(r) & (r > 0)])
    assert (s[1:] / s[:-1] > 1 + 2.0 ** -10).all() and np.isnan(r[nan_row]) and r[zero_row] == 0
    gstat, slot = [0, 0, R.f32_bits(1e-4), 0], np.zeros(2, np.float32)
    R.x8_guard_begin(0, 1e-3, 4.0, B, gstat, slot)
    assert slot[0] == 0 and slot[1] == np.float32(1e-3) and gstat[0] == B
    gstat[2] = R.f32_bits(1e-3)
    R.x8_guard_begin(1, 1e-3, 4.0, B, gstat, slot)
    assert slot[0] == np.float32(1e-3) and slot[1] == np.float32(4.0) * np.float32(1e-3)
    band, listed = R.x8_guard_flag(range(B), n, slot, 4, gstat)
    want = {i for i in range(B) if math.isnan(r[i]) or float(slot[0]) <= r[i] < float(slot[1])}
    assert band == want and listed == 4 and gstat[3] == len(want) - 4 and nan_row in band and zero_row not in band


def _lib():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    return _lib, _lib.load()


def _refused(L, lib, op, a, text):
    assert lib.nesti_debug_decision_step(op, ctypes.byref(a) if a is not None else None, None) != 0
    msg = lib.nesti_last_error().decode()
    assert msg.startswith("nesti_debug_decision_step: ") and text in msg, msg


def test_decision_step_refusals():
    """Every refusal returns before any device call: no GPU is needed (the pointers are never followed)."""
    L, lib = _lib()
    ops = {n: i for i, n in enumerate(L.DECISION_OPS)}
    assert len(ops) == 13
    fake = ctypes.c_void_p(0x1000)
    ptrs = [n for n, t in L.CDebugDecision._fields_ if t is ctypes.c_void_p]

    def full(**kw):
        a = L.CDebugDecision()
        for n in ptrs:
            setattr(a, n, fake)
        a.B, a.E, a.n_lists, a.cap, a.n_rounds, a.lstride, a.sstride = 300, 7, 1, 16, 19, 64, 4
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    _refused(L, lib, 0, None, "null argument")
    _refused(L, lib, -1, full(), "unknown op")
    _refused(L, lib, len(ops), full(), "unknown op")
    for name in ("gate_finish", "gate_flag", "gate_widen", "gate_recheck", "route"):
        _refused(L, lib, ops[name], full(E=0), "E outside")
        _refused(L, lib, ops[name], full(E=R.MAX_EXPERTS + 1), "E outside")
    for name in ("gate_flag", "gate_widen", "round_counts"):
        _refused(L, lib, ops[name], full(n_rounds=R.MAX_ROUNDS + 1), "n_rounds")
    # 11 lists x 24 rounds: the launcher's own refusal (one 256-thread block), also before any device call
    assert lib.nesti_debug_decision_step(ops["round_counts"], ctypes.byref(full(n_lists=11, n_rounds=24)), None) != 0
    assert lib.nesti_last_error().decode() == "round_counts: too many lists x rounds"
    needed = {"gate_finish": ["logits"], "gate_flag": ["logits", "expert", "keep", "fcounts", "flag_list", "cstat"],
              "gate_widen": ["keep", "fcounts", "flag_list", "cstat"],
              "gate_recheck": ["logits", "flag_list", "count_ptr", "keep", "expert", "cstat", "fcounts"],
              "round_counts": ["counts", "round_out"], "switch_finish": ["logits"], "x8_guard_begin": ["gstat", "slot"],
              "x8_guard_flag": ["lists", "count_ptr", "normals", "slot", "glist", "gcount", "gstat"],
              "x8_guard_fix": ["src", "glist", "gcount", "normals", "gstat"], "route": ["expert", "counts", "lists"],
              "scatter3": ["src", "normals"], "stat_max_export": ["word", "dst"], "stat_max_import": ["word", "src"]}
    assert sorted(needed) == sorted(ops)
    for name, fields in needed.items():
        for f in fields:
            _refused(L, lib, ops[name], full(**{f: None}), "null pointer")
    for name in ("gate_finish", "switch_finish"):       # routing lists: counts without lists
        _refused(L, lib, ops[name], full(lists=None), "null pointer")
