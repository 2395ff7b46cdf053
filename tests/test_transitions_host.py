"""CPU side of the transition cases (tests/transition_cases.py), on the compiled reference (or, where oracle/_ref is absent,
the restatement that tests/test_oracle_pin.py pins to it): every role reaches the branch of BiquadInterpFilter::setParams /
dualProcess, DoFilters, Mix and DoHrtfMix it was written for; the numpy restatement of the filter pair's state machine and
of its lerpf chain is the reference's, counter for counter and bit for bit; every transition moves the reference's output
by more than 100x the tolerance the GPU tests hold the kernels to; COEFF_TOLERANCE is eight times the chain's own rounding
noise.

The counter of a pair counts steps in its high bits and the samples done of the running step in its low five
(biquad.cpp:299-303): it does not count samples down.  A ramp started at 256 reads 229 after 37 samples (7 steps left, 5
samples into the next), 192 after 27 more and 193 after one more -- not 202 and 201; the `short` schedule's first change
comes in front of its 27-sample update (a fresh filter snaps, so nothing can ramp in the 37-sample update before it), and
the ramp reads 283 after it, 284 after the single sample, 91 after the next 191 and 0 from then on.  dualProcess runs a pair
on the larger counter and writes it to both filters, so after an update a pair's counters are always equal, and a retarget
of one filter in mid-ramp (256 against the other's 283) is seen in the counters only between the install and the next
update -- the `early` runs read the state there."""
from functools import lru_cache

import numpy as np
import pytest

import oracle_lib as ol
import transition_cases as tc
from test_tolerance_model import multi_voice_tolerance

LP, HP, SLP, SHP = 7, 8, 9, 10            # direct_lp.counter, direct_hp.counter, send_lp[0].counter, send_hp[0].counter in the integer state
COEFFS, TARGETS = slice(2, 7), slice(7, 12)     # of Biquad.as_tuple()


def _oracle():
    L = ol.load("ref" if ol.available("ref") else "port")
    L.L.oal_set_simd(1)
    return L


@lru_cache(maxsize=None)
def _ref(schedule, form, mhr, roles=None, mixed=True, hold=(), early=False):
    return tc.run(_oracle(), schedule, form, mhr=mhr, roles=roles, mixed=mixed, hold=dict(hold), early=early)


def _state(run, name):
    """role `name`'s integer state per update"""
    _, ints, extra = run
    return [ints[k][extra["watched"].index(extra["roles"][name])] for k in range(len(ints))]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def test_counter_arithmetic_hand_computed():
    # 256 = 8 steps of 32; 37 samples: one whole step and 5 samples of the next -> 7 * 32 | 5
    assert tc.counter_after(256, 37) == 229
    assert tc.counter_after(229, 27) == 192            # the step's other 27 samples: 6 steps left, none begun
    assert tc.counter_after(192, 1) == 193
    assert tc.counter_after(256, 27) == 283            # inside the first step: 8 * 32 | 27
    assert tc.counter_after(283, 1) == 284
    assert tc.counter_after(284, 191) == 91            # 4 + 5 * 32 + 27: 2 * 32 | 27
    assert tc.counter_after(91, 64) == 0
    assert tc.counter_after(256, 24) == 280
    assert tc.counter_after(256, 255) == 63 and tc.counter_after(256, 256) == 0 and tc.counter_after(256, 1024) == 0
    assert tc.counter_after(0, 100) == 0 and tc.counter_after(-1, 100) == -1


def test_coefficient_margins():
    changes = tc.gain_changes()
    sub = [c for c in changes if (c[0], c[1]) in tc.SUB_THRESHOLD_CHANGES]
    assert {c[0] for c in sub} == {"sub_threshold_settled", "sub_threshold_in_flight"}
    for c in changes:
        if c in sub:
            assert 0.0 < c[6] <= 1.0 / 128.0, c
        else:
            assert c[6] >= 1.0 / 32.0, c
    # every role that is to ramp has a large change; both filters of the extra role change in the same update
    large = {(c[0], c[1], c[2], c[3]) for c in changes if c not in sub}
    assert {("both_filters", 1, "direct", True), ("both_filters", 1, "send", True), ("both_filters", 2, "send", False)} <= large
    assert ("hp_only", 1, "direct", False) in large and not any(c[0] == "hp_only" and c[3] for c in changes)
    assert ("staggered", 1, "direct", True) in large and ("staggered", 2, "direct", False) in large


def test_gain_steps_sit_on_their_branches():
    """the `gains` role's dry targets: exactly 0, at or below the silence threshold, back up, and one change whose ramp step
    (target - current) / 64 is no larger than epsilon although the target differs (Mix, mixer_c.cpp:154-178)"""
    assert tc.GAIN_STEPS[1] == 0.0 and tc.GAIN_STEPS[3] == 1.0
    for sends, hrtf in ((0, False), (2, False)):
        g = [np.array(tc.voice_params(1, "gains", k, hrtf, sends, None).dry_gains[:5], np.float32) for k in range(tc.MAX_UPDATES)]
        assert np.all(g[1] == 0.0) and np.all(g[2] > 0.0) and np.all(g[2] <= tc.SILENCE) and np.all(g[3] > 0.1)
        k = tc.TINY_GAIN_UPDATE
        step = (g[k] - g[k - 1]) * np.float32(1.0 / 64.0)
        assert np.all(g[k] != g[k - 1]) and np.all(np.abs(step) <= tc.EPSILON), step
        for schedule in tc.SCHEDULES.values():
            assert len(schedule) <= k or schedule[k] >= 64          # (the ramp of that update is 64 samples long)


@pytest.mark.parametrize("form", ["dry_sends", "hrtf_sends"])
@pytest.mark.parametrize("schedule", list(tc.SCHEDULES))
def test_the_restatement_is_the_reference(schedule, form, synth_mhr):
    """PairModel (float32) against the reference's filters after every update: counters, targets and current coefficients of
    the direct pair and of send 0's pair, bit for bit"""
    run = _ref(schedule, form, synth_mhr if form.startswith("hrtf") else None)
    for name in tc.role_names(form):
        ints = _state(run, name)
        for which, (lp, hp, clp, chp) in enumerate((("direct_lp", "direct_hp", LP, HP), ("send_lp", "send_hp", SLP, SHP))):
            model = tc.model_run(name, schedule, which)[1]
            for k, m in enumerate(model):
                if m is None:
                    assert ints[k] is None
                    continue
                f = run[2]["floats"][k][name]
                assert (ints[k][clp], ints[k][chp]) == m[0], (name, which, k, ints[k], m[0])
                for j, key in enumerate((lp, hp)):
                    assert _bits(f[key][COEFFS]) == _bits(m[1][j]), (name, key, k, f[key][COEFFS], m[1][j])
                    assert _bits(f[key][TARGETS]) == _bits(m[2][j]), (name, key, k)


@pytest.mark.parametrize("form", ["dry_sends", "hrtf"])
def test_every_role_reaches_its_branch(form, synth_mhr):
    mhr = synth_mhr if form == "hrtf" else None
    runs = {s: _ref(s, form, mhr) for s in tc.SCHEDULES}
    short = runs["short"]

    # a ramp carried across updates shorter than a step, ended inside an update
    lp = [s[LP] for s in _state(short, "ramp")]
    assert lp == [0, 283, 284, 91, 0, 0, 0, 0], lp
    for schedule, run in runs.items():
        lp = [s[LP] for s in _state(run, "ramp")]
        done = np.cumsum((0,) + tc.SCHEDULES[schedule][1:])         # samples since the ramp began, after every update
        assert all((c == 0) == (k == 0 or done[k] >= 256) for k, c in enumerate(lp)), (schedule, lp)
        assert all(s[LP] == 0 and s[HP] == 0 for s in _state(run, "sub_threshold_settled")), schedule
        for name in tc.role_names(form):
            for s in _state(run, name):
                assert s is None or (s[LP] == s[HP] and (len(s) <= SLP or s[SLP] == s[SHP])), (schedule, name, s)
        st = _state(run, "late_on")
        assert [s[LP] for s in st[:2]] == [0, 0] and st[2][LP] == tc.counter_after(256, tc.SCHEDULES[schedule][2]), (schedule, st)
        st = _state(run, "fresh_voice")
        assert st[0] is None and st[1] is None and all(s[LP] == 0 and s[4] == 1 for s in st[2:]), (schedule, st)
        st = _state(run, "off_in_flight")
        f = run[2]["floats"][2]["off_in_flight"]
        assert st[1][LP] == tc.counter_after(256, tc.SCHEDULES[schedule][1]) and st[2][LP] == 0 and st[2][HP] == 0, (schedule, st)
        for key in ("direct_lp", "direct_hp"):
            assert f[key][0] == 0.0 and f[key][1] == 0.0 and f[key][COEFFS] == f[key][TARGETS], (schedule, key, f[key])
        assert st[3][LP] == tc.counter_after(256, tc.SCHEDULES[schedule][3]), (schedule, st)
        st = _state(run, "stop_in_flight")
        assert [s[0] for s in st[:3]] == [ol.VOICE_PLAYING, ol.VOICE_PLAYING, ol.VOICE_STOPPED], (schedule, st)
        assert st[2][1:3] == st[1][1:3], "a stopping voice's position stays"
        if form == "hrtf":
            d = [s[5:7] for s in _state(run, "hrir")]
            assert all(a[0] != b[0] and a[1] != b[1] for a, b in zip(d, d[1:])), (schedule, d)
            g = [run[2]["floats"][k]["hrir"]["hrtf_old_gain"] for k in range(len(d))]
            assert all(a != b for a, b in zip(g, g[1:])), g
        # the gain ramp is min(samplesToMix, 64) samples long (voice.cpp:1093) and the update mixes samplesToMix samples: however
        # short the update, the current gain arrives at its target in it (DoHrtfMix's two interpolations for a fade that
        # outlasts the mix, voice.cpp:857-861 and :884-889, are not reached from Voice::mix)
        for k in range(len(tc.SCHEDULES[schedule])):
            for name in ("gains", "hrir") if form == "hrtf" else ("gains",):
                p = tc.voice_params(run[2]["roles"][name], name, k, form == "hrtf", tc.FORM_SENDS[form], tc.directions(mhr) if mhr else None)
                f = run[2]["floats"][k][name]
                if form == "hrtf":
                    assert f["hrtf_old_gain"] == p.hrtf_gain, (schedule, name, k, f["hrtf_old_gain"], p.hrtf_gain)
                else:
                    assert f["dry_current"] == tuple(p.dry_gains[:5]), (schedule, name, k, f["dry_current"])
    # the pair runs on the larger counter: the retargeted low-pass (256) goes on at the high-pass's 283
    assert [s[LP] for s in _state(short, "retarget_in_flight")][:4] == [0, 283, 284, 91]
    assert [s[LP] for s in _state(short, "sub_threshold_in_flight")][:4] == [0, 283, 284, 91]
    assert [s[HP] for s in _state(short, "hp_only")][:4] == [0, 283, 284, 91]
    assert [s[LP] for s in _state(short, "off_in_flight")][:6] == [0, 283, 0, 127, 63, 0]
    assert [s[LP] for s in _state(short, "late_on")][:5] == [0, 0, 257, 64, 0]

    # between the install and the next update (the early runs: params(k + 1) are in when update k is read)
    early = _ref("short", form, mhr, early=True)
    assert [s[LP:HP + 1] for s in _state(early, "ramp")][:3] == [(256, 0), (283, 283), (284, 284)]
    # in mid-ramp a large change restarts the filter's counter, a sub-threshold one replaces the targets and lets it run
    assert _state(early, "retarget_in_flight")[1][LP:HP + 1] == (256, 283)
    assert _state(early, "sub_threshold_in_flight")[1][LP:HP + 1] == (283, 283)
    f = early[2]["floats"][1]["sub_threshold_in_flight"]["direct_lp"]
    assert _bits(f[TARGETS]) == _bits(tc.design(True, 0.104)) and f[COEFFS] != f[TARGETS]
    assert _state(early, "staggered")[1][LP:HP + 1] == (283, 256)           # staggered counters of one pair
    assert _state(early, "hp_only")[0][LP:HP + 1] == (0, 256)
    # settled: a sub-threshold change snaps
    f = early[2]["floats"][0]["sub_threshold_settled"]["direct_lp"]
    assert _state(early, "sub_threshold_settled")[0][LP] == 0 and _bits(f[COEFFS]) == _bits(tc.design(True, 0.495))
    assert _state(early, "late_on")[1][LP:HP + 1] == (256, 0) and _state(early, "off_in_flight")[2][LP:HP + 1] == (256, 256)
    assert _state(early, "stop_in_flight")[1][0] == ol.VOICE_STOPPING
    even = _ref("even", form, mhr, early=True)
    assert _state(even, "sub_threshold_in_flight")[1][LP] == 0              # (on 1024-sample updates the ramp is over: a snap)


# the roles whose transition is one change, against the role held in front of it: {role: update the parameters stay at}
HELD = [(name, 0) for name in tc.ROLES] + [("sub_threshold_in_flight", 1), ("retarget_in_flight", 1), ("staggered", 1),
                                           ("off_in_flight", 2), ("both_filters", 1)]


@pytest.mark.parametrize("schedule", list(tc.SCHEDULES))
@pytest.mark.parametrize("form", ["hrtf", "hrtf_sends", "dry", "dry_sends"])
def test_every_transition_is_audible(form, schedule, synth_mhr):
    """Each role alone on a scene, against the same voice with its parameters held (at params(0), and for the roles with a
    second change at the parameters in front of that): from the first update whose parameters differ on, the reference's
    buses differ by more than 100x the tolerance of one voice -- a kernel that missed the transition cannot pass."""
    mhr = synth_mhr if form.startswith("hrtf") else None
    for name, j in HELD:
        if name not in tc.role_names(form) or ((name, j) == ("both_filters", 1) and not tc.FORM_SENDS[form]):
            continue                    # (the extra role's second change is the send filter's alone)
        want = _ref(schedule, form, mhr, roles=(name,), mixed=False)[0]
        held = _ref(schedule, form, mhr, roles=(name,), mixed=False, hold=((name, j),))[0]
        first = max(j + 1, tc.START.get(name, 0))
        a = np.concatenate(want[first:]).astype(np.float64)
        b = np.concatenate(held[first:]).astype(np.float64)
        bound = multi_voice_tolerance(1, 64 if mhr else 1, float(np.abs(a).max()))
        diff = float(np.abs(a - b).max())
        print(f"{form} {schedule} {name} against params({j}): differs by {diff:.3e}, 100 x bound {100 * bound:.3e}")
        assert diff > 100 * bound, (form, schedule, name, j, diff, bound)
        if first > 0 and name not in tc.START:
            assert all(np.array_equal(x, y) for x, y in zip(want[:first], held[:first])), (form, schedule, name)


def test_coefficient_tolerance_is_eight_times_the_chain_noise():
    noise = tc.measure_coeff_noise()
    print(f"COEFF_NOISE measured {noise:.3e}; module {tc.COEFF_NOISE:.1e}, COEFF_TOLERANCE {tc.COEFF_TOLERANCE:.1e}")
    assert f"{noise:.1e}" == f"{tc.COEFF_NOISE:.1e}", noise
    assert f"COEFF_NOISE = {tc.COEFF_NOISE:.1e}" in tc.__doc__
    assert 8 * noise <= tc.COEFF_TOLERANCE <= 10 * noise, (noise, tc.COEFF_TOLERANCE)
