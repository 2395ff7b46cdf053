"""Playing voices whose parameters change: filter retargets (BiquadInterpFilter::setParams, core/filters/biquad.cpp:131-149),
ramps carried from update to update (dualProcess, :284-343), pairs cleared and restarted (DoFilters, core/voice.cpp:255-267),
gain ramps over min(samplesToMix, 64) samples (voice.cpp:1093; Mix, core/mixer/mixer_c.cpp:150-186), HRIR and gain
transitions (DoHrtfMix, voice.cpp:827-902), a stop in the middle of all of it -- the state every voice kernel restates
(csrc/dev_mix.hpp BiquadSetTarget / BiquadDualInterp, voice_wave.hip InstallPair, wave_common.hpp WaveDoFilters, ...).

One scene plays every role of ROLES at once, driven through any object with the oracle_lib.Scene interface.  A role is a
function params(k) of the update index; params(k) is delivered before update k (`early`: right behind update k - 1, in
front of the read-back of its results, so that a context that defers its update has the update's own voice kernel install
the block).  Role voices play at gain 0.5, every fourth voice is a filler at 1e-3 on another resampler key, as in
tests/loop_edge_cases.py.

Coefficient margins, asserted at import time with the numpy shelf design of tests/source_param_cases.py: every change of a
filter's gain either moves at least one coefficient by at least LARGE = 1/32 (check_set's 1/64 says "different" whatever
the rounding) or every coefficient by at most SUB = 1/128 (it says "the same").

COEFF_NOISE: the largest disagreement between the float32 and the float64 evaluation of the reference's lerpf chain
(biquad.cpp:235-240, :321-331; PairModel below restates it, tests/test_transitions_host.py pins the float32 evaluation to
the compiled reference bit for bit) over all roles, schedules, filters and steps, relative to max(|x|, 1):

    COEFF_NOISE = 1.2e-07        COEFF_TOLERANCE = 8 x = 1.0e-06

(8 x for the reason tests/source_param_cases.py gives for its TOLERANCE: it covers a device that contracts the two
operations of a lerpf into one and the like.)  test_transitions_host.py prints the figure and asserts
8 * noise <= COEFF_TOLERANCE <= 10 * noise."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import loop_edge_cases as lc
import oracle_lib as ol
from source_param_cases import _design_shelf

F32 = np.float32
SCHEDULES = {
    "even": (1024, 1024, 1024, 1024, 1024),
    "short": (37, 27, 1, 191, 64, 5, 300, 1024),    # ramps end inside 32-sample steps; updates below 64, below 32, of one sample
    "ragged": (1000, 24, 1024, 700),
}
FORM_SENDS = {"hrtf": 0, "hrtf_sends": 1, "dry": 0, "dry_sends": 2}
HF_NORM, LF_NORM = 5000.0 / 48000.0, 250.0 / 48000.0
STEP, RESAMPLER = 60211, ol.RS_SPLINE
ROLE_GAIN, FILLER_GAIN = 0.5, 1e-3
LARGE, SUB = 1.0 / 32.0, 1.0 / 128.0
COEFF_NOISE = 1.2e-07
COEFF_TOLERANCE = 1.0e-06
GAIN_RTOL, GAIN_FLOOR = 2e-6, 1e-6      # 16 float32 ulps of a two-operation lerpf: derived, not measured
SILENCE = 1e-5                          # GainSilenceThreshold (core/mixer/defs.h)
EPSILON = float(np.finfo(np.float32).eps)

BUFS = (lc.BufSpec(6000, 100, 5900, ol.FMT_FLOAT, 1), lc.BufSpec(5000, 0, 5000, ol.FMT_SHORT, 1))

# what a role asks for before update k.  flt / sflt: (active, gain_hf, gain_lf) of the direct filter / of send 0's filter;
# gain: a factor on the voice's gains (direct and sends); dir: index into directions() (None: the voice's own fixed
# direction); stop: set to Stopping before this update
P = namedtuple("P", "flt sflt gain dir stop")
BASE_FILTER = (1, 0.5, 1.0)


def _p(flt=BASE_FILTER, sflt=None, gain=1.0, dir=None, stop=False):
    return P(flt, flt if sflt is None else sflt, gain, dir, stop)


def _at(k, *vals):
    return vals[min(k, len(vals) - 1)]


GAIN_STEPS = (1.0, 0.0, 1e-5, 1.0, 1.0 + 4e-6, 0.6, 1.0, 0.35)      # exactly 0; below the silence threshold; back up; |step| <= epsilon
TINY_GAIN_UPDATE = 4
ROLES = {
    "ramp": lambda k: _p(flt=(1, _at(k, 0.5, 0.1), 1.0)),
    "retarget_in_flight": lambda k: _p(flt=(1, _at(k, 0.5, 0.1, 0.8), 1.0)),
    "sub_threshold_settled": lambda k: _p(flt=(1, _at(k, 0.5, 0.495), 1.0)),
    "sub_threshold_in_flight": lambda k: _p(flt=(1, _at(k, 0.5, 0.1, 0.104), 1.0)),
    "hp_only": lambda k: _p(flt=(1, 0.5, _at(k, 1.0, 0.1))),
    "staggered": lambda k: _p(flt=(1, _at(k, 0.5, 0.1), _at(k, 1.0, 1.0, 0.1))),
    "off_in_flight": lambda k: _p(flt=(_at(k, 1, 1, 0, 1), _at(k, 0.5, 0.1, 0.1, 0.7), _at(k, 1.0, 1.0, 1.0, 0.2))),
    "late_on": lambda k: _p(flt=(_at(k, 0, 0, 1), _at(k, 1.0, 1.0, 0.2), 1.0)),
    # the direct and the send filter change in the same update, by different amounts, the send's low shelf one update later
    "both_filters": lambda k: _p(flt=(1, _at(k, 0.5, 0.1), 1.0), sflt=(1, _at(k, 0.6, 0.15), _at(k, 1.0, 1.0, 0.15))),
    "gains": lambda k: _p(gain=_at(k, *GAIN_STEPS)),
    "stop_in_flight": lambda k: _p(flt=(1, _at(k, 0.5, 0.1, 0.8), 1.0), gain=_at(k, 1.0, 0.7, 0.9), stop=k == 2),
    "hrir": lambda k: _p(dir=k, gain=_at(k, 1.0, 0.6, 0.9, 0.5, 1.0, 0.7, 0.4, 0.8)),
    "fresh_voice": lambda k: _p(flt=(1, 0.3, 1.0)),
}
HRTF_ONLY = ("hrir",)
START = {"fresh_voice": 2}                  # added and started before this update (the last voice of its scene)
STOP_UPDATE = 2
MAX_UPDATES = max(len(s) for s in SCHEDULES.values())
# the delivery-path tests' roles (no voice that is added while the scene runs)
DELIVERY_ROLES = ("ramp", "retarget_in_flight", "sub_threshold_in_flight", "staggered", "off_in_flight", "gains",
                  "stop_in_flight", "hrir")


def role_names(form, roles=None):
    names = [n for n in ROLES if form.startswith("hrtf") or n not in HRTF_ONLY]
    if roles is not None:
        assert set(roles) <= set(ROLES)
        names = [n for n in names if n in roles]
    return names


# ---- coefficient margins -----------------------------------------------------------------------------------------------
def design(high, gain, F=F32):
    return [F(x) for x in _design_shelf(high, F(F32(HF_NORM if high else LF_NORM)), F(F32(gain)), F)]


def coefficient_move(high, g0, g1):
    return max(abs(float(a) - float(b)) for a, b in zip(design(high, g0), design(high, g1)))


def gain_changes():
    """[(role, update, 'direct' | 'send', high, from, to, largest coefficient move)] of every filter gain that changes"""
    out = []
    for name, params in ROLES.items():
        for which in (0, 1):
            for high in (True, False):
                prev = None
                for k in range(MAX_UPDATES):
                    g = params(k)[which][1 if high else 2]
                    if prev is not None and g != prev:
                        out.append((name, k, ("direct", "send")[which], high, prev, g, coefficient_move(high, prev, g)))
                    prev = g
    return out


SUB_THRESHOLD_CHANGES = {("sub_threshold_settled", 1), ("sub_threshold_in_flight", 2)}
for _c in gain_changes():
    if (_c[0], _c[1]) in SUB_THRESHOLD_CHANGES:
        assert 0.0 < _c[6] <= SUB, _c
    else:
        assert _c[6] >= LARGE, _c
assert SUB_THRESHOLD_CHANGES <= {(_c[0], _c[1]) for _c in gain_changes()}


# ---- the reference's state machine, restated ---------------------------------------------------------------------------
def counter_after(counter, n):
    """mCounter of a pair that starts an update of n samples at `counter` (dualProcess, biquad.cpp:288-340): the high bits count
    the steps left, the low five the samples done of the running step"""
    if counter <= 0:
        return counter
    steps, steprem = counter // 32, 32 - (counter & 31)
    while steps > 0:
        td = min(steprem, n)
        steprem -= td
        if steprem:
            return (steps * 32) | (32 - steprem)
        n -= td
        steprem = 32
        steps -= 1
        if steps == 0:
            return 0
        if n == 0:
            return steps * 32
    return 0


class PairModel:
    """A low-pass / high-pass pair of BiquadInterpFilter as Voice::mix drives it: setParamsFromSlope of both (the targets are
    float32 designs whatever F is; check_set and the three-way state machine, biquad.cpp:38-43, :131-149), then DoFilters over
    n samples (the clear of an inactive pair; dualProcess's counter arithmetic and its lerpf chain, :288-340) with every
    operation on the coefficients of type F.  The samples themselves are not modelled.  trace: the current coefficients of
    both filters after every lerpf step."""

    def __init__(self, F=F32):
        self.F = F
        self.tgt = [[F32(1), F32(0), F32(0), F32(0), F32(0)] for _ in range(2)]       # Coefficients{}
        self.cur = [[F(x) for x in t] for t in self.tgt]
        self.counter = [-1, -1]
        self.trace = []

    def _snap(self, j):
        self.counter[j] = 0
        self.cur[j] = [self.F(x) for x in self.tgt[j]]

    def set_params(self, gain_hf, gain_lf):
        for j, (high, g) in enumerate(((True, gain_hf), (False, gain_lf))):
            new = design(high, g)
            diff = any(not (abs(n - t) <= F32(0.015625)) for n, t in zip(new, self.tgt[j]))
            self.tgt[j] = new
            if not diff:
                if self.counter[j] <= 0:
                    self._snap(j)
            elif self.counter[j] >= 0:
                self.counter[j] = 256
            else:
                self._snap(j)

    def process(self, n, active):
        F = self.F
        if not active:
            self._snap(0)
            self._snap(1)
            return
        top = max(self.counter)
        if top <= 0:
            return
        steps, steprem = top // 32, 32 - (top & 31)
        while steps > 0:
            td = min(steprem, n)
            steprem -= td
            if steprem:
                self.counter = [(steps * 32) | (32 - steprem)] * 2
                return
            n -= td
            steprem = 32
            steps -= 1
            if steps == 0:
                self._snap(0)
                self._snap(1)
                return
            a = F(1.0) / F(steps + 1)
            for j in range(2):
                self.cur[j] = [c + (F(t) - c) * a for c, t in zip(self.cur[j], self.tgt[j])]
            self.trace.append([list(self.cur[0]), list(self.cur[1])])
            if n == 0:
                self.counter = [steps * 32] * 2
                return


def model_run(name, schedule, which=0, F=F32):
    """the pair of role `name` (which: 0 direct, 1 send 0) over a schedule: (model, [(counters, current coefficients, targets)
    after every update]); None before the voice exists"""
    m, out = PairModel(F), []
    start = START.get(name, 0)
    for k, n in enumerate(SCHEDULES[schedule]):
        if k < start or (name == "stop_in_flight" and k > STOP_UPDATE):
            out.append(None if k < start else out[-1])
            continue
        active, ghf, glf = ROLES[name](k)[which]
        m.set_params(ghf, glf)
        m.process(n, active)
        out.append((tuple(m.counter), [list(c) for c in m.cur], [list(t) for t in m.tgt]))
    return m, out


def measure_coeff_noise():
    """the largest |float32 - float64| of the lerpf chain's coefficients, relative to max(|x|, 1), over every role, schedule,
    filter and step"""
    worst = 0.0
    for name in ROLES:
        for schedule in SCHEDULES:
            for which in (0, 1):
                a, b = model_run(name, schedule, which, F32)[0], model_run(name, schedule, which, np.float64)[0]
                assert len(a.trace) == len(b.trace)
                for ta, tb in zip(a.trace, b.trace):
                    for fa, fb in zip(ta, tb):
                        for x, y in zip(fa, fb):
                            worst = max(worst, abs(float(x) - float(y)) / max(abs(float(y)), 1.0))
    return worst


# ---- HRIR directions ---------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def directions(mhr):
    """MAX_UPDATES (elevation, azimuth) pairs, chosen on the CPU so that both ears' delays differ from one to the next"""
    L = ol.load("ref" if ol.available("ref") else "port")
    L.hrtf_load(mhr)
    cands = [(ev, az) for az in (0.4, -1.3, 2.6, -0.5, 1.5, -2.4, 0.9, -2.9, 2.0, -0.9, 0.1, 3.0) for ev in (0.1, -0.5, 0.6, -0.2)]
    picked, last = [], None
    for ev, az in cands:
        d = L.hrtf_get_coeffs(ev, az, 2.0, 0.0)[1]
        if last is None or (d[0] != last[0] and d[1] != last[1]):
            picked.append((ev, az))
            last = d
        if len(picked) == MAX_UPDATES:
            return tuple(picked)
    raise AssertionError("the data set's delays do not vary enough")


# ---- the runner --------------------------------------------------------------------------------------------------------
def _filter(f):
    return ol.default_filter(active=int(f[0]), gain_hf=f[1], gain_lf=f[2])


def voice_params(i, name, k, hrtf, sends, dirs):
    """slot i's parameters before update k (name None: a filler)"""
    r = np.random.default_rng(1000 + i)
    ev, az = r.uniform(-0.5, 0.5), r.uniform(-np.pi, np.pi)
    dry = r.uniform(0.3, 1.0, 5)
    sg = [r.uniform(0.1, 0.4, 4) for _ in range(sends)]
    if name is None:
        p, gain, step, rs = _p(flt=(0, 1.0, 1.0)), FILLER_GAIN, lc.FILLER_STEP, lc.FILLER_RESAMPLER
    else:
        p, step, rs = ROLES[name](k), STEP, RESAMPLER
        gain = ROLE_GAIN * p.gain
        if p.dir is not None:
            ev, az = dirs[p.dir]
    snd = [(s, sg[s] * gain, _filter(p.sflt) if s == 0 else ol.default_filter()) for s in range(sends)]
    if hrtf:
        return ol.make_voice_params(step, rs, hrtf=(ev, az, 2.0, 0.0, gain), direct_filter=_filter(p.flt), sends=snd)
    return ol.make_voice_params(step, rs, dry_gains=dry * gain, direct_filter=_filter(p.flt), sends=snd)


def _ints(st, sends):
    out = (st.play_state, st.position, st.position_frac, st.has_buffer, st.fading, st.hrtf_old_delay[0], st.hrtf_old_delay[1],
           st.direct_lp.counter, st.direct_hp.counter)
    if sends:
        out += (st.send_lp[0].counter, st.send_hp[0].counter)
    return out


def _floats(st, sends):
    out = dict(direct_lp=st.direct_lp.as_tuple(), direct_hp=st.direct_hp.as_tuple(), hrtf_old_gain=st.hrtf_old_gain,
               dry_current=tuple(st.dry_current[:5]))
    if sends:
        out.update(send_lp=st.send_lp[0].as_tuple(), send_hp=st.send_hp[0].as_tuple())
    return out


def run(L, schedule, form, mhr=None, delivery="set_params", scene_kw=None, kernel_names=None, stats=None, roles=None,
        mixed=True, total=None, hold=None, early=False):
    """One schedule's roles on one scene.  delivery: 'set_params' (the synchronous call), 'block' (param_block + apply_block),
    'run' (mix_run with one block per update); a scene without parameter blocks (the oracle's) takes set_params.  roles: the
    roles to play (all of the form's); mixed: every fourth voice a filler; total: pad with fillers to this many voices, the
    roles spread over the range (then the integer state is read of the roles and a few fillers only); hold: {role: j}, roles
    that keep params(j) from update j on (one that is stopped or started in the schedule is not).  early: params(k + 1) go in
    right behind update k, in front of the read-back.
    Returns (buses per update, integer state per watched voice per update (None: no such voice yet),
             dict(roles={name: voice}, watched=[voice], floats=[{name: filter and gain state} per update]))."""
    todo = SCHEDULES[schedule]
    hold = hold or {}
    hrtf = form.startswith("hrtf")
    sends = FORM_SENDS[form]
    names = role_names(form, roles)
    slots = lc.layout(names, mixed, total)
    assert total is not None or len(slots) <= 64
    start = [START.get(n, 0) if e else 0 for n, e in slots]
    if any(start):
        assert total is None and start[-1] and not any(start[:-1]), "a voice added later is the scene's last"
    if hrtf:
        L.hrtf_load(mhr)
    dirs = directions(mhr) if hrtf else None
    sc = L.make_scene(num_dry=4 if hrtf else 5, num_real=2 if hrtf else 0, num_sends=sends, num_slots=sends,
                      wet_channels=4, hrtf=hrtf, **(scene_kw or {}))
    if kernel_names is not None:
        kernel_names.append(sc.voice_kernel_name())
    if hrtf:
        rng = np.random.default_rng(5)
        cc = np.zeros((4, 128, 2), np.float32)
        cc[:, :64] = rng.uniform(-0.2, 0.2, (4, 64, 2))
        sc.set_direct_hrtf(cc, [1.0, 0.8, 0.8, 0.8], 400.0 / 48000.0, 64)
    bufs = [sc.add_buffer(lc.encode(lc.buffer_data(b, seed=31 + j), b.fmt), b.fmt, loop_start=b.ls, loop_end=b.le)
            for j, b in enumerate(BUFS)]
    blocks_ok = hasattr(sc, "param_block") and delivery != "set_params"
    assert delivery in ("set_params", "block", "run") and not (early and delivery == "run")
    if blocks_ok and delivery == "run":
        sc.resident_set_short_run(0)
    role_of = {n: i for i, (n, e) in enumerate(slots) if e}
    watched = list(range(len(slots))) if total is None else sorted(set(role_of.values()) | {0, len(slots) // 2, len(slots) - 1})

    def plan(k, last):
        """what happens before update k: (voices added, voices whose parameters change, those parameters, voices stopped)"""
        adds, ids, ps, stops = [], [], [], []
        for i, (n, e) in enumerate(slots):
            held = e and n in hold
            if k < start[i] or (held and start[i]):
                continue
            if k == start[i]:
                adds.append(i)
            if e and n == "stop_in_flight" and not held and k > STOP_UPDATE:
                continue
            p = voice_params(i, n if e else None, min(k, hold[n]) if held else k, hrtf, sends, dirs)
            if last.get(i) != bytes(p):
                last[i] = bytes(p)
                ids.append(i)
                ps.append(p)
            if e and not held and ROLES[n](k).stop:
                stops.append(i)
        return adds, ids, ps, stops

    last = {}
    plans = [plan(k, last) for k in range(len(todo))]

    def add(i):
        assert sc.add_voice(bufs[i % 2], looping=True, position=(i * 7919) % 4800 + 100, frac=(i * 977) % 65536) == i

    for i in plans[0][0]:
        add(i)
    # every block is staged before the first update, as a host with a scripted scene stages them: a context that defers its
    # update submits it with the next call, whatever that call is, and only oalgpu_param_block_apply hands it its block
    blocks = [sc.param_block(np.array(ids), (ol.VoiceParams * len(ps))(*ps)) if blocks_ok and ids else None
              for _, ids, ps, _ in plans]

    def deliver(k):
        """what happens before update k; -> its parameter block (a 'run' delivery hands it to mix_run)"""
        adds, ids, ps, stops = plans[k]
        for i in (adds if k else ()):
            add(i)
        if blocks_ok and delivery == "block" and blocks[k] is not None:
            sc.apply_block(blocks[k])
        elif not blocks_ok:
            for i, p in zip(ids, ps):
                sc.set_params(i, p)
        for i in stops:
            sc.set_state(i, ol.VOICE_STOPPING)
        return blocks[k]

    buses, ints, floats = [], [], []
    block = deliver(0)
    for k, n in enumerate(todo):
        if k and not early:
            block = deliver(k)
        if blocks_ok and delivery == "run":
            sc.mix_run([block], n, post_process=hrtf)
        else:
            sc.mix(n, post_process=hrtf)
        if early and k + 1 < len(todo):
            deliver(k + 1)
        out = [sc.dry()[:, :n].ravel()]
        if hrtf:
            out.append(sc.hrtf_accum().ravel())
        for s in range(sends):
            out.append(sc.wet(s)[:, :n].ravel())
        buses.append(np.concatenate(out))
        exists = k + 1 if early else k
        sts = {i: sc.voice_state(i) for i in watched if start[i] <= exists and not (slots[i][1] and slots[i][0] in hold and start[i])}
        ints.append([_ints(sts[i], sends) if i in sts else None for i in watched])
        floats.append({nm: _floats(sts[i], sends) for nm, i in role_of.items() if i in sts})
    if stats is not None:
        stats.append(sc.resident_stats())
    sc.close()
    return buses, ints, dict(roles=role_of, watched=watched, floats=floats)
