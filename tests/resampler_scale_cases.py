"""Every resampler at every scale of its bsinc table: the steps, the update lengths, the scenes and a numpy restatement of
one resampled sample.

The bsinc resamplers pick one of 16 row sets by the step (BsincPrepare, alc/alu.cpp:140-164): the scale index `si`, its
tap count `m = table.m[si]`, the window offset `l = m/2 - 1` and, for the full bsinc above step 1.0, the factor `sf`
that blends the rows of `si` towards those of `si + 1`.  The voice kernels treat tap counts differently (rows staged in
LDS for some, read from the table in HBM for the rest), so every `si` of every bsinc resampler is a case of its own.

`steps_for(resampler)` is derived from the oracle's prepare_resampler and bsinc_table, not from a list: per scale index
the step range that reaches it is found by bisection (si falls as the step grows), and a middle step is chosen inside.
`run` plays one resampler on a scene through any object with the oracle_lib.Scene interface, in two layouts:
  one_key   one step on every voice: the workgroup's key voice carries the tested resampler, so the voices take the
            staged readers wherever the kernel stages that tap count;
  moving    all middle steps of the resampler at once, voice i on step (i + k) % len(steps) in update k, every fourth
            slot a quiet filler on another resampler: the generic loader, and keys and tap counts that change between
            updates.
`resample_one` restates one output sample of Resample_{Point,Linear,Cubic,FastBSinc,BSinc} (core/mixer/mixer_c.cpp:
40-105, mixer_sse.cpp:199-329, mixer_sse41.cpp:117-214) over the oracle's tables, with (si, sf, m, l) and the phase
index as arguments, so that tests/test_resampler_scales_host.py can perturb them."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import loop_edge_cases as lc
import oracle_lib as ol

FRAC_BITS = 16
FRAC_ONE = lc.FRAC_ONE
FRAC_MASK = FRAC_ONE - 1
MAX_PITCH = lc.MAX_PITCH
MAX_EDGE = lc.MAX_EDGE
SCALES = 16                     # BSincScaleCount
PHASES = 32                     # BSincPhaseCount and CubicPhaseCount
PHASE_DIFF_BITS = FRAC_BITS - 5
PHASE_DIFF_ONE = 1 << PHASE_DIFF_BITS

FAMILY = {ol.RS_FAST_BSINC12: 12, ol.RS_BSINC12: 12, ol.RS_FAST_BSINC24: 24, ol.RS_BSINC24: 24,
          ol.RS_FAST_BSINC48: 48, ol.RS_BSINC48: 48}
FULL_BSINC = (ol.RS_BSINC12, ol.RS_BSINC24, ol.RS_BSINC48)
PLAIN = (ol.RS_POINT, ol.RS_LINEAR, ol.RS_SPLINE, ol.RS_GAUSSIAN)
PLAIN_STEPS = (30000, 65536, 65537, 100000, 300000, 655360)
TOP_SCALE_STEPS = (60211, 65536)            # si = 15 is every step <= 1.0
RESAMPLERS = tuple(range(10))
NAMES = ("point", "linear", "spline", "gaussian", "fast_bsinc12", "bsinc12", "fast_bsinc24", "bsinc24", "fast_bsinc48",
         "bsinc48")

Step = namedtuple("Step", "step si role")       # role: 'middle' (played in scenes) | 'low' | 'high' (the range's ends)


def oracle():
    L = ol.load("ref" if ol.available("ref") else "port")
    L.L.oal_set_simd(1)
    return L


@lru_cache(maxsize=None)
def tables(family):
    return oracle().bsinc_table(family)


@lru_cache(maxsize=None)
def cubic(which):
    return oracle().cubic_table(which)


def scale_of(resampler, step):
    """(si, raw scale fraction, InterpState) of a bsinc resampler at a step, from the oracle's prepared state.  The raw
    fraction f is what BsincPrepare shapes into sf = 1 - sqrt(1 - f^2); it is recovered from sf."""
    st = oracle().prepare_resampler(resampler, step)
    si = tables(FAMILY[resampler])["filterOffset"].index(st.filter_offset)
    s = min(max(1.0 - float(st.sf), 0.0), 1.0)
    return si, float(np.sqrt(1.0 - s * s)), st


def _last_true(lo, hi, pred):
    """the largest x in [lo, hi] with pred(x), for a pred that holds on a prefix of the range that includes lo"""
    assert pred(lo)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


MIDDLE_FRACTION = 0.7           # the raw scale fraction aimed at: the middle of [0.5, 0.9]


@lru_cache(maxsize=None)
def steps_for(resampler):
    """[Step]: for the bsinc resamplers, per si in 0..14 the lowest, a middle and the highest step of the range that
    reaches it (middle: the largest step whose raw scale fraction is still >= MIDDLE_FRACTION), and two steps of
    si = 15; for the others PLAIN_STEPS."""
    if resampler in PLAIN:
        return tuple(Step(s, None, "middle") for s in PLAIN_STEPS)
    out = []
    high = MAX_PITCH
    for si in range(SCALES - 1):
        assert scale_of(resampler, high)[0] == si
        low = high + 1 - _last_true(1, high - FRAC_ONE, lambda d: scale_of(resampler, high + 1 - d)[0] == si)
        mid = _last_true(low, high, lambda s: scale_of(resampler, s)[1] >= MIDDLE_FRACTION)
        out += [Step(low, si, "low"), Step(mid, si, "middle"), Step(high, si, "high")]
        high = low - 1
    assert high == FRAC_ONE
    out += [Step(s, SCALES - 1, "middle") for s in TOP_SCALE_STEPS]
    return tuple(out)


def middle_steps(resampler):
    return tuple(s.step for s in steps_for(resampler) if s.role == "middle")


def todo_for(step):
    """Three update lengths: the longest whose first source window still fits the register gather's window whatever the
    voice's fraction, a whole line (over the window for steps above ~1.06: the chunked loader, CalcBufferSize's
    splitting), and a short ragged one."""
    n_fit = _last_true(1, 1024, lambda n: lc.calc_buffer_size(FRAC_MASK, step, n)[1] <= lc.WINDOW)
    return (n_fit, 1024, 37)


# ---------------------------------------------------------------------------------------------------- the scenes
BUF_FRAMES = 6000
TESTED_GAIN, FILLER_GAIN = 0.5, 1e-3
ONE_KEY_VOICES = 8              # two workgroups of the 4-wide kernels
MOVING_TESTED = 48              # + every fourth slot a filler = 64 slots; 3 updates put ~8 voices on each of 17 steps
FILLER_STEP, FILLER_RESAMPLER = lc.FILLER_STEP, lc.FILLER_RESAMPLER


def buffer_noise(seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, BUF_FRAMES)


def voice_start(i):
    """(buffer index 0..3, position, fraction) of slot i: formats alternate, positions cover the buffer (some windows
    wrap at the loop end), fractions cover the phases"""
    return i % 4, (i * 1543 + 211) % BUF_FRAMES, (i * 24593 + 40000) % FRAC_ONE


def slots_of(layout, nvoices=None):
    """[is_tested] per voice slot"""
    if layout == "one_key":
        return [True] * (nvoices or ONE_KEY_VOICES)
    assert layout == "moving"
    out = []
    while sum(out) < (nvoices or MOVING_TESTED):
        out.append(len(out) % 4 != 0)
    return out


def moving_todo(steps):
    return (min(todo_for(s)[0] for s in steps), 1024, 37)


def run(L, layout, resampler, steps, form="hrtf", mhr=None, nvoices=None, scene_kw=None, kernel_names=None):
    """One scene.  one_key: steps = (step,); moving: steps = the resampler's middle steps.
    Returns (buses per update, [(play state, position, fraction, has buffer, fading) per voice] per update, tested slots)."""
    slots = slots_of(layout, nvoices)
    todo = todo_for(steps[0]) if layout == "one_key" else moving_todo(steps)
    hrtf = form.startswith("hrtf")
    sends = {"hrtf": 0, "hrtf_sends": 1, "dry": 0, "dry_sends": 2}[form]
    if hrtf:
        L.hrtf_load(mhr)
    sc = L.make_scene(num_dry=4 if hrtf else 5, num_real=2 if hrtf else 0, num_sends=sends, num_slots=sends,
                      wet_channels=4, hrtf=hrtf, **(scene_kw or {}))
    if kernel_names is not None:
        kernel_names.append(sc.voice_kernel_name())
    if hrtf:
        rng = np.random.default_rng(5)
        cc = np.zeros((4, 128, 2), np.float32)
        cc[:, :64] = rng.uniform(-0.2, 0.2, (4, 64, 2))
        sc.set_direct_hrtf(cc, [1.0, 0.8, 0.8, 0.8], 400.0 / 48000.0, 64)
    bufs = []
    for b in range(4):
        fmt = ol.FMT_FLOAT if b % 2 == 0 else ol.FMT_SHORT
        bufs.append(sc.add_buffer(lc.encode(buffer_noise(700 + b), fmt), fmt))

    def params(i, k):
        tested = slots[i]
        gain = TESTED_GAIN if tested else FILLER_GAIN
        r = np.random.default_rng(1000 + i)
        snd = [(s, r.uniform(0.1, 0.4, 4) * gain, ol.default_filter()) for s in range(sends)]
        st, rs = (steps[(i + k) % len(steps)], resampler) if tested else (FILLER_STEP, FILLER_RESAMPLER)
        if hrtf:
            return ol.make_voice_params(st, rs, hrtf=(r.uniform(-0.5, 0.5), r.uniform(-np.pi, np.pi), 2.0, 0.0, gain),
                                        sends=snd)
        return ol.make_voice_params(st, rs, dry_gains=r.uniform(0.3, 1.0, 5) * gain, sends=snd)

    for i in range(len(slots)):
        b, pos, frac = voice_start(i)
        sc.add_voice(bufs[b], looping=True, position=pos, frac=frac)
    buses, ints = [], []
    for k, n in enumerate(todo):
        if k == 0 or len(steps) > 1:
            for i in range(len(slots)):
                if k == 0 or slots[i]:
                    sc.set_params(i, params(i, k))
        sc.mix(n, post_process=hrtf)
        out = [sc.dry()[:, :n].ravel()]
        if hrtf:
            out.append(sc.hrtf_accum().ravel())
        for s in range(sends):
            out.append(sc.wet(s)[:, :n].ravel())
        buses.append(np.concatenate(out))
        sts = []
        for i in range(len(slots)):
            st = sc.voice_state(i)
            sts.append((st.play_state, st.position, st.position_frac, st.has_buffer, st.fading))
        ints.append(sts)
    sc.close()
    return buses, ints, [i for i, t in enumerate(slots) if t]


# ---------------------------------------------------------------------------------------------------- the restatement
F = np.float32
PADDED = {}


def _tab(family):
    """the table with a tail of zeros: a row set addressed with another scale's tap count may reach past the end"""
    if family not in PADDED:
        PADDED[family] = np.concatenate([tables(family)["tab"], np.zeros(4 * PHASES * 48, np.float32)])
    return PADDED[family]


def resample_one(kind, src, pos, frac, table=None, si=None, sf=0.0, m=None, dphase=0, main_loop=True):
    """One output sample.  kind: 0 point, 1 linear, 2 cubic (table: 0 spline, 1 gaussian), 3 fast bsinc, 4 bsinc
    (table: 12, 24, 48).  src: float32 samples; pos: the first sample the filter reads (the caller has taken l off);
    dphase: added to the phase index (modulo the phase count).  The expressions are mixer_c.cpp's; the sums are taken
    in the SSE functions' order, which every test's oracle runs: four partial sums added (0+3)+(1+2), the cubic in the
    SSE4.1 main loop (0+1)+(2+3).  (The C loops' left-to-right sums round as the compiler contracts them.)"""
    if kind == 0:                                               # do_point
        return F(src[pos])
    if kind == 1:                                               # do_lerp: a + (b - a) * mu
        mu = F(frac) * F(1.0 / FRAC_ONE)
        return F(src[pos] + (src[pos + 1] - src[pos]) * mu)
    pi = ((frac >> PHASE_DIFF_BITS) + dphase) % PHASES
    pf = F(frac & (PHASE_DIFF_ONE - 1)) * F(1.0 / PHASE_DIFF_ONE)
    if kind == 2:                                               # do_cubic, Resample_Cubic_SSE / _SSE4
        row = cubic(table)[pi]
        r = (row[:4] + pf * row[4:]) * src[pos:pos + 4]
        if main_loop:
            return F(F(r[0] + r[1]) + F(r[2] + r[3]))
        return F(F(r[0] + r[3]) + F(r[1] + r[2]))
    tab = _tab(table)
    base = tables(table)["filterOffset"][si] + 2 * pi * m
    fil, phd = tab[base:base + m], tab[base + m:base + 2 * m]
    if kind == 3:                                               # do_fastbsinc: fil + pf*phd
        f = fil + pf * phd
    else:                                                       # do_bsinc: (fil + sf*scd) + pf*(phd + sf*spd)
        scd = tab[base + 2 * PHASES * m:base + 2 * PHASES * m + m]
        spd = tab[base + 2 * PHASES * m + m:base + 2 * PHASES * m + 2 * m]
        sf = F(sf)
        f = (fil + sf * scd) + pf * (phd + sf * spd)
    p = f * src[pos:pos + m]
    r4 = np.zeros(4, np.float32)
    for j in range(0, m, 4):
        r4 = r4 + p[j:j + 4]
    return F(F(r4[0] + r4[3]) + F(r4[1] + r4[2]))


def state_of(resampler, step):
    """the arguments of resample_one that PrepareResampler chooses: dict(kind, table, si, sf, m, l)"""
    st = oracle().prepare_resampler(resampler, step)
    if resampler in PLAIN:
        return dict(kind=st.kind, table=st.table if st.kind == 2 else None, si=None, sf=0.0, m=None,
                    l=1 if st.kind == 2 else 0)
    si = tables(st.table)["filterOffset"].index(st.filter_offset)
    return dict(kind=st.kind, table=st.table, si=si, sf=float(st.sf), m=int(st.m), l=int(st.l))


def resample_call(resampler, step, src, frac, n, dphase=0, **perturbed):
    """oal_resample restated: src[0] is MaxResamplerEdge samples before the first source sample.  perturbed: si, sf, m
    or l to use in place of what PrepareResampler chose."""
    s = dict(state_of(resampler, step), **perturbed)
    src = np.ascontiguousarray(src, np.float32)
    out = np.zeros(n, np.float32)
    pos = MAX_EDGE - s["l"]
    for i in range(n):
        out[i] = resample_one(s["kind"], src, pos, frac, table=s["table"], si=s["si"], sf=s["sf"], m=s["m"],
                              dphase=dphase, main_loop=i < (n & ~3))
        frac += step
        pos += frac >> FRAC_BITS
        frac &= FRAC_MASK
    return out
