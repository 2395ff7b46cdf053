"""Cases and the reference side of the parameter stage for multi-channel and non-spatialized sources
(oalgpu_voice_set_channel_sources, ChannelParamsKernel, oalgpu_channel_source_params_host), on top of source_param_cases.

* calc(): a numpy restatement, from the reference's sources and independent of csrc/dev_source_channels.hpp, of CalcVoiceParams'
  route (alc/alu.cpp:2024-2030, DirectChannels off), of CalcNonAttnVoiceParams (:1659-1710) and of the multi-channel legs of
  CalcHrtfPanning (:1229-1310) and CalcNormalPanning (:1365-1465) over the channel maps (:892-897, :1471-1521) with
  GetPanGainSelector (:1079-1113); the attenuated route's gains, distance, spread, direction, step and filters are
  source_param_cases.calc's.  One numpy scalar operation of the chosen type per operation of the reference (float32: its
  arithmetic; float64: the same formulas without its rounding).  tests/test_channel_source_host.py pins mStep of the
  non-attenuated route against the compiled reference's stereo sources, exactly.
* table(): 308 seeded channel sources over every branch (test_channel_source_host.py counts them).  As in source_param_cases
  a case is dropped if the restatement changes a branch or an integer result under a +-4 ulp nudge of every float input; a case
  whose warped channel position is shorter than 1e-3 is dropped too (the reference divides by that length).  The warp's
  `len < 1` is NOT such a branch: with no spread the warped position IS the unit direction and its length falls on either side
  of 1 by rounding, where dividing by it changes the last bit only.
* TOLERANCE: per output class, by source_param_cases' method (8 x the largest float32-against-float64 disagreement of the
  restatement over the kept cases, both contexts).  Measured here (test_channel_source_host.py prints the figures):

      class      float32 vs float64 over this table    source_param_cases.NOISE    tolerance
      gain       1.4e-06                               1.8e-05                     1.5e-04 (source_param_cases')
      gain_hf    0 (no cone, no absorption here)       1.3e-07                     1.1e-06 (source_param_cases')
      angle      3.78e-07                              1.3e-07                     3.1e-06 (8 x 3.78e-07)
      pan        5.1e-07                               1.8e-05                     1.5e-04 (source_param_cases')
      coeff      2.08e-07                              2.0e-07                     1.7e-06 (8 x 2.08e-07)

  (angle: the azimuth of a warped and renormalised channel position, atan2 of two rounded quotients.)

  A class that stays under source_param_cases.NOISE keeps source_param_cases.TOLERANCE; one that does not gets 8 x its own
  figure.
"""
import numpy as np

import oalgpu
import source_param_cases as sc
from oalgpu import synth

F32 = np.float32
MONO, STEREO, REAR, QUAD, X51, X61, X71 = range(7)
OFF, ON, AUTO = range(3)
LAYOUT_NAMES = ("mono", "stereo", "rear", "quad", "x51", "x61", "x71")
L, R, C, LFE = range(4)

SIN30, COS30 = 0.5, 0.866025403785
SIN45 = COS45 = float(F32(np.sqrt(2.0)) * F32(0.5))
SIN110, COS110 = 0.939692620786, -0.342020143326
# ChanPosMap (alu.cpp:1471-1510): (channel's side for GetPanGainSelector, position); StereoMap's positions come from StereoPan
MAPS = {
    MONO: [(C, (0.0, 0.0, -1.0))],
    STEREO: [(L, None), (R, None)],
    REAR: [(L, (-SIN30, 0.0, COS30)), (R, (SIN30, 0.0, COS30))],
    QUAD: [(L, (-SIN45, 0.0, -COS45)), (R, (SIN45, 0.0, -COS45)), (L, (-SIN45, 0.0, COS45)), (R, (SIN45, 0.0, COS45))],
    X51: [(L, (-SIN30, 0.0, -COS30)), (R, (SIN30, 0.0, -COS30)), (C, (0.0, 0.0, -1.0)), (LFE, (0.0, 0.0, 0.0)),
          (L, (-SIN110, 0.0, -COS110)), (R, (SIN110, 0.0, -COS110))],
    X61: [(L, (-SIN30, 0.0, -COS30)), (R, (SIN30, 0.0, -COS30)), (C, (0.0, 0.0, -1.0)), (LFE, (0.0, 0.0, 0.0)),
          (C, (0.0, 0.0, 1.0)), (L, (-1.0, 0.0, 0.0)), (R, (1.0, 0.0, 0.0))],
    X71: [(L, (-SIN30, 0.0, -COS30)), (R, (SIN30, 0.0, -COS30)), (C, (0.0, 0.0, -1.0)), (LFE, (0.0, 0.0, 0.0)),
          (L, (-SIN30, 0.0, COS30)), (R, (SIN30, 0.0, COS30)), (L, (-1.0, 0.0, 0.0)), (R, (1.0, 0.0, 0.0))],
}
DEFAULT_STEREO_PAN = (float(F32(np.pi) / F32(6.0)), float(-F32(np.pi) / F32(6.0)))       # pi_v<float> / 6.0f

# source_param_cases' listeners, and one whose XScale / ZScale push the direction out of the unit sphere (len >= 1 in the warp)
LISTENERS = list(sc.LISTENERS) + [sc.listener(distance_model=sc.INVERSE_CLAMPED, xyz_scale=(1.25, 1.0, 1.25))]
SCALED_LISTENER = len(LISTENERS) - 1

# measured by measure_noise() over the kept cases (test_channel_source_host.py asserts that these are the figures)
NOISE = {"gain": 1.4e-06, "gain_hf": 0.0, "angle": 3.78e-07, "pan": 5.1e-07, "coeff": 2.08e-07}
OWN_TOLERANCE = {"angle": 3.1e-06, "coeff": 1.7e-06}       # 8 x, rounded up to two digits, where NOISE exceeds source_param_cases.NOISE
TOLERANCE = {k: (sc.TOLERANCE[k] if NOISE[k] <= sc.NOISE[k] else OWN_TOLERANCE[k]) for k in NOISE}


def channel_source(src, channels, spatialize=AUTO, stereo_pan=DEFAULT_STEREO_PAN, panning=0.0):
    return dict(src=src, channels=channels, spatialize=spatialize, stereo_pan=list(stereo_pan), panning=panning)


def for_cfg(cs, cfg):
    return dict(cs, src=sc.for_cfg(cs["src"], cfg))


def attenuated(cs):
    """CalcVoiceParams' route with DirectChannels off (alu.cpp:2024-2030): True = CalcAttnVoiceParams"""
    return not (cs["spatialize"] == OFF or (cs["spatialize"] == AUTO and cs["channels"] != MONO))


def source_struct(cs, voices=()):
    return oalgpu.ChannelSource.make(sc.props_struct(cs["src"]), cs["channels"], cs["spatialize"], voices, cs["stereo_pan"], cs["panning"])


def sources_array(css, voices=None):
    arr = (oalgpu.ChannelSource * len(css))()
    for i, cs in enumerate(css):
        arr[i] = source_struct(cs, voices[i] if voices is not None else ())
    return arr


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _calc_non_attenuated(src, lis, env, cfg, F, nudge):
    """CalcNonAttnVoiceParams (alu.cpp:1659-1710) and the filters of CalcPanningAndFilters (:1619-1656), in source_param_cases.calc's
    result form"""
    def inp(name, v):
        v = F32(v)
        if nudge is not None:
            v = nudge(name, v)
        return F(v)
    c = lambda v: F(F32(v))
    zero, one = F(0.0), F(1.0)
    numsends = cfg["num_sends"]
    direct = [inp("direct%d" % i, v) for i, v in enumerate(src["direct"])]
    sends = [[s[0]] + [inp("send%d_%d" % (k, i), v) for i, v in enumerate(s[1:])] for k, s in enumerate(src["send"])]
    sendslots = [-1] * sc.MAX_SENDS
    for i in range(numsends):
        slot = sends[i][0]
        if slot >= 0 and env[slot]["active"]:
            sendslots[i] = slot
    # :1679-1686
    pitch = F(F32(cfg["frequency"])) / F(F32(cfg["sample_rate"])) * inp("pitch", src["pitch"])
    if pitch > c(10.0):
        step = 10 << 16
    else:
        step = max(int(np.rint(np.float64(pitch * c(65536.0)))), 1)
    rs_kind, rs_si, rs_sf = sc.prepare_resampler(src["resampler"], step, F)
    # :1688-1706
    gain, min_gain, max_gain, lgain = inp("gain", src["gain"]), inp("min_gain", src["min_gain"]), inp("max_gain", src["max_gain"]), inp("l_gain", lis["gain"])
    mingain = min(min_gain, max_gain)
    branch = {"src_clamp": -1 if gain < mingain else (1 if max_gain < gain else 0)}
    srcgain = mingain if gain < mingain else (max_gain if max_gain < gain else gain)
    mixmax = c(1000.0)
    branch["dry_ceiling"] = bool(srcgain * direct[0] * lgain > mixmax)
    dry = [min(mixmax, srcgain * direct[0] * lgain), direct[1], direct[3]]
    wet = [[min(mixmax, srcgain * sends[i][1] * lgain), sends[i][2], sends[i][4]] for i in range(numsends)]
    # :1619-1656
    inv_rate = one / F(F32(cfg["sample_rate"]))
    coeffs = [sc._design_shelf(True, direct[2] * inv_rate, dry[1], F), sc._design_shelf(False, direct[4] * inv_rate, dry[2], F)]
    coeffs += [sc._design_shelf(True, sends[i][3] * inv_rate, wet[i][1], F) for i in range(numsends)]
    coeffs += [sc._design_shelf(False, sends[i][5] * inv_rate, wet[i][2], F) for i in range(numsends)]
    active = [bool(dry[1] != one or dry[2] != one)] + [bool(wet[i][1] != one or wet[i][2] != one) for i in range(numsends)]
    return dict(step=step, rs=(rs_kind, rs_si), rs_sf=rs_sf, send_slot=sendslots, filter_active=active, dry=dry, wet=wet,
                distance=zero, spread=zero, dir=[zero, zero, -one], ev=zero, az=zero, hrtf_dist=F(np.inf), coeffs=coeffs, branch=branch,
                hf_norm=[direct[2] * inv_rate] + [sends[i][3] * inv_rate for i in range(numsends)],
                lf_norm=[direct[4] * inv_rate] + [sends[i][5] * inv_rate for i in range(numsends)])


def _line_gains(pos, spread, gain, amap, F, n):
    co = sc._ambi_coeffs(-pos[0], pos[1], -pos[2], spread, F)
    out = [F(0.0)] * n
    for t, (idx, scale) in enumerate(zip(*amap)):
        out[t] = F(F32(scale)) * co[idx] * gain
    return out


def calc(cs, lis, env, cfg, F=F32, nudge=None):
    """-> (base, channels): base = the source's results in source_param_cases.calc's form (either route), channels[c] = what
    CalcPanningAndFilters leaves in channel voice c"""
    def inp(name, v):
        v = F32(v)
        if nudge is not None:
            v = nudge(name, v)
        return F(v)
    c = lambda v: F(F32(v))
    zero, one = F(0.0), F(1.0)
    src, layout = cs["src"], cs["channels"]
    base = sc.calc(src, lis, env, cfg, F, nudge) if attenuated(cs) else _calc_non_attenuated(src, lis, env, cfg, F, nudge)
    base["branch"]["route"] = attenuated(cs)
    numsends = cfg["num_sends"]
    dry0, wet0 = base["dry"][0], [w[0] for w in base["wet"]]
    distance, spread, d3 = base["distance"], base["spread"], base["dir"]
    has_distance = bool(distance > F(sc.EPS))
    base["branch"]["has_distance"] = has_distance

    def finish(ch, pos, pangain, dry_spread, send_spread):
        ch["pos"], ch["pangain"] = pos, pangain
        ch["dry"] = dry0 * pangain
        ch["wet"] = [w * pangain for w in wet0]
        ch["dry_gains"] = [zero] * 32 if cfg["hrtf"] else _line_gains(pos, dry_spread, ch["dry"], cfg["dry_map"], F, 32)
        ch["send_gains"] = [[zero] * 25 for _ in range(sc.MAX_SENDS)]
        for i in range(numsends):
            if base["send_slot"][i] >= 0:
                ch["send_gains"][i] = _line_gains(pos, send_spread, ch["wet"][i], cfg["wet_map"], F, 25)
        return ch

    if layout == MONO:
        # the mono 3D point source's own legs (:1209-1227, :1343-1362; MonoMap without distance): source_param_cases' subject.  Panning
        # does not reach it: al/source.cpp hands 0 down unless mPanningEnabled
        ch = dict(silent=False, ev=base["ev"], az=base["az"], hrtf_dist=base["hrtf_dist"], hrtf_spread=spread, short=None, length=None)
        return base, [finish(ch, d3, one, spread, spread)]

    # GetPanGainSelector, :1079-1113
    panning = inp("panning", cs["panning"])
    lgain, rgain = min(one - panning, one), min(one + panning, one)
    side_gain = {L: lgain, R: rgain, C: min(lgain, rgain)}
    channels = []
    for k, (side, mpos) in enumerate(MAPS[layout]):
        if side == LFE:
            # skipped by CalcHrtfPanning; CalcNormalPanning's one audible case needs Dry.Buffer == RealOut.Buffer
            ch = dict(silent=True, ev=zero, az=zero, hrtf_dist=base["hrtf_dist"], hrtf_spread=zero, short=None, length=None)
            ch = finish(ch, [zero, zero, zero], zero, zero, zero)
            ch["dry_gains"] = [zero] * 32
            ch["send_gains"] = [[zero] * 25 for _ in range(sc.MAX_SENDS)]
            channels.append(ch)
            continue
        if layout == STEREO:
            a = inp("stereo_pan%d" % k, cs["stereo_pan"][k])
            cpos = [-np.sin(a), zero, -np.cos(a)]          # :1555-1561, for the default angles too
        else:
            cpos = [c(v) for v in mpos]
        pangain = side_gain[side]
        ch = dict(silent=False, short=None, length=None)
        if has_distance:
            a = one - (c(1.0 / np.pi) * F(0.5)) * spread
            pos = [cpos[i] + (d3[i] - cpos[i]) * a for i in range(3)]
            length = np.sqrt(pos[0] * pos[0] + pos[1] * pos[1] + pos[2] * pos[2])
            ch["short"], ch["length"] = bool(length < one), float(length)
            if length < one:
                pos = [v / length for v in pos]
            ch["ev"] = np.arcsin(min(max(pos[1], -one), one)) if cfg["hrtf"] else zero
            ch["az"] = np.arctan2(pos[0], -pos[2]) if cfg["hrtf"] else zero
            ch["hrtf_dist"], ch["hrtf_spread"] = base["hrtf_dist"], zero
            channels.append(finish(ch, pos, pangain, zero, zero))
        else:
            pos = cpos
            ch["ev"] = np.arcsin(pos[1]) if cfg["hrtf"] else zero
            ch["az"] = np.arctan2(pos[0], -pos[2]) if cfg["hrtf"] else zero
            ch["hrtf_dist"], ch["hrtf_spread"] = F(np.inf), zero                    # spreadmult = 0: not a mono 3D source
            # :1302: the HRTF leg's sends take `spread`, not spreadmult; CalcNormalPanning's both take spreadmult
            channels.append(finish(ch, pos, pangain, zero, spread if cfg["hrtf"] else zero))
    return base, channels


def voice_params(base, ch, src, cfg):
    """channel voice `ch` of the restatement's results as an oalgpu_voice_params"""
    p = oalgpu.VoiceParams()
    p.step = base["step"]
    p.resampler = src["resampler"]
    p.direct_filter = oalgpu.FilterParams(int(base["filter_active"][0]), float(base["dry"][1]), float(base["hf_norm"][0]),
                                          float(base["dry"][2]), float(base["lf_norm"][0]))
    p.dry_gains[:] = [float(x) for x in ch["dry_gains"]]
    p.hrtf_ev, p.hrtf_az, p.hrtf_dist, p.hrtf_spread = float(ch["ev"]), float(ch["az"]), float(ch["hrtf_dist"]), float(ch["hrtf_spread"])
    p.hrtf_gain = float(ch["dry"])
    for i in range(sc.MAX_SENDS):
        p.send_slot[i] = base["send_slot"][i]
    for i in range(cfg["num_sends"]):
        p.send_filter[i] = oalgpu.FilterParams(int(base["filter_active"][1 + i]), float(base["wet"][i][1]), float(base["hf_norm"][1 + i]),
                                               float(base["wet"][i][2]), float(base["lf_norm"][1 + i]))
        p.send_gains[i][:] = [float(x) for x in ch["send_gains"][i]]
    return p


def check_voice_params(vp, base, ch, cfg, who=""):
    """an oalgpu_voice_params of oalgpu_channel_source_params_host against the restatement: integers exact, floats within
    TOLERANCE of their class (source_param_cases.check_voice_params' classes and scales; a gain's scale is the source's, before
    pangain)"""
    ns = cfg["num_sends"]
    assert vp.step == base["step"], (who, vp.step, base["step"])
    assert [vp.send_slot[i] for i in range(sc.MAX_SENDS)] == list(base["send_slot"]), who
    assert [vp.direct_filter.active] + [vp.send_filter[i].active for i in range(ns)] == [int(a) for a in base["filter_active"]], who

    def close(x, y, tol, floor, what):
        x, y = float(x), float(y)
        if not np.isfinite(y):
            assert x == y, (who, what, x, y)
            return
        assert abs(x - y) <= tol * max(abs(y), floor), (who, what, x, y, abs(x - y) / max(abs(y), floor), tol)
    close(vp.hrtf_gain, ch["dry"], TOLERANCE["gain"], max(1e-3, float(base["dry"][0])), "dry base")
    close(vp.direct_filter.gain_hf, base["dry"][1], TOLERANCE["gain_hf"], 1e-3, "dry hf")
    assert vp.direct_filter.gain_lf == float(base["dry"][2]) and vp.direct_filter.hf_norm == float(base["hf_norm"][0]), who
    assert vp.direct_filter.lf_norm == float(base["lf_norm"][0]), who
    top = max([1e-3, float(base["dry"][0])] + [float(w[0]) for w in base["wet"]])
    for i in range(ns):
        close(vp.send_filter[i].gain_hf, base["wet"][i][1], TOLERANCE["gain_hf"], 1e-3, "wet hf")
        assert vp.send_filter[i].gain_lf == float(base["wet"][i][2]), who
        for t in range(25):
            close(vp.send_gains[i][t], ch["send_gains"][i][t], TOLERANCE["pan"], top, "send gain")
    for t in range(32):
        close(vp.dry_gains[t], ch["dry_gains"][t], TOLERANCE["pan"], top, "dry gain")
    if ch["silent"]:
        assert vp.hrtf_gain == 0.0 and not any(vp.dry_gains) and not any(any(g) for g in vp.send_gains), who
    elif cfg["hrtf"]:
        for x, y, what in ((vp.hrtf_ev, ch["ev"], "ev"), (vp.hrtf_az, ch["az"], "az"), (vp.hrtf_spread, ch["hrtf_spread"], "spread")):
            err = abs(float(x) - float(y))
            assert min(err, 2.0 * np.pi - err) <= TOLERANCE["angle"] * np.pi, (who, what, x, y)   # (an azimuth of +-pi: one direction)
        close(vp.hrtf_dist, ch["hrtf_dist"], 2.0 ** -22, 1e-3, "hrtf distance")


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def _build():
    lcg = synth.Lcg(0x5EED0061)
    cases = []
    k = 0

    def base(head_relative=None):
        nonlocal k
        k += 1
        s = sc._base(lcg, k)
        if head_relative is not None:
            s["head_relative"] = head_relative
        return s

    def add(tag, lis, env, cs):
        cases.append(dict(tag=tag, lis=lis, env=env, cs=cs))

    def pan(n):
        return (-lcg.uniform(0.2, 0.9), 0.0, lcg.uniform(0.2, 0.9))[n % 3]

    def stereo_pan(n):
        return DEFAULT_STEREO_PAN if n % 2 == 0 else (lcg.uniform(0.1, 1.4), -lcg.uniform(0.1, 1.4))
    multi = (STEREO, REAR, QUAD, X51, X61, X71)
    for rep in range(8):
        env = rep % 2
        for layout in range(7):                             # every layout under every spatialize mode
            for mode in (OFF, ON, AUTO):
                add("%s_%s" % (LAYOUT_NAMES[layout], ("off", "on", "auto")[mode]), 0, env,
                    channel_source(base(), layout, mode, stereo_pan(rep + layout), pan(rep + layout + mode)))
        layout = multi[rep % 6]
        # radius 0 / inside / around the listener, the source away from it and at it
        here = [0.0, 0.0, 0.0]
        for what in ("zero", "below", "above"):
            s = base(1)
            dist = float(np.linalg.norm(np.array(s["position"])))
            s["radius"] = {"zero": 0.0, "below": dist * lcg.uniform(0.1, 0.8), "above": dist * lcg.uniform(1.2, 3.0)}[what]
            add("radius_" + what, 0, env, channel_source(s, multi[(rep + 1) % 6] if what == "below" else layout, ON, panning=pan(rep)))
        s = base(1); s["position"] = here; s["radius"] = 0.0
        add("at_listener", 0, env, channel_source(s, layout, ON, panning=pan(rep + 1)))
        for n in range(2 if rep < 4 else 1):
            s = base(1); s["position"] = here; s["radius"] = 1.5; s["send"][0][0] = 0
            add("at_listener_radius", 0, env, channel_source(s, multi[(rep + 3 * n) % 6], ON, panning=pan(rep + 2)))
        # a direction pushed out of the unit sphere by XScale / ZScale: len >= 1 in the warp, with and without a radius
        s = base(1); s["distance_model"] = sc.INVERSE_CLAMPED; s["position"] = [lcg.uniform(1.0, 3.0) * (1 if rep % 2 else -1), 0.1, -lcg.uniform(0.2, 2.0)]
        s["radius"] = (0.0, 0.2)[rep % 2]
        add("scaled_direction", SCALED_LISTENER, env, channel_source(s, layout, ON, panning=pan(rep)))
        # a send into the inactive slot of environment 1
        s = base(); s["send"][0][0] = 1; s["send"][1][0] = 1
        add("inactive_slot", 0, 1, channel_source(s, layout, (OFF, ON)[rep % 2], panning=pan(rep)))
        # Gain outside [MinGain, MaxGain] and the GainMixMax ceiling on the non-attenuated route
        for n in range(2 if rep < 4 else 1):
            s = base(); s["gain"] = lcg.uniform(1.5, 4.0); s["max_gain"] = lcg.uniform(0.5, 1.0)
            add("gain_above_max", 0, env, channel_source(s, multi[(rep + 3 * n) % 6], OFF, panning=pan(rep)))
            s = base(); s["gain"] = lcg.uniform(0.05, 0.2); s["min_gain"] = lcg.uniform(0.3, 0.6)
            add("gain_below_min", 0, env, channel_source(s, multi[(rep + 3 * n) % 6], AUTO, panning=pan(rep + 1)))
        s = base(); s["gain"] = lcg.uniform(30.0, 60.0); s["max_gain"] = 100.0; s["direct"][0] = 40.0; s["send"][0][1] = 35.0
        add("gain_mix_max", 0, env, channel_source(s, layout, OFF, panning=pan(rep + 2)))
        # StereoPan away from +-30 degrees on both routes
        add("stereo_pan_on", 0, env, channel_source(base(), STEREO, ON, stereo_pan(1), pan(rep)))
        add("stereo_pan_off", 0, env, channel_source(base(), STEREO, OFF, stereo_pan(1), pan(rep + 1)))
        # the non-attenuated step below / at / above one and above MaxPitch, over the resamplers
        for n in range(4):
            rsm = (rep * 4 + n) % 10
            what = ("below", "at", "above", "max_pitch")[n]
            s = base(); s["resampler"] = rsm
            s["pitch"] = {"below": lcg.uniform(0.3, 0.95) * 48000.0 / 44100.0, "at": 48000.0 / 44100.0,
                          "above": lcg.uniform(1.1, 6.0) * 48000.0 / 44100.0, "max_pitch": lcg.uniform(11.0, 14.0)}[what]
            add("step_" + what, 0, env, channel_source(s, layout, (OFF, AUTO)[n % 2], panning=pan(n)))
    return cases


def integer_results(base, channels):
    """what must not move under a +-4 ulp nudge of the inputs (HRIR indices of channel positions are NOT among them: the maps'
    azimuths sit on the default data set's 2 degree grid, where one ulp of atan2 picks the neighbouring pair with weights (1 - e, e))"""
    out = sc.integer_results(base)
    out["silent"] = tuple(ch["silent"] for ch in channels)
    return out


MIN_LENGTH = 1e-3
_TABLE = None


def table():
    """-> (kept cases, dropped cases)"""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    kept, dropped = [], []
    patterns = [lambda name: 1, lambda name: -1]
    for case in _build():
        stable = True
        lis, env = LISTENERS[case["lis"]], sc.ENVIRONMENTS[case["env"]]
        for cfg in (sc.DRY_CFG, sc.HRTF_CFG):
            cs = for_cfg(case["cs"], cfg)
            base, channels = calc(cs, lis, env, cfg)
            want = integer_results(base, channels)
            if any(ch["length"] is not None and ch["length"] < MIN_LENGTH for ch in channels):
                stable = False
            for sign_of in patterns:
                if stable and integer_results(*calc(cs, lis, env, cfg, nudge=sc._ulp_nudge(4, sign_of))) != want:
                    stable = False
            if not stable:
                break
        (kept if stable else dropped).append(case)
    _TABLE = (kept, dropped)
    return _TABLE


def measure_noise(cases):
    """source_param_cases.measure_noise over channel sources: the largest float32-against-float64 disagreement of the restatement
    per output class, each channel voice counted"""
    noise = {k: 0.0 for k in NOISE}

    def rel(a, b, floor):
        a, b = float(a), float(b)
        if not np.isfinite(b):
            return 0.0
        return abs(a - b) / max(abs(b), floor)
    for case in cases:
        lis, env = LISTENERS[case["lis"]], sc.ENVIRONMENTS[case["env"]]
        for cfg in (sc.DRY_CFG, sc.HRTF_CFG):
            cs = for_cfg(case["cs"], cfg)
            (a, ach), (b, bch) = calc(cs, lis, env, cfg, F32), calc(cs, lis, env, cfg, np.float64)
            top = max(1e-3, float(b["dry"][0]), *[float(w[0]) for w in b["wet"]])
            for x, y in [(a["dry"][1], b["dry"][1])] + [(a["wet"][i][1], b["wet"][i][1]) for i in range(cfg["num_sends"])]:
                noise["gain_hf"] = max(noise["gain_hf"], rel(x, y, 1e-3))
            for ca, cb in zip(a["coeffs"], b["coeffs"]):
                for x, y in zip(ca, cb):
                    noise["coeff"] = max(noise["coeff"], rel(x, y, 1.0))
            for p, q in zip(ach, bch):
                noise["gain"] = max(noise["gain"], rel(p["dry"], q["dry"], max(1e-3, float(b["dry"][0]))))
                for i in range(cfg["num_sends"]):
                    noise["gain"] = max(noise["gain"], rel(p["wet"][i], q["wet"][i], max(1e-3, float(b["wet"][i][0]))))
                for x, y in ((p["ev"], q["ev"]), (p["az"], q["az"]), (p["hrtf_spread"], q["hrtf_spread"])):
                    err = abs(float(x) - float(y))
                    noise["angle"] = max(noise["angle"], min(err, 2.0 * np.pi - err) / np.pi)
                for x, y in zip(p["dry_gains"] + sum(p["send_gains"], []), q["dry_gains"] + sum(q["send_gains"], [])):
                    noise["pan"] = max(noise["pan"], rel(x, y, top))
    return noise
