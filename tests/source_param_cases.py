"""Cases and the reference side of the 3D source parameter stage (oalgpu_voice_set_source_props, SourceParamsKernel,
oalgpu_source_params_host).

* calc(): an op-for-op numpy restatement of the reference's CalcAttnVoiceParams (alc/alu.cpp:1712-2010) and of what
  CalcPanningAndFilters (:1512-1657; CalcHrtfPanning :1198-1311, CalcNormalPanning :1314-1469) does for a mono 3D point
  source, with BsincPrepare (:140-164), setParamsFromSlope / BiquadFilter::SetParams (core/filters/biquad.h:60-62, :172-177;
  biquad.cpp:48-129) and CalcAmbiCoeffs / ComputePanGains (core/ambidefs.h:219-265, core/mixer.cpp:16-102).  Written from the
  reference's sources, independent of csrc/dev_source.hpp; every operation is one numpy scalar operation of the chosen type
  (float32: the reference's arithmetic; float64: the same formulas without its rounding).  tests/test_source_params_host.py
  pins it against the compiled reference (mStep of 200 sources, exactly).
* table(): ~400 seeded sources (the LCG of SURVEY.md 8d) over every branch of the two functions, each under one of nine
  listeners and one of two slot environments.  A case is dropped at construction time if the restatement, with every float
  input nudged by +-4 ulp, changes a branch or an integer result (such a case tests the rounding of one operation, not
  the stage): at most 10 % of the table and no branch entirely (asserted by the CPU tests).
* TOLERANCE: per output class, 8 x the largest relative disagreement between the float32 and the float64 evaluation of the
  restatement over the table -- the reference's own rounding noise; the factor covers the device math library's documented
  bounds (up to 16 ulp for pow where glibc is under 1).  Measured on the CPU by measure_noise() over the kept cases, both
  contexts (test_source_params_host.py::test_tolerances_are_eight_times_the_reference_noise prints the figures and asserts
  that the constants below are those):

      class      what                                               float32 vs float64    tolerance
      gain       DryGain.Base, WetGain[i].Base / max(|x|, 1e-3)     1.8e-05               1.5e-04
      gain_hf    DryGain.HF, WetGain[i].HF / max(|x|, 1e-3)         1.3e-07               1.1e-06
      angle      HRTF elevation, azimuth; spread / pi               1.3e-07               1.1e-06
      pan        line gains / the largest Base gain of the source   1.8e-05               1.5e-04
      coeff      shelf coefficients / max(|x|, 1)                   2.0e-07               1.6e-06

  (gain and pan carry the cancellation of the linear model's 1 - scale * rolloff near its zero: the reference's own float32
  result is that far from the formula's value there.)
"""
import ctypes as C

import numpy as np

import oalgpu
from oalgpu import synth

F32 = np.float32
EPS = F32(1.1920928955078125e-07)
FRAC_ONE = 65536
MAX_SENDS = 6

# what the restatement's float32 and float64 evaluations disagree by at most over table(), per output class, relative to the
# class's scale (gains and filter coefficients: the larger of the value and 1e-3 resp. 1 -- a coefficient is a ratio of sums of
# order 1; angles: radians against pi), and the tolerance the device gets: 8 x, rounded up to two digits.  Measured by
# measure_noise() on the CPU; test_source_params_host.py asserts 8 * noise[k] <= TOLERANCE[k] <= 10 * noise[k].
NOISE = {"gain": 1.8e-05, "gain_hf": 1.3e-07, "angle": 1.3e-07, "pan": 1.8e-05, "coeff": 2.0e-07}
TOLERANCE = {"gain": 1.5e-04, "gain_hf": 1.1e-06, "angle": 1.1e-06, "pan": 1.5e-04, "coeff": 1.6e-06}

(DISABLE, INVERSE, INVERSE_CLAMPED, LINEAR, LINEAR_CLAMPED, EXPONENT, EXPONENT_CLAMPED) = range(7)
FLT_MAX = float(np.finfo(np.float32).max)


# ---------------------------------------------------------------------------------------------------------------------
# contexts
# ---------------------------------------------------------------------------------------------------------------------
def listener(matrix=None, position=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0), gain=1.0, meters_per_unit=1.0,
             air_absorption_gain_hf=0.99426, doppler_factor=1.0, speed_of_sound=343.3, source_distance_model=0,
             distance_model=DISABLE, cone_scale=1.0, nfc_scale=1.0, xyz_scale=(1.0, 1.0, 1.0)):
    """ContextParams{} (core/context.h:67-84) unless told otherwise"""
    return dict(matrix=list(matrix) if matrix is not None else [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1],
                position=list(position), velocity=list(velocity), gain=gain, meters_per_unit=meters_per_unit,
                air_absorption_gain_hf=air_absorption_gain_hf, doppler_factor=doppler_factor, speed_of_sound=speed_of_sound,
                source_distance_model=source_distance_model, distance_model=distance_model, cone_scale=cone_scale,
                nfc_scale=nfc_scale, xyz_scale=list(xyz_scale))


def _normalize32(v):
    v = [F32(x) for x in v]
    lsq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    if lsq > EPS:
        inv = F32(1.0) / np.sqrt(lsq)
        return [x * inv for x in v]
    return [F32(0.0)] * 3


def oriented_listener(at, up, position, velocity, **kw):
    """CalcContextParams (alc/alu.cpp:508-555): the rotation from AT and UP, the listener's velocity rotated by it"""
    n, v = _normalize32(at), _normalize32(up)
    u = _normalize32([n[1] * v[2] - n[2] * v[1], n[2] * v[0] - n[0] * v[2], n[0] * v[1] - n[1] * v[0]])
    rot = [u[0], v[0], -n[0], F32(0), u[1], v[1], -n[1], F32(0), u[2], v[2], -n[2], F32(0), F32(0), F32(0), F32(0), F32(1)]
    vel = [F32(x) for x in velocity] + [F32(0)]
    rv = [vel[0] * rot[0 * 4 + c] + vel[1] * rot[1 * 4 + c] + vel[2] * rot[2 * 4 + c] + vel[3] * rot[3 * 4 + c] for c in range(3)]
    return listener(matrix=[float(x) for x in rot], position=position, velocity=[float(x) for x in rv], **kw)


# listener 0: rotated, translated, moving, the distance model taken from the source; 1 + m: ContextParams{} with the context's
# distance model m
LISTENERS = [oriented_listener((0.3, -0.2, -1.0), (0.1, 1.0, 0.05), (1.5, -0.5, 2.0), (3.0, 0.0, -2.0), gain=0.9, meters_per_unit=1.25,
                               source_distance_model=1)] + [listener(distance_model=m) for m in range(7)]

# what CalcAttnVoiceParams reads of the effect slots (EffectSlotBase::RoomRolloff, DecayTime, AirAbsorptionGainHF), two sets
ENVIRONMENTS = [
    [dict(active=1, room_rolloff=0.3, decay_time=1.49, air_absorption_gain_hf=0.9943),
     dict(active=1, room_rolloff=0.0, decay_time=2.9, air_absorption_gain_hf=1.0)],
    [dict(active=1, room_rolloff=0.1, decay_time=0.0, air_absorption_gain_hf=0.98),
     dict(active=0, room_rolloff=0.5, decay_time=1.0, air_absorption_gain_hf=0.9)],
]

# a dry-line context (second-order 2D: W, Y, X, V, U) with two sends into two first-order slots; an HRTF context with one
DRY_CFG = dict(hrtf=False, sample_rate=48000, frequency=44100, num_dry=5, num_real=2, num_sends=2, num_slots=2, wet_channels=4,
               dry_map=([0, 1, 3, 4, 8], [1.0, 1.0, 1.0, 1.0, 1.0]), wet_map=([0, 1, 2, 3], [1.0, 1.0, 1.0, 1.0]))
HRTF_CFG = dict(hrtf=True, sample_rate=48000, frequency=44100, num_dry=4, num_real=2, num_sends=1, num_slots=1, wet_channels=4,
                dry_map=([0, 1, 2, 3], [1.0, 1.0, 1.0, 1.0]), wet_map=([0, 1, 2, 3], [1.0, 1.0, 1.0, 1.0]))


def source(**kw):
    """the defaults of a new AL source (al/source.cpp) in oalgpu_source_props' fields"""
    s = dict(pitch=1.0, gain=1.0, outer_gain=0.0, min_gain=0.0, max_gain=1.0, inner_angle=360.0, outer_angle=360.0,
             ref_distance=1.0, max_distance=FLT_MAX, rolloff_factor=1.0, position=[0.0, 0.0, -1.0], velocity=[0.0, 0.0, 0.0],
             direction=[0.0, 0.0, 0.0], head_relative=0, distance_model=INVERSE_CLAMPED, resampler=1, dry_gain_hf_auto=1,
             wet_gain_auto=1, wet_gain_hf_auto=1, outer_gain_hf=1.0, air_absorption_factor=0.0, room_rolloff_factor=0.0,
             doppler_factor=1.0, radius=0.0, direct=[1.0, 1.0, 5000.0, 1.0, 250.0],
             send=[[-1, 1.0, 1.0, 5000.0, 1.0, 250.0] for _ in range(MAX_SENDS)])
    s.update(kw)
    return s


def for_cfg(src, cfg):
    """the source with its send slots folded into the context's slots"""
    s = dict(src)
    s["send"] = [[(x[0] % cfg["num_slots"]) if x[0] >= 0 and cfg["num_slots"] else -1] + list(x[1:]) for x in src["send"]]
    return s


def props_struct(src):
    p = oalgpu.SourceProps()
    for k in ("pitch", "gain", "outer_gain", "min_gain", "max_gain", "inner_angle", "outer_angle", "ref_distance", "max_distance",
              "rolloff_factor", "head_relative", "distance_model", "resampler", "dry_gain_hf_auto", "wet_gain_auto", "wet_gain_hf_auto",
              "outer_gain_hf", "air_absorption_factor", "room_rolloff_factor", "doppler_factor", "radius"):
        setattr(p, k, src[k])
    for k in ("position", "velocity", "direction"):
        getattr(p, k)[:] = src[k]
    p.direct_gain, p.direct_gain_hf, p.direct_hf_reference, p.direct_gain_lf, p.direct_lf_reference = src["direct"]
    for i, s in enumerate(src["send"]):
        p.send[i].slot = int(s[0])
        p.send[i].gain, p.send[i].gain_hf, p.send[i].hf_reference, p.send[i].gain_lf, p.send[i].lf_reference = s[1:]
    return p


def props_array(sources):
    arr = (oalgpu.SourceProps * len(sources))()
    for i, s in enumerate(sources):
        arr[i] = props_struct(s)
    return arr


def listener_struct(lis):
    p = oalgpu.ListenerParams()
    p.matrix[:] = lis["matrix"]; p.position[:] = lis["position"]; p.velocity[:] = lis["velocity"]; p.xyz_scale[:] = lis["xyz_scale"]
    for k in ("gain", "meters_per_unit", "air_absorption_gain_hf", "doppler_factor", "speed_of_sound", "source_distance_model",
              "distance_model", "cone_scale", "nfc_scale"):
        setattr(p, k, lis[k])
    return p


def env_array(env, cfg):
    arr = (oalgpu.SlotEnvironment * cfg["num_slots"])()
    for i in range(cfg["num_slots"]):
        e = env[i]
        arr[i] = oalgpu.SlotEnvironment(e["active"], e["room_rolloff"], e["decay_time"], e["air_absorption_gain_hf"])
    return arr


def context_desc(cfg, max_voices=64, device=0, mode=oalgpu.MATH_FAST):
    return oalgpu.ContextDesc(device, mode, cfg["sample_rate"], cfg["num_dry"], cfg["num_real"], cfg["num_sends"], cfg["num_slots"],
                              cfg["wet_channels"], 1 if cfg["hrtf"] else 0, max_voices, 64, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
_BSINC = {}


def _bsinc_consts(family):
    if family not in _BSINC:
        t = oalgpu.Api().bsinc_table(family)
        _BSINC[family] = (F32(t["scaleBase"]), F32(t["scaleRange"]), list(t["m"]))
    return _BSINC[family]


def prepare_resampler(resampler, step, F=F32):
    """PrepareResampler / BsincPrepare (alc/alu.cpp:140-164, :253-281) -> (kind, scale index, sf)"""
    if resampler < 4:
        return (min(resampler, 2), -1, F(0.0))
    family = (12, 12, 24, 24, 48, 48)[resampler - 4]
    fast = resampler in (4, 6, 8)
    base, rng, _ = _bsinc_consts(family)
    si, sf = 15, F(0.0)
    if step > FRAC_ONE:
        sf = F(F32(FRAC_ONE)) / F(F32(step)) - F(base)
        sf = max(F(0.0), F(16.0) * sf * F(rng) - F(1.0))
        si = int(sf)
        sf = sf - F(si)
        sf = F(1.0) - np.sqrt(F(1.0) - sf * sf)
    return ((4 if (not fast and step > FRAC_ONE) else 3), si, sf)


def _design_shelf(high, f0norm, gain, F):
    """setParamsFromSlope(HighShelf | LowShelf, f0norm, gain, 1.0f) -> BiquadFilter::SetParams: b0, b1, b2, a1, a2 over a0"""
    one, two = F(1.0), F(2.0)
    gain = max(gain, F(F32(0.001)))
    rcpq = np.sqrt((gain + one / gain) * (one / F(1.0) - one) + two)
    gain = max(gain, F(F32(0.00001)))
    w0 = F(F32(np.pi)) * two * min(f0norm, F(F32(0.49)))
    sinw, cosw = np.sin(w0), np.cos(w0)
    alpha = sinw / two * rcpq
    sqrtgain_alpha_2 = two * np.sqrt(gain) * alpha
    if high:
        b0 = gain * ((gain + one) + (gain - one) * cosw + sqrtgain_alpha_2)
        b1 = -two * gain * ((gain - one) + (gain + one) * cosw)
        b2 = gain * ((gain + one) + (gain - one) * cosw - sqrtgain_alpha_2)
        a0 = (gain + one) - (gain - one) * cosw + sqrtgain_alpha_2
        a1 = two * ((gain - one) - (gain + one) * cosw)
        a2 = (gain + one) - (gain - one) * cosw - sqrtgain_alpha_2
    else:
        b0 = gain * ((gain + one) - (gain - one) * cosw + sqrtgain_alpha_2)
        b1 = two * gain * ((gain - one) - (gain + one) * cosw)
        b2 = gain * ((gain + one) - (gain - one) * cosw - sqrtgain_alpha_2)
        a0 = (gain + one) + (gain - one) * cosw + sqrtgain_alpha_2
        a1 = -two * ((gain - one) + (gain + one) * cosw)
        a2 = (gain + one) + (gain - one) * cosw - sqrtgain_alpha_2
    return [b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0]


def _ambi_coeffs(y, z, x, spread, F):
    """CalcAmbiCoeffs(y, z, x, spread), ACN 0..8 (core/ambidefs.h:219-245, core/mixer.cpp:16-69)"""
    c = lambda v: F(F32(v))
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    co = [F(1.0), c(1.7320508075688772) * y, c(1.7320508075688772) * z, c(1.7320508075688772) * x,
          c(3.872983346) * xy, c(3.872983346) * yz, c(1.118033989) * (F(3.0) * zz - F(1.0)), c(3.872983346) * xz,
          c(1.936491673) * (xx - yy)]
    if spread > F(0.0):
        ca = np.cos(spread * F(0.5))
        scale = np.sqrt(F(1.0) + c(0.31830988618379067154) * F(0.5) * spread)
        zh = [scale, scale * F(0.5) * (ca + F(1.0)), scale * F(0.5) * ((ca + F(1.0)) * ca)]
        co = [co[0] * zh[0]] + [v * zh[1] for v in co[1:4]] + [v * zh[2] for v in co[4:9]]
    return co


def calc(src, lis, env, cfg, F=F32, nudge=None):
    """CalcAttnVoiceParams + CalcPanningAndFilters of `src` under listener `lis` and slot environments `env` in context `cfg`.
    nudge: None, or a function (name, float32 value) -> float32 value applied to every float input."""
    def inp(name, v):
        v = F32(v)
        if nudge is not None:
            v = nudge(name, v)
        return F(v)
    c = lambda v: F(F32(v))
    zero, one = F(0.0), F(1.0)
    numsends = cfg["num_sends"]
    P = {k: inp(k, src[k]) for k in ("pitch", "gain", "outer_gain", "min_gain", "max_gain", "inner_angle", "outer_angle", "ref_distance",
                                     "max_distance", "rolloff_factor", "outer_gain_hf", "air_absorption_factor", "room_rolloff_factor",
                                     "doppler_factor", "radius")}
    pos = [inp("position%d" % i, v) for i, v in enumerate(src["position"])] + [one]
    vel = [inp("velocity%d" % i, v) for i, v in enumerate(src["velocity"])] + [zero]
    dirn = [inp("direction%d" % i, v) for i, v in enumerate(src["direction"])] + [zero]
    direct = [inp("direct%d" % i, v) for i, v in enumerate(src["direct"])]
    sends = [[s[0]] + [inp("send%d_%d" % (k, i), v) for i, v in enumerate(s[1:])] for k, s in enumerate(src["send"])]
    L = {k: inp("l_" + k, lis[k]) for k in ("gain", "meters_per_unit", "air_absorption_gain_hf", "doppler_factor", "speed_of_sound",
                                            "cone_scale", "nfc_scale")}
    M = [inp("l_m%d" % i, v) for i, v in enumerate(lis["matrix"])]
    lpos = [inp("l_p%d" % i, v) for i, v in enumerate(lis["position"])] + [one]
    lvel = [inp("l_v%d" % i, v) for i, v in enumerate(lis["velocity"])] + [zero]
    scale3 = [c(v) for v in lis["xyz_scale"]]
    branch = {}

    # alu.cpp:1721-1741
    sendslots = [-1] * MAX_SENDS
    roomrolloff = [zero] * MAX_SENDS
    for i in range(numsends):
        slot = sends[i][0]
        if slot >= 0 and env[slot]["active"]:
            sendslots[i] = slot
            roomrolloff[i] = P["room_rolloff_factor"] + inp("e_rr%d" % slot, env[slot]["room_rolloff"])

    def matvec(v):
        return [v[0] * M[0 * 4 + k] + v[1] * M[1 * 4 + k] + v[2] * M[2 * 4 + k] + v[3] * M[3 * 4 + k] for k in range(4)]

    def normalize(v):
        lsq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        if lsq > F(EPS):
            length = np.sqrt(lsq)
            inv = one / length
            return [v[0] * inv, v[1] * inv, v[2] * inv], length, True
        return [zero, zero, zero], zero, False

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    # :1743-1762
    if not src["head_relative"]:
        pos = matvec([pos[k] - lpos[k] for k in range(4)])
        vel = matvec(vel)
        dirn = matvec(dirn)
    else:
        vel = [vel[k] + lvel[k] for k in range(4)]
    tosource, distance, branch["has_distance"] = normalize(pos)
    dirn, dlen, branch["has_direction"] = normalize(dirn)
    directional = dlen > zero

    # :1764-1851
    model = src["distance_model"] if lis["source_distance_model"] else lis["distance_model"]
    ref, maxd, rolloff = P["ref_distance"], P["max_distance"], P["rolloff_factor"]
    atten = distance
    if model in (INVERSE_CLAMPED, LINEAR_CLAMPED, EXPONENT_CLAMPED):
        if not (ref <= maxd):
            atten = ref
            branch["clamp"] = "ref>max"
        else:
            atten = min(max(distance, ref), maxd)
            branch["clamp"] = "lo" if distance < ref else ("hi" if maxd < distance else "in")
    dry = [P["gain"], one, one]
    wet = [[P["gain"], one, one] for _ in range(MAX_SENDS)]
    dry_attn_base = one
    if model in (INVERSE, INVERSE_CLAMPED):
        if ref > zero:
            dist = ref + (atten - ref) * rolloff
            branch["inv_dry"] = bool(dist > zero)
            if dist > zero:
                dry_attn_base = ref / dist
                dry[0] = dry[0] * dry_attn_base
            for i in range(numsends):
                wdist = ref + (atten - ref) * roomrolloff[i]
                branch["inv_wet%d" % i] = bool(wdist > zero)
                if wdist > zero:
                    wet[i][0] = wet[i][0] * (ref / wdist)
    elif model in (LINEAR, LINEAR_CLAMPED):
        if maxd != ref:
            scale = (atten - ref) / (maxd - ref)
            a = one - scale * rolloff
            branch["lin_dry"] = bool(a < zero)
            dry_attn_base = max(a, zero)
            dry[0] = dry[0] * dry_attn_base
            for i in range(numsends):
                w = one - scale * roomrolloff[i]
                branch["lin_wet%d" % i] = bool(w < zero)
                wet[i][0] = wet[i][0] * max(w, zero)
    elif model in (EXPONENT, EXPONENT_CLAMPED):
        if atten > zero and ref > zero:
            ratio = atten / ref
            dry_attn_base = np.power(ratio, -rolloff)
            dry[0] = dry[0] * dry_attn_base
            for i in range(numsends):
                wet[i][0] = wet[i][0] * np.power(ratio, -roomrolloff[i])

    # :1853-1882
    wetcone, wetconehf = one, one
    branch["cone"] = 0
    if directional and P["inner_angle"] < c(360.0):
        rad2deg = c(180.0 / np.pi)
        angle = rad2deg * F(2.0) * np.arccos(-dot(dirn, tosource)) * L["cone_scale"]
        conegain, conehf = one, one
        if angle >= P["outer_angle"]:
            conegain, conehf = P["outer_gain"], P["outer_gain_hf"]
            branch["cone"] = 3
        elif angle >= P["inner_angle"]:
            scale = (angle - P["inner_angle"]) / (P["outer_angle"] - P["inner_angle"])
            conegain = one + (P["outer_gain"] - one) * scale
            conehf = one + (P["outer_gain_hf"] - one) * scale
            branch["cone"] = 2
        else:
            branch["cone"] = 1
        dry[0] = dry[0] * conegain
        if src["dry_gain_hf_auto"]:
            dry[1] = dry[1] * conehf
        if src["wet_gain_auto"]:
            wetcone = conegain
        if src["wet_gain_hf_auto"]:
            wetconehf = conehf

    # :1884-1903
    gain_mix_max = c(1000.0)
    mingain = min(P["min_gain"], P["max_gain"])
    maxgain = P["max_gain"]

    def clamp(v, lo, hi):
        return lo if v < lo else (hi if hi < v else v)
    branch["dry_clamp"] = -1 if dry[0] < mingain else (1 if maxgain < dry[0] else 0)
    dry[0] = clamp(dry[0], mingain, maxgain) * direct[0]
    branch["dry_ceiling"] = bool(dry[0] * L["gain"] > gain_mix_max)
    dry[0] = min(gain_mix_max, dry[0] * L["gain"])
    dry[1] = dry[1] * direct[1]
    dry[2] = direct[3]
    for i in range(numsends):
        g = clamp(wet[i][0] * wetcone, mingain, maxgain) * sends[i][1]
        wet[i] = [min(gain_mix_max, g * L["gain"]), sends[i][2] * wetconehf, sends[i][4]]

    # :1905-1954
    branch["beyond_ref"] = bool(distance > ref)
    if distance > ref:
        distance_units = (distance - ref) * rolloff
        distance_meters = distance_units * L["meters_per_unit"]
        absorb = distance_meters * P["air_absorption_factor"]
        branch["absorb"] = bool(absorb > F(EPS))
        if absorb > F(EPS):
            dry[1] = dry[1] * np.power(L["air_absorption_gain_hf"], absorb)
        if src["wet_gain_auto"]:
            for i in range(numsends):
                if sendslots[i] < 0:
                    continue
                e = env[sendslots[i]]
                decay_time = inp("e_dt%d" % sendslots[i], e["decay_time"])
                if not (decay_time > zero):
                    continue
                slot_absorb = inp("e_aa%d" % sendslots[i], e["air_absorption_gain_hf"])
                if slot_absorb < one and absorb > F(EPS):
                    wet[i][1] = wet[i][1] * np.power(slot_absorb, absorb)
                decay_distance = decay_time * c(343.3)
                fact = distance_meters / decay_distance
                g = np.power(c(0.001), fact) * (one - dry_attn_base) + dry_attn_base
                wet[i][0] = wet[i][0] * g

    # :1957-1999
    pitch = P["pitch"]
    doppler = P["doppler_factor"] * L["doppler_factor"]
    branch["doppler"] = 0
    if doppler > zero:
        vss = dot(vel, tosource) * -doppler
        vls = dot(lvel, tosource) * -doppler
        sos = L["speed_of_sound"]
        if not (vls < sos):
            pitch = zero
            branch["doppler"] = 1
        elif not (vss < sos):
            pitch = F(np.inf)
            branch["doppler"] = 2
        else:
            pitch = pitch * ((sos - vls) / (sos - vss))
            branch["doppler"] = 3
    pitch = pitch * (F(F32(cfg["frequency"])) / F(F32(cfg["sample_rate"])))
    if pitch > c(10.0):
        step = 10 << 16
    else:
        step = max(int(np.rint(np.float64(pitch * c(65536.0)))), 1)      # fastf2u: to nearest even
    rs_kind, rs_si, rs_sf = prepare_resampler(src["resampler"], step, F)

    # :2002-2006
    spread = zero
    pi = c(np.pi)
    branch["spread"] = 0
    if P["radius"] > distance:
        spread = pi * F(2.0) - distance / P["radius"] * pi
        branch["spread"] = 1
    elif distance > zero:
        spread = np.arcsin(P["radius"] / distance) * F(2.0)
        branch["spread"] = 2

    # CalcPanningAndFilters for FmtMono, !mPanningEnabled: CalcHrtfPanning :1207-1227 / :1272-1310, CalcNormalPanning :1343-1362 /
    # :1413-1465 with MonoMap (:1471-1473)
    if distance > F(EPS):
        d3 = [tosource[k] * scale3[k] for k in range(3)]
        hrtf_dist = distance * L["nfc_scale"]
    else:
        d3 = [zero, zero, -one]
        hrtf_dist = F(np.inf)
    ev = np.arcsin(clamp(d3[1], -one, one)) if cfg["hrtf"] else zero
    az = np.arctan2(d3[0], -d3[2]) if cfg["hrtf"] else zero
    co = _ambi_coeffs(-d3[0], d3[1], -d3[2], spread, F)
    acn = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8}
    dry_gains = [zero] * 32
    if not cfg["hrtf"]:
        for t, (idx, sc) in enumerate(zip(*cfg["dry_map"])):
            dry_gains[t] = c(sc) * co[acn[idx]] * dry[0]
    send_gains = [[zero] * 25 for _ in range(MAX_SENDS)]
    for i in range(numsends):
        if sendslots[i] >= 0:
            for t, (idx, sc) in enumerate(zip(*cfg["wet_map"])):
                send_gains[i][t] = c(sc) * co[acn[idx]] * wet[i][0]

    # :1619-1656
    inv_rate = one / F(F32(cfg["sample_rate"]))
    coeffs = [_design_shelf(True, direct[2] * inv_rate, dry[1], F), _design_shelf(False, direct[4] * inv_rate, dry[2], F)]
    coeffs += [_design_shelf(True, sends[i][3] * inv_rate, wet[i][1], F) for i in range(numsends)]
    coeffs += [_design_shelf(False, sends[i][5] * inv_rate, wet[i][2], F) for i in range(numsends)]
    active = [bool(dry[1] != one or dry[2] != one)] + [bool(wet[i][1] != one or wet[i][2] != one) for i in range(numsends)]
    return dict(step=step, rs=(rs_kind, rs_si), rs_sf=rs_sf, send_slot=sendslots, filter_active=active, dry=dry, wet=wet[:numsends],
                distance=distance, spread=spread, dir=d3, ev=ev, az=az, hrtf_dist=hrtf_dist, dry_gains=dry_gains,
                send_gains=send_gains, coeffs=coeffs, branch=branch,
                hf_norm=[direct[2] * inv_rate] + [sends[i][3] * inv_rate for i in range(numsends)],
                lf_norm=[direct[4] * inv_rate] + [sends[i][5] * inv_rate for i in range(numsends)])


def voice_params(r, src, cfg):
    """the restatement's results as an oalgpu_voice_params + the (dir, spread, dry_gain, send_gain) row of oalgpu_voice_set_pan"""
    p = oalgpu.VoiceParams()
    p.step = r["step"]
    p.resampler = src["resampler"]
    p.direct_filter = oalgpu.FilterParams(int(r["filter_active"][0]), float(r["dry"][1]), float(r["hf_norm"][0]), float(r["dry"][2]),
                                          float(r["lf_norm"][0]))
    p.dry_gains[:] = [float(x) for x in r["dry_gains"]]
    p.hrtf_ev, p.hrtf_az, p.hrtf_dist, p.hrtf_spread = float(r["ev"]), float(r["az"]), float(r["hrtf_dist"]), float(r["spread"])
    p.hrtf_gain = float(r["dry"][0])
    for i in range(MAX_SENDS):
        p.send_slot[i] = r["send_slot"][i]
    for i in range(cfg["num_sends"]):
        p.send_filter[i] = oalgpu.FilterParams(int(r["filter_active"][1 + i]), float(r["wet"][i][1]), float(r["hf_norm"][1 + i]),
                                               float(r["wet"][i][2]), float(r["lf_norm"][1 + i]))
        p.send_gains[i][:] = [float(x) for x in r["send_gains"][i]]
    pan = [float(x) for x in r["dir"]] + [float(r["spread"]), float(r["dry"][0])] + [float(r["wet"][i][0]) if i < cfg["num_sends"] else 0.0
                                                                                      for i in range(MAX_SENDS)]
    return p, pan


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def _ulp_nudge(k, sign_of):
    def nudge(name, v):
        s = sign_of(name)
        # (0 and 1 stay: they are the neutral values whose exactness IS the input -- an HF gain of exactly 1 means no filter)
        if not np.isfinite(v) or v == 0 or abs(v) == 1 or s == 0:
            return v
        for _ in range(k):
            v = np.nextafter(v, F32(np.inf) if s > 0 else F32(-np.inf))
        return v
    return nudge


def integer_results(r, mhr=None, cfg=None):
    """what must not move under a +-4 ulp nudge of the inputs: the branches and the integer results"""
    out = dict(r["branch"])
    out.update(step=r["step"], rs=r["rs"], active=tuple(r["filter_active"]), slots=tuple(r["send_slot"]))
    if mhr is not None and cfg["hrtf"]:
        out["hrir"] = hrir_blend(mhr, cfg, r)[0:2]
    return out


def hrir_blend(mhr, cfg, r):
    """HrtfStore::getCoeffs' index half (core/hrtf.cpp:192-245) for the restatement's direction: (indices, delays, weights)"""
    vp = C.c_void_p
    oalgpu.lib.oalgpu_hrtf_blend_host.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp]
    dirs = np.array([r["ev"], r["az"], r["hrtf_dist"], r["spread"]], np.float32)
    idx, w, ps, de = np.zeros(4, np.uint32), np.zeros(4, np.float32), np.zeros(1, np.float32), np.zeros(2, np.uint32)
    rc = oalgpu.lib.oalgpu_hrtf_blend_host(mhr, len(mhr), cfg["sample_rate"], dirs.ctypes.data_as(vp), 1, idx.ctypes.data_as(vp),
                                           w.ctypes.data_as(vp), ps.ctypes.data_as(vp), de.ctypes.data_as(vp))
    assert rc == 0
    return tuple(int(x) for x in idx), tuple(int(x) for x in de), w


def _unit(lcg):
    while True:
        v = [lcg.uniform(-1.0, 1.0) for _ in range(3)]
        n = float(np.sqrt(sum(x * x for x in v)))
        if 0.2 < n <= 1.0:
            return [x / n for x in v]


def _base(lcg, k):
    """a plain random source: somewhere 0.3 .. 9 units away, filtered now and then, with one or two sends"""
    d = _unit(lcg)
    r = lcg.uniform(0.3, 9.0)
    s = source(position=[d[0] * r, d[1] * r, d[2] * r], gain=lcg.uniform(0.05, 1.0), pitch=lcg.uniform(0.6, 1.6), resampler=k % 10,
               distance_model=1 + k % 6, rolloff_factor=lcg.uniform(0.3, 2.0), ref_distance=lcg.uniform(0.5, 2.0),
               max_distance=lcg.uniform(4.0, 12.0), room_rolloff_factor=lcg.uniform(0.0, 0.5))
    s["direct"] = [lcg.uniform(0.5, 1.0), 1.0 if k % 3 == 0 else lcg.uniform(0.2, 0.95), 5000.0, 1.0 if k % 4 else lcg.uniform(0.3, 0.9), 250.0]
    s["send"][0] = [k % 2, lcg.uniform(0.3, 1.0), 1.0 if k % 5 else lcg.uniform(0.3, 0.9), 5000.0, 1.0, 250.0]
    s["send"][1] = [(-1, 0, 1)[k % 3], lcg.uniform(0.3, 1.0), 1.0, 4000.0, 1.0 if k % 7 else 0.6, 300.0]
    return s


def _cone(lcg, s, lis, where):
    """points the source's cone so that the angle to the listener lands inside / between / outside the cone's angles"""
    s["inner_angle"], s["outer_angle"] = 60.0, 200.0
    s["outer_gain"], s["outer_gain_hf"] = lcg.uniform(0.05, 0.6), 1.0
    # the direction from the source to the listener, in world space, turned by a known angle (|cos| <= 0.99 keeps acos well conditioned)
    to_listener = np.array(lis["position"]) - np.array(s["position"]) if not s["head_relative"] else -np.array(s["position"])
    to_listener = to_listener / np.linalg.norm(to_listener)
    half = {"inside": lcg.uniform(8.1, 25.0), "between": lcg.uniform(40.0, 90.0), "outside": lcg.uniform(110.0, 171.0)}[where]
    other = np.cross(to_listener, np.array(_unit(lcg)))
    other = other / np.linalg.norm(other)
    d = np.cos(np.radians(half)) * to_listener + np.sin(np.radians(half)) * other
    s["direction"] = [float(x) * 1.7 for x in d]
    return s


def _build():
    lcg = synth.Lcg(0x5EED0051)
    cases = []

    def add(tag, lis, env, s):
        cases.append(dict(tag=tag, lis=lis, env=env, src=s))
    k = 0
    for rep in range(8):
        for m in range(7):                                  # every distance model, from the source and from the context
            k += 1; s = _base(lcg, k); s["distance_model"] = m
            add("model%d_source" % m, 0, rep % 2, s)
            k += 1; s = _base(lcg, k); s["distance_model"] = (m + 3) % 7
            add("model%d_context" % m, 1 + m, rep % 2, s)
        for m in (INVERSE_CLAMPED, LINEAR_CLAMPED, EXPONENT_CLAMPED):
            k += 1; s = _base(lcg, k); s["distance_model"] = m; s["ref_distance"], s["max_distance"] = 5.0, 2.0
            add("ref_gt_max", 0, rep % 2, s)
        k += 1; s = _base(lcg, k); s["ref_distance"] = 0.0; s["distance_model"] = (INVERSE, EXPONENT, LINEAR, INVERSE_CLAMPED)[rep % 4]
        add("ref_zero", 0, rep % 2, s)
        for where, scale in (("below_ref", 0.5), ("at_ref", 1.0), ("beyond_max", 1.0)):
            k += 1; s = _base(lcg, k); s["head_relative"] = 1; s["distance_model"] = (INVERSE_CLAMPED, LINEAR_CLAMPED, EXPONENT_CLAMPED)[rep % 3]
            d = _unit(lcg)
            s["ref_distance"], s["max_distance"] = 2.0, 6.0
            r = {"below_ref": 1.0, "at_ref": 2.0, "beyond_max": 7.5}[where]
            s["position"] = [d[0] * r, d[1] * r, d[2] * r]
            if where == "at_ref":                           # exactly at RefDistance: on an axis, so that the norm is exact
                s["position"] = [[2.0, 0.0, 0.0], [0.0, -2.0, 0.0], [0.0, 0.0, 2.0]][rep % 3]
            add(where, 0, rep % 2, s)
        k += 1; s = _base(lcg, k); s["distance_model"] = (LINEAR, LINEAR_CLAMPED)[rep % 2]; s["max_distance"] = s["ref_distance"] = 3.0
        add("linear_max_eq_ref", 0, rep % 2, s)
        k += 1; s = _base(lcg, k); s["rolloff_factor"] = 0.0
        add("rolloff_zero", 0, rep % 2, s)
        for where in ("inside", "between", "outside"):
            for off in (None, "dry_gain_hf_auto", "wet_gain_auto", "wet_gain_hf_auto"):
                if off is not None and rep >= 3 and where != "between":
                    continue
                k += 1; s = _base(lcg, k); s["head_relative"] = rep % 2
                s = _cone(lcg, s, LISTENERS[0], where)
                s["outer_gain_hf"] = lcg.uniform(0.2, 0.9)
                if off:
                    s[off] = 0
                add("cone_" + where + ("" if off is None else "_no_" + off), 0, rep % 2, s)
        for what in ("nominal", "vls", "vss", "factor_zero"):
            k += 1; s = _base(lcg, k); s["head_relative"] = rep % 2
            v = _unit(lcg)
            s["velocity"] = [x * lcg.uniform(5.0, 60.0) for x in v]
            lis = 0
            if what == "factor_zero":
                s["doppler_factor"] = 0.0
            if what == "vss":                               # the source races towards the listener
                tl = -np.array(s["position"]) if s["head_relative"] else np.array(LISTENERS[0]["position"]) - np.array(s["position"])
                tl = tl / np.linalg.norm(tl)
                s["velocity"] = [float(x) * 800.0 for x in tl]; s["doppler_factor"] = 1.0
                if s["head_relative"]:
                    s["velocity"] = [float(x) * 800.0 for x in tl]
            if what == "vls":                               # the listener races away from the source: a listener of its own
                lis = 8
                s["head_relative"] = 0; s["position"] = [0.0, 0.0, -lcg.uniform(2.0, 5.0)]
            add("doppler_" + what, lis, rep % 2, s)
        for on in (0, 1):
            k += 1; s = _base(lcg, k); s["head_relative"] = on
            add("head_relative_%d" % on, 0, rep % 2, s)
        for f in (0.0, 0.7, 3.0):
            k += 1; s = _base(lcg, k); s["air_absorption_factor"] = f; s["send"][0][0] = rep % 2; s["send"][1][0] = 1 - rep % 2
            r = lcg.uniform(1.2, 4.0) * s["ref_distance"]; d = _unit(lcg); s["head_relative"] = 1
            s["position"] = [d[0] * r, d[1] * r, d[2] * r]
            add("air_absorption_%g" % f, 0, rep % 2, s)
        k += 1; s = _base(lcg, k); s["wet_gain_auto"] = 0; s["air_absorption_factor"] = 1.0
        add("wet_gain_auto_off", 0, 0, s)
        k += 1; s = _base(lcg, k); s["send"][0][0] = 0; s["air_absorption_factor"] = 0.5
        add("decay_time_zero", 0, 1, s)
        for what in ("zero", "below", "above"):
            k += 1; s = _base(lcg, k)
            dist = float(np.linalg.norm(np.array(s["position"]) - np.array(LISTENERS[0]["position"])))
            s["radius"] = {"zero": 0.0, "below": dist * lcg.uniform(0.1, 0.8), "above": dist * lcg.uniform(1.2, 3.0)}[what]
            add("radius_" + what, 0, rep % 2, s)
        k += 1; s = _base(lcg, k)
        if rep % 2:
            s["head_relative"] = 1; s["position"] = [0.0, 0.0, 0.0]
        else:
            s["position"] = list(LISTENERS[0]["position"])
        s["radius"] = (0.0, 0.0, 1.5, 1.5)[rep % 4]
        add("at_listener", 0, rep % 2, s)
        k += 1; s = _base(lcg, k); s["min_gain"], s["max_gain"] = 0.8, 0.3
        add("min_gt_max", 0, rep % 2, s)
        k += 1; s = _base(lcg, k); s["gain"] = lcg.uniform(1.5, 4.0); s["max_gain"] = lcg.uniform(0.5, 1.0)
        s["head_relative"] = 1; s["position"] = [0.0, 0.3, -0.4]; s["distance_model"] = INVERSE_CLAMPED
        add("above_max_gain", 0, rep % 2, s)
        k += 1; s = _base(lcg, k); s["gain"] = lcg.uniform(30.0, 60.0); s["max_gain"] = 100.0; s["direct"][0] = 40.0; s["send"][0][1] = 35.0
        s["head_relative"] = 1; s["position"] = [0.0, 0.0, -0.5]; s["distance_model"] = DISABLE
        add("gain_mix_max", 0, rep % 2, s)
        for rsm in range(10):                               # every resampler, the step below / at / above one and above MaxPitch
            what = ("below", "at", "above", "max_pitch")[(rsm + rep) % 4]
            k += 1; s = _base(lcg, k); s["resampler"] = rsm; s["doppler_factor"] = 0.0
            s["pitch"] = {"below": lcg.uniform(0.3, 0.95) * 48000.0 / 44100.0, "at": 48000.0 / 44100.0,
                          "above": lcg.uniform(1.1, 6.0) * 48000.0 / 44100.0, "max_pitch": lcg.uniform(11.0, 14.0)}[what]
            add("resampler%d_%s" % (rsm, what), 0, rep % 2, s)
    return cases


# listener 8: moving away from anything in front of it faster than sound
LISTENERS.append(listener(velocity=(0.0, 0.0, 400.0), source_distance_model=1))

_TABLE = None


def table(mhr=None):
    """-> (kept cases, dropped cases).  mhr (bytes of the golden data set) adds the HRIR indices and delays to what a nudge must
    not move; without it (no data set at hand) the table is the same minus that test."""
    global _TABLE
    if _TABLE is not None and _TABLE[2] == (mhr is not None):
        return _TABLE[0], _TABLE[1]
    kept, dropped = [], []
    # every input up, every input down (mixed signs would take apart the cases that sit ON a boundary by construction --
    # distance == RefDistance, MaxDistance == RefDistance -- which equal nudges of both sides keep there)
    patterns = [lambda name: 1, lambda name: -1]
    for case in _build():
        stable = True
        for cfg in (DRY_CFG, HRTF_CFG):
            src = for_cfg(case["src"], cfg)
            lis, env = LISTENERS[case["lis"]], ENVIRONMENTS[case["env"]]
            want = integer_results(calc(src, lis, env, cfg), mhr, cfg)
            for sign_of in patterns:
                got = integer_results(calc(src, lis, env, cfg, nudge=_ulp_nudge(4, sign_of)), mhr, cfg)
                if got != want:
                    stable = False
                    break
            if not stable:
                break
        (kept if stable else dropped).append(case)
    _TABLE = (kept, dropped, mhr is not None)
    return kept, dropped


def measure_noise(cases):
    """the largest disagreement between the float32 and the float64 evaluation of the restatement, per output class"""
    noise = {k: 0.0 for k in NOISE}

    def rel(a, b, floor):
        a, b = float(a), float(b)
        if not np.isfinite(b):
            return 0.0
        return abs(a - b) / max(abs(b), floor)
    for case in cases:
        for cfg in (DRY_CFG, HRTF_CFG):
            src = for_cfg(case["src"], cfg)
            lis, env = LISTENERS[case["lis"]], ENVIRONMENTS[case["env"]]
            a, b = calc(src, lis, env, cfg, F32), calc(src, lis, env, cfg, np.float64)
            for x, y in [(a["dry"][0], b["dry"][0])] + [(a["wet"][i][0], b["wet"][i][0]) for i in range(cfg["num_sends"])]:
                noise["gain"] = max(noise["gain"], rel(x, y, 1e-3))
            for x, y in [(a["dry"][1], b["dry"][1])] + [(a["wet"][i][1], b["wet"][i][1]) for i in range(cfg["num_sends"])]:
                noise["gain_hf"] = max(noise["gain_hf"], rel(x, y, 1e-3))
            for x, y in ((a["ev"], b["ev"]), (a["az"], b["az"]), (a["spread"], b["spread"])):
                noise["angle"] = max(noise["angle"], abs(float(x) - float(y)) / np.pi)
            for x, y in zip(a["dry_gains"] + sum(a["send_gains"], []), b["dry_gains"] + sum(b["send_gains"], [])):
                noise["pan"] = max(noise["pan"], rel(x, y, max(1e-3, float(b["dry"][0]), *[float(w[0]) for w in b["wet"]])))
            for ca, cb in zip(a["coeffs"], b["coeffs"]):
                for x, y in zip(ca, cb):
                    noise["coeff"] = max(noise["coeff"], rel(x, y, 1.0))
    return noise


def check_voice_params(vp, r, cfg, who=""):
    """an oalgpu_voice_params (oalgpu_source_params_host) against the restatement's results `r`: integers exact, floats within
    TOLERANCE of their class"""
    ns = cfg["num_sends"]
    assert vp.step == r["step"], (who, vp.step, r["step"])
    assert [vp.send_slot[i] for i in range(MAX_SENDS)] == list(r["send_slot"]), who
    assert [vp.direct_filter.active] + [vp.send_filter[i].active for i in range(ns)] == [int(a) for a in r["filter_active"]], who

    def close(x, y, tol, floor, what):
        x, y = float(x), float(y)
        if not np.isfinite(y):
            assert x == y, (who, what, x, y)
            return
        assert abs(x - y) <= tol * max(abs(y), floor), (who, what, x, y, abs(x - y) / max(abs(y), floor), tol)
    close(vp.hrtf_gain, r["dry"][0], TOLERANCE["gain"], 1e-3, "dry base")
    close(vp.direct_filter.gain_hf, r["dry"][1], TOLERANCE["gain_hf"], 1e-3, "dry hf")
    assert vp.direct_filter.gain_lf == float(r["dry"][2]) and vp.direct_filter.hf_norm == float(r["hf_norm"][0]), who
    assert vp.direct_filter.lf_norm == float(r["lf_norm"][0]), who
    top = max([1e-3, float(r["dry"][0])] + [float(w[0]) for w in r["wet"]])
    for i in range(ns):
        close(vp.send_filter[i].gain_hf, r["wet"][i][1], TOLERANCE["gain_hf"], 1e-3, "wet hf")
        assert vp.send_filter[i].gain_lf == float(r["wet"][i][2]), who
        for t in range(25):
            close(vp.send_gains[i][t], r["send_gains"][i][t], TOLERANCE["pan"], top, "send gain")
    for t in range(32):
        close(vp.dry_gains[t], r["dry_gains"][t], TOLERANCE["pan"], top, "dry gain")
    if cfg["hrtf"]:
        for x, y, what in ((vp.hrtf_ev, r["ev"], "ev"), (vp.hrtf_az, r["az"], "az"), (vp.hrtf_spread, r["spread"], "spread")):
            assert abs(float(x) - float(y)) <= TOLERANCE["angle"] * np.pi, (who, what, x, y)
        close(vp.hrtf_dist, r["hrtf_dist"], 2.0 ** -22, 1e-3, "hrtf distance")
