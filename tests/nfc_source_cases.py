"""Cases and the reference side of the near-field half of the source stage (SourceNfcKernel, oalgpu_channel_source_nfc_host):
the w0 CalcNormalPanning hands to NfcFilter::adjust on a device with AvgSpeakerDist > 0 (alc/alu.cpp:1325-1341, :1413-1428)
and what adjust leaves (core/filters/nfc.cpp:56-219).

* distance(), w0(), adjust(): an op-for-op numpy restatement, every operation one numpy scalar operation of the chosen type
  (float32: the reference's arithmetic).  Written from the reference's sources -- the four orders as nfc.cpp has them, a
  first-order section as g_0 = 1 + b_00, not as a second-order one with a zero -- and independent of csrc/dev_source_nfc.hpp
  and csrc/dev_nfc_design.hpp.  The distance is the one CalcPanningAndFilters receives: on CalcAttnVoiceParams' route the norm
  of the source's position in listener space (subtractions, the matrix product's multiplications and additions, a square root:
  common/vecmat.h:51-65, :112-120), on CalcNonAttnVoiceParams' route 0.  Only + - * / sqrt max and comparisons lie between a
  case's inputs and its fourteen coefficients, all correctly rounded in IEEE arithmetic, so the comparison is bit for bit.
* CASES: every branch -- the identity filter of a source at the listener, the AvgSpeakerDist / 4 clamp, ordinary distances,
  head-relative and world positions under a rotated and translated listener, NfcScale other than 1, the non-attenuated
  route (spatialize OFF; AUTO with a stereo source), a 5.1 source with an LFE voice, a source with OALGPU_NO_VOICE channels.
"""
import numpy as np

import channel_source_cases as cc
import oalgpu
import source_param_cases as sc

F32 = np.float32
EPS = F32(1.1920928955078125e-07)
SPEED_OF_SOUND = F32(343.3)
AVG_SPEAKER_DIST = 1.5
NO_VOICE = oalgpu.NO_VOICE

ROTATED = sc.LISTENERS[0]                                   # rotated, translated, moving
PLAIN = sc.listener()
SCALED = sc.listener(nfc_scale=0.25)
ROTATED_SCALED = dict(ROTATED, nfc_scale=2.5)
LISTENERS = {"plain": PLAIN, "rotated": ROTATED, "scaled": SCALED, "rotated_scaled": ROTATED_SCALED}


def distance(cs, lis, F=F32):
    """the distance CalcPanningAndFilters receives for channel source `cs` under listener `lis`"""
    if not cc.attenuated(cs):
        return F(0.0)                                       # CalcNonAttnVoiceParams: CalcPanningAndFilters(0, 0, -1, 0, 0, ...)
    src = cs["src"]
    pos = [F(F32(v)) for v in src["position"]] + [F(1.0)]
    if not src["head_relative"]:
        M = [F(F32(v)) for v in lis["matrix"]]
        lpos = [F(F32(v)) for v in lis["position"]] + [F(1.0)]
        rel = [pos[k] - lpos[k] for k in range(4)]
        pos = [rel[0] * M[0 * 4 + k] + rel[1] * M[1 * 4 + k] + rel[2] * M[2 * 4 + k] + rel[3] * M[3 * 4 + k] for k in range(4)]
    lsq = pos[0] * pos[0] + pos[1] * pos[1] + pos[2] * pos[2]
    return np.sqrt(lsq) if lsq > F(EPS) else F(0.0)         # al::Vector::normalize


def w0(dist, lis, avg, rate, F=F32):
    """-> (w0, branch): 'identity' (:1423), 'clamp' (max() took AvgSpeakerDist / 4) or 'distance'"""
    avg, samplerate = F(F32(avg)), F(F32(rate))
    if dist > F(EPS):
        scaled, least = dist * F(F32(lis["nfc_scale"])), avg / F(4.0)
        mdist = max(scaled, least)
        return F(SPEED_OF_SOUND) / (mdist * samplerate), ("clamp" if scaled < least else "distance")
    return F(SPEED_OF_SOUND) / (avg * samplerate), "identity"


def _sections(w, F):
    """NfcFilterCreateN / NfcFilterAdjustN at w: per order (its gain factor, [coefficients 1..o])"""
    r = F(0.5) * w
    c = lambda v: F(F32(v))
    one, two, four = F(1.0), F(2.0), F(4.0)
    out = {}
    b_00 = c(1.0) * r; g_0 = one + b_00
    out[1] = (g_0, [two * b_00 / g_0])
    b_10 = c(3.0) * r; b_11 = c(3.0) * (r * r); g_1 = one + b_10 + b_11
    out[2] = (g_1, [(two * b_10 + four * b_11) / g_1, four * b_11 / g_1])
    b_10 = c(3.6778) * r; b_11 = c(6.4595) * (r * r); b_00 = c(2.3222) * r; g_1 = one + b_10 + b_11; g_0 = one + b_00
    out[3] = (g_1 * g_0, [(two * b_10 + four * b_11) / g_1, four * b_11 / g_1, two * b_00 / g_0])
    b_10 = c(4.2076) * r; b_11 = c(11.4877) * (r * r); b_00 = c(5.7924) * r; b_01 = c(9.1401) * (r * r)
    g_1 = one + b_10 + b_11; g_0 = one + b_00 + b_01
    out[4] = (g_1 * g_0, [(two * b_10 + four * b_11) / g_1, four * b_11 / g_1, (two * b_00 + four * b_01) / g_0, four * b_01 / g_0])
    return out


def adjust(w1, w, F=F32):
    """NfcFilter::init(w1) then adjust(w) -> the 14 coefficients: a0 of the orders 1..4, then b1; b1 b2; b1 b2 b3; b1 b2 b3 b4"""
    init, adj = _sections(F(w1), F), _sections(F(w), F)
    a0 = [(F(1.0) / init[o][0]) * adj[o][0] for o in (1, 2, 3, 4)]
    b = [x for o in (1, 2, 3, 4) for x in adj[o][1]]
    return np.array(a0 + b, F)


def device_w1(avg, rate, F=F32):
    """InitNearFieldCtrl (alc/panning.cpp:285-299)"""
    return F(SPEED_OF_SOUND) / F(F32(avg)) / F(F32(rate))


def expected(cs, lis, avg=AVG_SPEAKER_DIST, rate=48000, F=F32):
    """-> (w0, the 14 coefficients, branch) of every channel voice of `cs`"""
    w, branch = w0(distance(cs, lis, F), lis, avg, rate, F)
    return w, adjust(device_w1(avg, rate, F), w, F), branch


def _src(position, head_relative=0, **kw):
    return sc.source(position=list(position), head_relative=head_relative, **kw)


# (tag, listener, channel source, the voices a GPU test gives it -- None: one per channel, or the channels left without a voice)
CASES = [
    ("at_listener_head_relative", "plain", cc.channel_source(_src((0.0, 0.0, 0.0), 1), cc.MONO, cc.ON), None),
    ("at_listener_world", "rotated", cc.channel_source(_src(ROTATED["position"]), cc.MONO, cc.AUTO), None),
    ("within_quarter_distance", "plain", cc.channel_source(_src((0.1, 0.05, -0.2)), cc.MONO, cc.ON), None),
    ("on_the_clamp_side_scaled", "scaled", cc.channel_source(_src((0.0, 0.0, -1.25)), cc.MONO, cc.ON), None),
    ("ordinary", "plain", cc.channel_source(_src((2.0, 0.5, -3.0)), cc.MONO, cc.AUTO), None),
    ("ordinary_head_relative_rotated", "rotated", cc.channel_source(_src((1.0, -0.25, 4.0), 1), cc.MONO, cc.ON), None),
    ("world_rotated", "rotated", cc.channel_source(_src((-3.5, 1.0, 0.75)), cc.MONO, cc.AUTO), None),
    ("nfc_scale_up", "rotated_scaled", cc.channel_source(_src((0.5, 0.25, 1.0)), cc.STEREO, cc.ON), None),
    ("nfc_scale_down", "scaled", cc.channel_source(_src((6.0, 0.0, -8.0)), cc.MONO, cc.ON), None),
    ("stereo_off", "rotated", cc.channel_source(_src((5.0, 0.0, -2.0)), cc.STEREO, cc.OFF), None),
    ("stereo_auto", "plain", cc.channel_source(_src((5.0, 0.0, -2.0)), cc.STEREO, cc.AUTO), None),
    ("mono_off", "plain", cc.channel_source(_src((0.0, 3.0, 0.0)), cc.MONO, cc.OFF), None),
    ("x51_with_lfe", "rotated", cc.channel_source(_src((0.0, 2.0, -2.5)), cc.X51, cc.ON), None),
    ("x71_without_lfe_and_rears", "plain", cc.channel_source(_src((-1.0, 0.0, -0.5)), cc.X71, cc.ON), (3, 4, 5)),
    ("quad_near", "plain", cc.channel_source(_src((0.0, 0.0, -0.3)), cc.QUAD, cc.ON), None),
]
