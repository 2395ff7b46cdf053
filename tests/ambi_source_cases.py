"""Cases and the reference side of the parameter stage for B-Format sources (oalgpu_voice_set_ambi_sources, AmbiParamsKernel,
oalgpu_ambi_source_params_host), on top of source_param_cases and channel_source_cases.

* calc(): a numpy restatement, from the reference's sources and independent of csrc/dev_source_ambi.hpp, of CalcAmbisonicPanning
  (alc/alu.cpp:911-1076) with AmbiRotator (:799-888, its constants as RotatorCoeffs computes them, :738-792) and
  UpsampleBFormatTransform (:457-477); the route's gains, distance, spread, direction, step and filters are
  source_param_cases.calc's (spatialize ON) or channel_source_cases' CalcNonAttnVoiceParams (OFF, AUTO).  One numpy scalar
  operation of the chosen type per operation of the reference.  The layout and scaling tables and the upsamplers are the
  fixture's (tests/golden/ambi_tables.npz: what the compiled reference holds).
* table(): eleven groups (GROUPS) x spatialize OFF / AUTO / ON x 0 / 1 / 2 sends.  As in source_param_cases a case is dropped if
  the restatement changes a branch or an integer result under a +-4 ulp nudge of every float input.
* What must match (tests/test_ambi_sources_host.py): the mix matrix bit for bit on every route; every line gain bit for bit on
  the OFF / AUTO route; on the ON route the gain classes within channel_source_cases.TOLERANCE.
* ROTATOR_NOISE / ROTATOR_TOLERANCE: the float32 restatement of the rotator against the float64 restatement of the same
  recurrence, largest absolute difference of a matrix entry over the table's orientations at order 4 (entries are <= 1 in
  magnitude), and 8 x that figure (DESIGN 3.25's rule), rounded up to two digits.  test_ambi_sources_host.py asserts that the
  measurement still gives the figure."""
import os

import numpy as np

import channel_source_cases as cc
import oalgpu
import source_param_cases as sc
from oalgpu import synth

F32 = np.float32
OFF, ON, AUTO = cc.OFF, cc.ON, cc.AUTO
FUMA, ACN = 0, 1
S_FUMA, S_SN3D, S_N3D = 0, 1, 2
NO_VOICE = oalgpu.NO_VOICE
HERE = os.path.dirname(os.path.abspath(__file__))
TABLES = np.load(os.path.join(HERE, "golden", "ambi_tables.npz"))
SCALES = {S_FUMA: TABLES["FromFuMa"], S_SN3D: TABLES["FromSN3D"], S_N3D: TABLES["FromN3D"]}
INDEX = {(FUMA, False): TABLES["IndexFromFuMa"], (FUMA, True): TABLES["IndexFromFuMa2D"], (ACN, False): TABLES["IndexFromACN"],
         (ACN, True): TABLES["IndexFromACN2D"]}
UPSAMPLERS = {(1, False): TABLES["FirstOrderUp"], (1, True): TABLES["FirstOrder2DUp"], (2, False): TABLES["SecondOrderUp"],
              (2, True): TABLES["SecondOrder2DUp"], (3, False): TABLES["ThirdOrderUp"], (3, True): TABLES["ThirdOrder2DUp"],
              (4, True): TABLES["FourthOrder2DUp"]}

ROTATOR_NOISE = 6.2e-07
ROTATOR_TOLERANCE = 5.0e-06


def channels_of(order, is_2d):
    return 2 * order + 1 if is_2d else (order + 1) ** 2


def needs_upsampler(dev_order, mix_2d, order, is_2d):
    """alu.cpp:1009-1010"""
    return dev_order > order or (dev_order >= 2 and not mix_2d and is_2d)


def device_cfg(order, mix_2d, num_sends):
    """a dry-line context whose dry bus holds every channel of an ambisonic mix of `order` (the 2D subset for 2D mixing), with scales
    that differ from line to line, and first-order slots"""
    idx = [int(i) for i in (TABLES["IndexFromACN2D"][:2 * order + 1] if mix_2d else range((order + 1) ** 2))]
    scale = [1.0 if i == 0 else float(F32(1.0 / (1.0 + 0.0625 * (i % 5)))) for i in idx]
    slots = num_sends                                       # (a fourth-order bus and one first-order slot: 29 of the library's 32 mixing lines)
    return dict(hrtf=False, sample_rate=48000, frequency=44100, num_dry=len(idx), num_real=2, num_sends=num_sends, num_slots=slots,
                wet_channels=4, dry_map=(idx, scale), wet_map=([0, 1, 2, 3], [1.0, 1.0, 1.0, 1.0]), ambi_order=order, mix_2d=mix_2d)


def ambi_source(src, order, is_2d=False, spatialize=AUTO, layout=ACN, scaling=S_SN3D, orient_at=(0.0, 0.0, -1.0), orient_up=(0.0, 1.0, 0.0)):
    return dict(src=src, order=order, is_2d=is_2d, spatialize=spatialize, layout=layout, scaling=scaling, orient_at=list(orient_at),
                orient_up=list(orient_up))


def for_cfg(cs, cfg):
    return dict(cs, src=sc.for_cfg(cs["src"], cfg))


def attenuated(cs):
    """CalcVoiceParams' route (alu.cpp:2024-2030): a B-Format source is never mono 3D"""
    return cs["spatialize"] == ON


def source_struct(cs, voices=()):
    return oalgpu.AmbiSource.make(sc.props_struct(cs["src"]), cs["order"], cs["is_2d"], cs["spatialize"], cs["layout"], cs["scaling"],
                                  cs["orient_at"], cs["orient_up"], voices)


def sources_array(css, voices=None):
    arr = (oalgpu.AmbiSource * len(css))()
    for i, cs in enumerate(css):
        arr[i] = source_struct(cs, voices[i] if voices is not None else ())
    return arr


def upsamplers_for(cfg, css):
    """what a context of cfg must be given for these sources: {(order, is_2d): matrix}"""
    return {(cs["order"], cs["is_2d"]): UPSAMPLERS[(cs["order"], cs["is_2d"])] for cs in css
            if needs_upsampler(cfg["ambi_order"], cfg["mix_2d"], cs["order"], cs["is_2d"])}


def params_host(cfg, lis, env, css):
    """oalgpu_ambi_source_params_host over the cases' sources -> (VoiceParams array, rot, mix)"""
    return oalgpu.ambi_source_params_host(sc.context_desc(cfg), sc.listener_struct(lis), sources_array(css), cfg["frequency"],
                                          cfg["ambi_order"], cfg["mix_2d"], upsamplers_for(cfg, css),
                                          slots=sc.env_array(env, cfg) if cfg["num_slots"] else None, dry_map=cfg["dry_map"],
                                          wet_maps=(cfg["wet_map"][0] * cfg["num_slots"], cfg["wet_map"][1] * cfg["num_slots"])
                                          if cfg["num_slots"] else None)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def rotator_coeffs():
    """RotatorCoeffs (alu.cpp:738-792): {(l, n, m): (u, v, w)}, computed in double and narrowed -- with v of m = 0 as Ivanic and
    Ruedenberg's Table I has it, (1 + delta_m0) inside the root: -sqrt((l - 1) l / (2 denom)).  The reference has the factor outside
    (-sqrt((l - 1) l / denom), alu.cpp:774), which is not a rotation: reference_rotator_coeffs() and
    test_ambi_sources_host.py::test_the_references_m0_constant_is_not_a_rotation"""
    out = {}
    for l in range(2, 5):
        for n in range(-l, l + 1):
            for m in range(-l, l + 1):
                denom = float((2 * l) * (2 * l - 1) if abs(n) == l else (l * l - n * n))
                if m == 0:
                    u, v, w = F32(np.sqrt(l * l / denom)), F32(np.sqrt(2.0 * ((l - 1) * l) / denom) * -0.5), F32(0.0)
                else:
                    am = abs(m)
                    u = F32(np.sqrt((l * l - m * m) / denom))
                    v = F32(np.sqrt((l + am - 1) * (l + am) / denom) * 0.5)
                    w = F32(np.sqrt((l - am - 1) * (l - am) / denom) * -0.5)
                out[(l, n, m)] = (u, v, w)
    return out


def reference_rotator_coeffs():
    """the same with the reference's own v of m = 0 (alu.cpp:774)"""
    out = rotator_coeffs()
    for (l, n, m), (u, v, w) in list(out.items()):
        if m == 0:
            denom = float((2 * l) * (2 * l - 1) if abs(n) == l else (l * l - n * n))
            out[(l, n, m)] = (u, F32(np.sqrt((l - 1) * l / denom) * -1.0), w)
    return out


_ROT_COEFFS = rotator_coeffs()


def ambi_rotator(R, order, F):
    """AmbiRotator (alu.cpp:799-888) on the 25 x 25 list-of-lists R whose zeroth- and first-order block is filled"""
    sqrt2 = F(F32(np.sqrt(2.0)))

    def P(i, l, a, n, last_base):
        ri1, rim1, ri0 = R[3][i + 2], R[1][i + 2], R[2][i + 2]
        x = last_base + (l - 1) + a
        if n == -l:
            return ri1 * R[last_base][x] + rim1 * R[last_base + (l - 1) * 2][x]
        if n == l:
            return ri1 * R[last_base + (l - 1) * 2][x] - rim1 * R[last_base][x]
        return ri0 * R[last_base + (l - 1) + n][x]

    def V(l, m, n, lb):
        if m > 0:
            p0, p1 = P(1, l, m - 1, n, lb), P(-1, l, -m + 1, n, lb)
            return p0 * sqrt2 if m == 1 else p0 - p1
        p0, p1 = P(1, l, m + 1, n, lb), P(-1, l, -m - 1, n, lb)
        return p1 * sqrt2 if m == -1 else p0 + p1

    def W(l, m, n, lb):
        if m > 0:
            return P(1, l, m + 1, n, lb) + P(-1, l, -m - 1, n, lb)
        return P(1, l, m - 1, n, lb) - P(-1, l, -m + 1, n, lb)

    base, last_base = 4, 1
    for l in range(2, order + 1):
        for n in range(-l, l + 1):
            for m in range(-l, l + 1):
                u, v, w = _ROT_COEFFS[(l, n, m)]
                r = F(0.0)
                if u != 0:
                    r = r + F(u) * P(0, l, m, n, last_base)
                if v != 0:
                    r = r + F(v) * V(l, m, n, last_base)
                if w != 0:
                    r = r + F(w) * W(l, m, n, last_base)
                R[base + l + n][base + l + m] = r
        last_base = base
        base += 2 * l + 1
    return R


def _normalize(v, F):
    lsq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    if lsq > F(sc.EPS):
        inv = F(1.0) / np.sqrt(lsq)
        return [x * inv for x in v]
    return [F(0.0)] * 3


def first_order_block(cs, lis, F, nudge=None):
    """alu.cpp:976-998 -> the 25 x 25 shrot with its zeroth- and first-order elements"""
    def inp(name, v):
        v = F32(v)
        if nudge is not None:
            v = nudge(name, v)
        return F(v)
    N = _normalize([inp("at%d" % k, cs["orient_at"][k]) for k in range(3)], F)
    V = _normalize([inp("up%d" % k, cs["orient_up"][k]) for k in range(3)], F)
    if not cs["src"]["head_relative"]:
        m = [inp("l_matrix%d" % k, v) for k, v in enumerate(lis["matrix"])]
        zero = F(0.0)

        def mul(vec):
            vec = list(vec) + [zero]
            return [vec[0] * m[0 * 4 + c] + vec[1] * m[1 * 4 + c] + vec[2] * m[2 * 4 + c] + vec[3] * m[3 * 4 + c] for c in range(3)]
        N, V = mul(N), mul(V)
    U = _normalize([N[1] * V[2] - N[2] * V[1], N[2] * V[0] - N[0] * V[2], N[0] * V[1] - N[1] * V[0]], F)
    R = [[F(0.0)] * 25 for _ in range(25)]
    R[0][0] = F(1.0)
    R[1][1], R[1][2], R[1][3] = U[0], -U[1], U[2]
    R[2][1], R[2][2], R[2][3] = -V[0], V[1], -V[2]
    R[3][1], R[3][2], R[3][3] = -N[0], N[1], -N[2]
    return R


def upsample(R, up, dev_order, F):
    """UpsampleBFormatTransform (alu.cpp:457-477): rows of `up` x 25; the other rows stay zero here"""
    nch = (dev_order + 1) ** 2
    out = [[F(0.0)] * 25 for _ in range(25)]
    for i in range(len(up)):
        for k in range(nch):
            a = F(up[i][k])
            for j in range(25):
                out[i][j] = R[k][j] * a + out[i][j]
    return out


def ambi_coeffs25(y, z, x, F):
    """CalcAmbiCoeffs(y, z, x) without spread, ACN 0..24 (core/ambidefs.h:219-271)"""
    c = lambda v: F(F32(v))
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    three, five, seven = F(3.0), F(5.0), F(7.0)
    return [F(1.0), c(1.7320508075688772) * y, c(1.7320508075688772) * z, c(1.7320508075688772) * x,
            c(3.872983346) * xy, c(3.872983346) * yz, c(1.118033989) * (three * zz - F(1.0)), c(3.872983346) * xz, c(1.936491673) * (xx - yy),
            c(2.091650066) * (y * (three * xx - yy)), c(10.24695076) * (z * xy), c(1.620185175) * (y * (five * zz - F(1.0))),
            c(1.322875656) * (z * (five * zz - three)), c(1.620185175) * (x * (five * zz - F(1.0))), c(5.123475383) * (z * (xx - yy)),
            c(2.091650066) * (x * (xx - three * yy)),
            c(8.874119675) * (xy * (xx - yy)), c(6.274950199) * ((three * xx - yy) * yz), c(3.354101966) * (xy * (seven * zz - F(1.0))),
            c(2.371708245) * (yz * (seven * zz - three)), c(0.375) * (F(35.0) * (zz * zz) - F(30.0) * zz + three),
            c(2.371708245) * (xz * (seven * zz - three)), c(1.677050983) * ((xx - yy) * (seven * zz - F(1.0))),
            c(6.274950199) * ((xx - three * yy) * xz), c(2.218529919) * ((xx * xx) - F(6.0) * (xx * yy) + (yy * yy))]


def calc(cs, lis, env, cfg, F=F32, nudge=None):
    """-> (base, channels, rot, mix): base = the source's results in source_param_cases.calc's form (either route), channels[c] =
    the line gains CalcAmbisonicPanning leaves in channel voice c, rot / mix = the two 25 x 25 matrices (None without coverage)"""
    zero, one = F(0.0), F(1.0)
    src = cs["src"]
    plain = dict(cfg, dry_map=([0], [1.0]))                 # (the mono stage's own line gains are not this stage's)
    base = sc.calc(src, lis, env, plain, F, nudge) if attenuated(cs) else cc._calc_non_attenuated(src, lis, env, plain, F, nudge)
    base["branch"]["route"] = attenuated(cs)
    numsends = cfg["num_sends"]
    distance, spread = base["distance"], base["spread"]
    has_distance = bool(distance > F(sc.EPS))
    coverage = one if not has_distance else (F(F32(1.0 / np.pi)) * F(0.5) * spread)
    covered = bool(coverage > zero)
    base["branch"]["has_distance"], base["branch"]["covered"] = has_distance, covered
    # (xpos, ypos, zpos): CalcAttnVoiceParams hands the zeroed ToSource down for a source at the listener (alu.cpp:2008-2009)
    pos = [zero, zero, zero] if (attenuated(cs) and not has_distance) else base["dir"]
    panned = ambi_coeffs25(-pos[0], pos[1], -pos[2], F)
    scales = [F(v) for v in SCALES[cs["scaling"]]]
    nch = channels_of(cs["order"], cs["is_2d"])
    index_map = [int(v) for v in INDEX[(cs["layout"], cs["is_2d"])][:nch]]
    dry_base, wet_base = base["dry"][0], [w[0] for w in base["wet"]]

    def pan_gains(coeffs, amap, gain, n):
        out = [zero] * n
        for t, (idx, scale) in enumerate(zip(*amap)):
            out[t] = F(F32(scale)) * coeffs[idx] * gain
        return out

    def channel(coeffs, dry_gain, wet_gains):
        ch = dict(dry_gains=[zero] * 32, send_gains=[[zero] * 25 for _ in range(sc.MAX_SENDS)])
        if coeffs is None:
            return ch
        ch["dry_gains"] = pan_gains(coeffs, cfg["dry_map"], dry_gain, 32)
        for i in range(numsends):
            if base["send_slot"][i] >= 0:
                ch["send_gains"][i] = pan_gains(coeffs, cfg["wet_map"], wet_gains[i], 25)
        return ch

    if not covered:                                         # :959-970
        chans = [channel(panned, dry_base * scales[0], [w * scales[0] for w in wet_base])]
        chans += [channel(None, zero, None) for _ in range(1, nch)]
        return base, chans, None, None

    rot = ambi_rotator(first_order_block(cs, lis, F, nudge), cfg["ambi_order"], F)
    if needs_upsampler(cfg["ambi_order"], cfg["mix_2d"], cs["order"], cs["is_2d"]):
        mix = upsample(rot, UPSAMPLERS[(cs["order"], cs["is_2d"])], cfg["ambi_order"], F)
    else:
        mix = rot
    pscale = (one - coverage) * scales[0]
    coeffs = [v * pscale for v in panned]
    chans = []
    for c in range(nch):
        acn = index_map[c]
        scale = scales[acn] * coverage
        coeffs = [mix[acn][j] * scale + coeffs[j] for j in range(25)]
        chans.append(channel(coeffs, dry_base, wet_base))
        coeffs = [zero] * 25
    return base, chans, rot, mix


def voice_params(base, ch, src, cfg):
    """channel voice `ch` of the restatement's results as an oalgpu_voice_params"""
    p = oalgpu.VoiceParams()
    p.step = base["step"]
    p.resampler = src["resampler"]
    p.direct_filter = oalgpu.FilterParams(int(base["filter_active"][0]), float(base["dry"][1]), float(base["hf_norm"][0]),
                                          float(base["dry"][2]), float(base["lf_norm"][0]))
    p.dry_gains[:] = [float(x) for x in ch["dry_gains"]]
    for i in range(sc.MAX_SENDS):
        p.send_slot[i] = base["send_slot"][i]
    for i in range(cfg["num_sends"]):
        p.send_filter[i] = oalgpu.FilterParams(int(base["filter_active"][1 + i]), float(base["wet"][i][1]), float(base["hf_norm"][1 + i]),
                                               float(base["wet"][i][2]), float(base["lf_norm"][1 + i]))
        p.send_gains[i][:] = [float(x) for x in ch["send_gains"][i]]
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_voice_params(vp, base, ch, cfg, exact, who=""):
    """an oalgpu_voice_params of oalgpu_ambi_source_params_host against the restatement: integers exact; the line gains bit for bit
    where `exact` (the OFF / AUTO route), otherwise within channel_source_cases.TOLERANCE of their class, a gain's scale being
    the source's largest base gain"""
    ns = cfg["num_sends"]
    assert vp.step == base["step"], (who, vp.step, base["step"])
    assert [vp.send_slot[i] for i in range(sc.MAX_SENDS)] == list(base["send_slot"]), who
    assert [vp.direct_filter.active] + [vp.send_filter[i].active for i in range(ns)] == [int(a) for a in base["filter_active"]], who
    assert vp.direct_filter.gain_lf == float(base["dry"][2]) and vp.direct_filter.hf_norm == float(base["hf_norm"][0]), who
    assert vp.direct_filter.lf_norm == float(base["lf_norm"][0]), who

    def close(x, y, tol, floor, what):
        x, y = float(x), float(y)
        assert abs(x - y) <= tol * max(abs(y), floor), (who, what, x, y, abs(x - y) / max(abs(y), floor), tol)
    close(vp.direct_filter.gain_hf, base["dry"][1], cc.TOLERANCE["gain_hf"], 1e-3, "dry hf")
    for i in range(ns):
        close(vp.send_filter[i].gain_hf, base["wet"][i][1], cc.TOLERANCE["gain_hf"], 1e-3, "wet hf")
        assert vp.send_filter[i].gain_lf == float(base["wet"][i][2]), who
    got = [list(vp.dry_gains)] + [list(vp.send_gains[i]) for i in range(sc.MAX_SENDS)]
    want = [ch["dry_gains"]] + ch["send_gains"]
    if exact:
        assert vp.direct_filter.gain_hf == float(base["dry"][1]), who
        for g, w in zip(got, want):
            assert np.array_equal(_bits(g), _bits([float(x) for x in w])), (who, g, w)
        return
    top = max([1e-3, float(base["dry"][0])] + [float(w[0]) for w in base["wet"]])
    for g, w in zip(got, want):
        for x, y in zip(g, w):
            close(x, y, cc.TOLERANCE["pan"], top, "line gain")


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
# group -> (device order, 2D mixing, source order, 2D source, layout, scaling)
GROUPS = {
    "first_on_first": (1, False, 1, False, ACN, S_N3D),             # no rotator, no upsample
    "first_2d_on_second_2d": (2, True, 1, True, ACN, S_SN3D),       # FirstOrder2DUp: the bridge's case
    "third_on_fourth": (4, False, 3, False, ACN, S_SN3D),           # 16 voices, ThirdOrderUp, rotator to band 4
    "second_2d_on_third_3d": (3, False, 2, True, ACN, S_N3D),       # the 2D-into-3D rule
    "fourth_2d_on_fourth_3d": (4, False, 4, True, ACN, S_SN3D),     # FourthOrder2DUp, equal orders
    "third_fuma_on_third": (3, False, 3, False, FUMA, S_FUMA),      # permutation and scales, no upsample
    "at_listener": (4, False, 3, False, ACN, S_SN3D),
    "away_radius_zero": (4, False, 3, False, ACN, S_N3D),           # coverage 0 on the ON route: channel 0 only
    "with_radius": (3, False, 2, True, ACN, S_SN3D),                # coverage between 0 and 1 on the ON route
    "head_relative": (2, True, 1, True, FUMA, S_FUMA),
    "missing_voice": (4, False, 3, False, ACN, S_SN3D),
}
MISSING_CHANNEL = 5                                                  # the channel without a voice in "missing_voice"


def _build():
    lcg = synth.Lcg(0x5EED0071)
    cases = []
    k = 0
    lis = sc.LISTENERS[0]
    for group, (dev_order, mix_2d, order, is_2d, layout, scaling) in GROUPS.items():
        for mode in (OFF, AUTO, ON):
            for sends in (0, 1, 2):
                k += 1
                s = sc._base(lcg, k)
                s["head_relative"] = 1 if group == "head_relative" else 0
                if sends:
                    s["send"][0][0] = 0
                    s["send"][1][0] = 1 if sends == 2 else -1
                if group == "at_listener":
                    s["position"] = list(lis["position"]); s["radius"] = 0.0
                elif group == "away_radius_zero":
                    s["radius"] = 0.0
                else:
                    p = np.array(s["position"], np.float64) - (0.0 if s["head_relative"] else np.array(lis["position"]))
                    s["radius"] = float(np.linalg.norm(p)) * (lcg.uniform(0.2, 0.8) if group != "third_on_fourth" else lcg.uniform(1.2, 2.5))
                at, up = sc._unit(lcg), sc._unit(lcg)
                while abs(float(np.dot(at, up))) > 0.8 * float(np.linalg.norm(at) * np.linalg.norm(up)):
                    up = sc._unit(lcg)
                scale = lcg.uniform(0.5, 3.0)               # (OrientAt need not be a unit vector)
                cs = ambi_source(s, order, is_2d, mode, layout, scaling, [x * scale for x in at], up)
                cases.append(dict(tag="%s_%s_%dsends" % (group, ("off", "on", "auto")[mode], sends), group=group, sends=sends, lis=0, env=0,
                                  dev=(dev_order, mix_2d), cs=cs))
    return cases


def cfg_of(case):
    return device_cfg(case["dev"][0], case["dev"][1], case["sends"])


def integer_results(base):
    return sc.integer_results(base)


_TABLE = None


def table():
    """-> (kept cases, dropped cases)"""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    kept, dropped = [], []
    patterns = [lambda name: 1, lambda name: -1]
    for case in _build():
        lis, env, cfg = sc.LISTENERS[case["lis"]], sc.ENVIRONMENTS[case["env"]], cfg_of(case)
        cs = for_cfg(case["cs"], cfg)
        want = integer_results(calc(cs, lis, env, cfg)[0])
        stable = all(integer_results(calc(cs, lis, env, cfg, nudge=sc._ulp_nudge(4, sign_of))[0]) == want for sign_of in patterns)
        (kept if stable else dropped).append(case)
    _TABLE = (kept, dropped)
    return _TABLE


def measure_rotator_noise(cases):
    """the float32 restatement of the rotator against the float64 one at order 4 over the cases' orientations: the largest absolute
    difference of a matrix entry"""
    worst = 0.0
    lis = sc.LISTENERS[0]
    for case in cases:
        a = ambi_rotator(first_order_block(case["cs"], lis, F32), 4, F32)
        b = ambi_rotator(first_order_block(case["cs"], lis, np.float64), 4, np.float64)
        worst = max(worst, float(np.abs(np.array(a, np.float64) - np.array(b, np.float64)).max()))
    return worst
