"""The parameter stage of B-Format sources compiled for the host (oalgpu_ambi_source_params_host: csrc/dev_source_ambi.hpp's
arithmetic, the same functions AmbiParamsKernel compiles for the device) against the numpy restatement of
tests/ambi_source_cases.py, the fixture tests/golden/ambi_tables.npz against the compiled reference, the rotator against the
reference's own encoder, and every refusal with its message."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ambi_source_cases as ac
import channel_source_cases as cc
import oalgpu
import oracle_lib as ol
import source_param_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("oalgpu_context_set_ambi_order", "oalgpu_context_set_ambi_upsampler", "oalgpu_voice_set_ambi_sources",
       "oalgpu_param_block_create_from_ambi_sources", "oalgpu_ambi_source_params_host", "oalgpu_ambi_tables_host")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_entry_points_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oalgpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(oalgpu_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and hasattr(oalgpu.lib, name), name
    for struct in ("oalgpu_ambi_source", "oalgpu_ambi_device"):
        assert re.search(r"\}\s*%s\s*;" % struct, hdr), struct
    # the header says what stays out
    text = open(os.path.join(ROOT, "include", "oalgpu.h")).read()
    assert "UHJ and Super Stereo formats" in text and "Pairwise" in text
    assert C.sizeof(oalgpu.AmbiSource) == C.sizeof(oalgpu.SourceProps) + 4 * 5 + 4 * 6 + 4 * oalgpu.MAX_AMBI_CHANNELS


def test_fixture_holds_the_compiled_references_tables():
    """FirstOrderUp and SecondOrderUp as the oracle hands them out (when it is built); the tables the library derives from their
    definitions equal the fixture's bit for bit"""
    t = ac.TABLES
    assert sorted(t.files) == sorted(["FirstOrderUp", "FirstOrder2DUp", "SecondOrderUp", "SecondOrder2DUp", "ThirdOrderUp", "ThirdOrder2DUp",
                                      "FourthOrder2DUp", "FromFuMa", "FromSN3D", "FromN3D", "IndexFromFuMa", "IndexFromFuMa2D", "IndexFromACN",
                                      "IndexFromACN2D"])
    for (order, _), m in ac.UPSAMPLERS.items():
        assert m.shape == ((order + 1) ** 2, 25) and m.dtype == np.float32
    if ol.available("ref"):
        R = ol.load("ref")
        _, up1, _ = R.ambi_upmix_info(2)
        assert np.array_equal(_bits(up1), _bits(t["FirstOrderUp"]))
        f32p = C.POINTER(C.c_float)
        R.L.oal_ambi_upmix_info2.argtypes = [C.c_uint32, C.c_int, f32p, f32p]
        R.L.oal_ambi_upmix_info2.restype = None
        sc2, up2 = np.zeros(3, np.float32), np.zeros((9, 25), np.float32)
        R.L.oal_ambi_upmix_info2(3, 0, sc2.ctypes.data_as(f32p), up2.ctypes.data_as(f32p))
        assert np.array_equal(_bits(up2), _bits(t["SecondOrderUp"]))
    scales, index = oalgpu.ambi_tables_host()
    for i, name in enumerate(("FromFuMa", "FromSN3D", "FromN3D")):
        assert np.array_equal(_bits(scales[i]), _bits(t[name])), name
    for i, name in enumerate(("IndexFromFuMa", "IndexFromFuMa2D", "IndexFromACN", "IndexFromACN2D")):
        n = len(t[name])
        assert np.array_equal(index[i][:n], t[name]) and not index[i][n:].any(), name


PLAIN = sc.listener()
# a turned listener whose AT and UP are at right angles (source_param_cases.LISTENERS[0]'s are not, and CalcContextParams does not
# orthogonalise: its matrix is no rotation, and neither is anything built from it)
_AT = np.array([0.3, -0.2, -1.0])
_UP = np.array([0.1, 1.0, 0.05])
TURNED = sc.oriented_listener([float(v) for v in _AT], [float(v) for v in _UP - _AT * (np.dot(_AT, _UP) / np.dot(_AT, _AT))],
                              (1.5, -0.5, 2.0), (0.0, 0.0, 0.0))


def _rotation(at, up, order=4, lis=PLAIN, head_relative=1):
    """the rotation matrix the host compilation builds for an orientation on a device of `order` (a source at the listener: full
    coverage)"""
    cfg = ac.device_cfg(order, False, 0)
    src = sc.source(position=[0.0, 0.0, 0.0], head_relative=head_relative)
    cs = ac.ambi_source(src, order, False, ac.OFF, ac.ACN, ac.S_N3D, at, up)
    _, rot, mix = ac.params_host(cfg, lis, sc.ENVIRONMENTS[0], [cs])
    assert np.array_equal(_bits(rot), _bits(mix))           # equal orders, 3D: no upsample
    return rot[0]


def test_identity_orientation_is_the_identity_matrix():
    rot = _rotation((0.0, 0.0, -1.0), (0.0, 1.0, 0.0))
    assert np.array_equal(rot, np.eye(25, dtype=np.float32))
    rot = _rotation((0.0, 0.0, -3.0), (0.0, 0.5, 0.0), order=2)      # (not unit vectors; the bands above the order stay empty)
    want = np.zeros((25, 25), np.float32); want[:9, :9] = np.eye(9)
    assert np.array_equal(rot, want)


def _encode(direction_ambi):
    """the N3D encoding of a direction given in ambisonic coordinates (y, z, x), by the compiled reference's CalcDirectionCoeffs
    where the oracle is built, by the library's own CalcAmbiCoeffs otherwise (a source without coverage on an identity dry map:
    channel 0's line gains are the coefficients)"""
    y, z, x = [float(v) for v in direction_ambi]
    d = np.array([-y, z, -x], np.float32)                   # OpenAL space (core/mixer.h:71-72)
    if ol.available("ref"):
        return ol.load("ref").direction_coeffs(d).astype(np.float64)
    cfg = dict(ac.device_cfg(4, False, 0), dry_map=(list(range(25)), [1.0] * 25))
    src = sc.source(position=[float(v) * 2.0 for v in d], head_relative=1, radius=0.0, distance_model=sc.DISABLE, gain=1.0)
    cs = ac.ambi_source(src, 1, False, ac.ON, ac.ACN, ac.S_N3D)
    out, _, _ = oalgpu.ambi_source_params_host(sc.context_desc(cfg), sc.listener_struct(PLAIN), ac.sources_array([cs]), cfg["frequency"], 4, False,
                                               {(1, False): ac.UPSAMPLERS[(1, False)]}, dry_map=cfg["dry_map"])
    return np.array(list(out[0].dry_gains)[:25], np.float64)


def _orientation(rng):
    at, up = rng.normal(size=3), rng.normal(size=3)
    up = up - at * (np.dot(at, up) / np.dot(at, at))        # (the reference does not orthogonalise: a rotation needs AT and UP at right angles)
    return [float(v) for v in at], [float(v) for v in up]


def _carry_residual(rot, order, rng, encode):
    """with the convention the mixer uses (output j = sum over input channels c of in[c] * matrix[c][j]) the first-order block says
    where a direction of the source's frame lies in the listener's; -> the largest |matrix^T e(source direction) - e(listener
    direction)| over four directions, the largest 1-norm of a source encoding, the largest higher-band coefficient met"""
    nch = (order + 1) ** 2
    block = rot[1:4, 1:4]
    worst = norm1 = top = 0.0
    for _ in range(4):
        d = rng.normal(size=3); d = (d / np.linalg.norm(d)).astype(np.float32).astype(np.float64)           # (y, z, x) of the source's frame
        out = block.T @ d
        e_in, e_out = encode(d), encode(out / np.linalg.norm(out))
        worst = max(worst, float(np.abs((rot.T @ e_in)[:nch] - e_out[:nch]).max()))
        norm1 = max(norm1, float(np.abs(e_in[:nch]).sum()))
        top = max(top, float(np.abs(e_out[4:nch]).max()))
    return worst, norm1, top


def test_rotator_carries_encodings_between_the_frames():
    """For random orientations at orders 2 to 4 the matrix must carry the encoding of a direction in the source's frame to the
    encoding of the same direction in the listener's frame (encodings by the compiled reference's CalcDirectionCoeffs, or the
    library's own CalcAmbiCoeffs where the oracle is absent; the transpose convention from the first-order block).  The bound on
    every coefficient is ROTATOR_TOLERANCE: 8 x the measured float32-against-float64 disagreement of the recurrence over the case
    table (ambi_source_cases), 5.0e-06.  Measured over the twelve orientations below: residuals of 1.4e-07 .. 1.2e-06."""
    kept, _ = ac.table()
    noise = ac.measure_rotator_noise(kept)
    print("rotator float32 vs float64 over the table: %.3g (recorded %.3g, tolerance %.3g)" % (noise, ac.ROTATOR_NOISE, ac.ROTATOR_TOLERANCE))
    assert noise <= ac.ROTATOR_NOISE and ac.ROTATOR_TOLERANCE >= 8.0 * ac.ROTATOR_NOISE > 0.9 * ac.ROTATOR_TOLERANCE
    rng = np.random.default_rng(0x5EED0072)
    failures = []
    for trial in range(12):
        order = 2 + trial % 3
        at, up = _orientation(rng)
        lis = TURNED if trial % 2 else PLAIN
        rot = _rotation(at, up, order, lis, head_relative=0 if trial % 2 else 1).astype(np.float64)
        nch = (order + 1) ** 2
        assert not rot[nch:].any() and not rot[:, nch:].any()
        worst, norm1, top = _carry_residual(rot, order, rng, _encode)
        bound = ac.ROTATOR_TOLERANCE
        print("trial %d order %d: residual %.3g bound %.3g" % (trial, order, worst, bound))
        assert top > 0.1                                    # (the higher bands are not empty)
        if worst > bound:
            failures.append((trial, order, worst, bound))
    assert not failures, failures


def test_the_references_m0_constant_is_not_a_rotation():
    """what the library builds IS the recurrence of the restatement (bit for bit the float32 one, within ROTATOR_TOLERANCE of the
    float64 one), an orthogonal matrix -- and it is NOT the reference's where the reference is not a rotation: with RotatorCoeffs'
    own v of m = 0 (alu.cpp:774, the factor (1 + delta_m0) outside the root) the same recurrence misses the check above by
    0.05 .. 1.3 and is off orthogonality by up to 0.5, in the columns |m| <= l - 2 only; the columns |m| >= l - 1, all a 2D device
    reads, are the same under both constants"""
    rng = np.random.default_rng(0x5EED0073)
    exact64 = lambda d: np.array(ac.ambi_coeffs25(d[0], d[1], d[2], np.float64))
    for trial in range(6):
        order = 2 + trial % 3
        nch = (order + 1) ** 2
        at, up = _orientation(rng)
        rot = _rotation(at, up, order)
        cs = ac.ambi_source(sc.source(head_relative=1), order, False, ac.OFF, ac.ACN, ac.S_N3D, at, up)
        r32 = np.array(ac.ambi_rotator(ac.first_order_block(cs, PLAIN, np.float32), order, np.float32), np.float32)
        r64 = np.array(ac.ambi_rotator(ac.first_order_block(cs, PLAIN, np.float64), order, np.float64))
        assert np.array_equal(_bits(rot), _bits(r32)), trial
        assert np.abs(rot.astype(np.float64) - r64).max() <= ac.ROTATOR_TOLERANCE, trial
        assert np.abs(r64[:nch, :nch] @ r64[:nch, :nch].T - np.eye(nch)).max() <= 1e-6, trial
        worst, _, top = _carry_residual(r64, order, rng, exact64)
        assert worst <= 1e-6 and top > 0.1, (trial, order, worst)
        saved = ac._ROT_COEFFS
        try:
            ac._ROT_COEFFS = ac.reference_rotator_coeffs()
            ref64 = np.array(ac.ambi_rotator(ac.first_order_block(cs, PLAIN, np.float64), order, np.float64))
        finally:
            ac._ROT_COEFFS = saved
        as_is, _, _ = _carry_residual(ref64, order, rng, exact64)
        assert as_is > 1e-2, (trial, order, as_is)
        assert np.abs(ref64[:nch, :nch] @ ref64[:nch, :nch].T - np.eye(nch)).max() > 1e-2, trial
        differ = np.abs(ref64 - r64).max(axis=0) > 1e-9      # by column
        for l in range(2, order + 1):
            for m in range(-l, l + 1):
                assert differ[l * l + l + m] == (abs(m) <= l - 2), (trial, l, m)
        assert not differ[:4].any()


def test_the_table_covers_the_issues_cases():
    kept, dropped = ac.table()
    total = len(kept) + len(dropped)
    assert total == 11 * 9 and len(dropped) <= 0.1 * total, (len(kept), [c["tag"] for c in dropped])
    for group in ac.GROUPS:
        mine = [c for c in kept if c["group"] == group]
        assert len(mine) >= 5, (group, len(mine))            # no group dropped whole
        assert {c["cs"]["spatialize"] for c in mine} == {ac.OFF, ac.ON, ac.AUTO} and {c["sends"] for c in mine} == {0, 1, 2}, group
    seen = set()
    for c in kept:
        lis, env, cfg = sc.LISTENERS[c["lis"]], sc.ENVIRONMENTS[c["env"]], ac.cfg_of(c)
        base, chans, rot, mix = ac.calc(ac.for_cfg(c["cs"], cfg), lis, env, cfg)
        b = base["branch"]
        cov = "none" if not b["covered"] else ("full" if not b["has_distance"] else "partial")
        seen.add((c["group"], b["route"], cov))
        if c["group"] == "away_radius_zero" and b["route"]:
            assert cov == "none" and mix is None and not any(any(ch["dry_gains"]) for ch in chans[1:])
        if c["group"] in ("with_radius", "third_on_fourth") and b["route"]:
            assert cov == "partial", c["tag"]
        if c["group"] == "at_listener":
            assert cov == "full", c["tag"]
    assert ("away_radius_zero", True, "none") in seen and ("with_radius", True, "partial") in seen and ("at_listener", True, "full") in seen
    assert ("head_relative", True, "partial") in seen or ("head_relative", True, "none") in seen


def test_host_compilation_against_the_restatement():
    """the mix matrix (and the rotation) bit for bit on every route; every line gain bit for bit on the OFF / AUTO route; the gain
    classes within channel_source_cases.TOLERANCE on the ON route"""
    kept, _ = ac.table()
    exact = close = 0
    for c in kept:
        lis, env, cfg = sc.LISTENERS[c["lis"]], sc.ENVIRONMENTS[c["env"]], ac.cfg_of(c)
        cs = ac.for_cfg(c["cs"], cfg)
        base, chans, rot, mix = ac.calc(cs, lis, env, cfg)
        out, hrot, hmix = ac.params_host(cfg, lis, env, [cs])
        if mix is None:
            assert not hrot.any() and not hmix.any(), c["tag"]
        else:
            assert np.array_equal(_bits(np.array(rot, np.float32)), _bits(hrot[0])), c["tag"]
            assert np.array_equal(_bits(np.array(mix, np.float32)), _bits(hmix[0])), c["tag"]
            up = ac.needs_upsampler(cfg["ambi_order"], cfg["mix_2d"], cs["order"], cs["is_2d"])
            assert up != np.array_equal(hrot[0], hmix[0]), c["tag"]
        nch = ac.channels_of(cs["order"], cs["is_2d"])
        assert len(chans) == nch
        for k in range(oalgpu.MAX_AMBI_CHANNELS):
            if k < nch:
                ac.check_voice_params(out[k], base, chans[k], cfg, not ac.attenuated(cs), "%s channel %d" % (c["tag"], k))
            else:
                assert bytes(out[k]) == bytes(C.sizeof(oalgpu.VoiceParams)), (c["tag"], k)
        assert any(out[0].dry_gains) or float(base["dry"][0]) == 0.0, c["tag"]
        if ac.attenuated(cs):
            close += 1
        else:
            exact += 1
    assert exact >= 50 and close >= 25, (exact, close)


def test_sources_of_one_call_do_not_disturb_each_other():
    """several sources of different orders in one host call equal the calls one by one"""
    kept, _ = ac.table()
    mine = [c for c in kept if c["dev"] == (4, False) and c["sends"] == 2][:6]
    assert len({(c["cs"]["order"], c["cs"]["is_2d"]) for c in mine}) >= 2
    lis, env, cfg = sc.LISTENERS[0], sc.ENVIRONMENTS[0], ac.cfg_of(mine[0])
    css = [ac.for_cfg(c["cs"], cfg) for c in mine]
    out, rot, mix = ac.params_host(cfg, lis, env, css)
    for i, cs in enumerate(css):
        one, r1, m1 = ac.params_host(cfg, lis, env, [cs])
        assert np.array_equal(_bits(m1[0]), _bits(mix[i])) and np.array_equal(_bits(r1[0]), _bits(rot[i]))
        for k in range(oalgpu.MAX_AMBI_CHANNELS):
            assert bytes(one[k]) == bytes(out[i * oalgpu.MAX_AMBI_CHANNELS + k]), (i, k)


def test_host_refusals():
    lis, env = sc.LISTENERS[0], sc.ENVIRONMENTS[0]
    cfg = ac.device_cfg(3, False, 2)
    good = ac.for_cfg(ac.ambi_source(sc.source(), 1), cfg)

    def refused(match, cs, cfg=cfg, ups=None):
        with pytest.raises(oalgpu.OalgpuError, match=match):
            oalgpu.ambi_source_params_host(sc.context_desc(cfg), sc.listener_struct(lis), ac.sources_array([cs]), cfg["frequency"],
                                           cfg["ambi_order"], cfg["mix_2d"], ac.upsamplers_for(cfg, [cs]) if ups is None else ups,
                                           slots=sc.env_array(env, cfg), dry_map=cfg["dry_map"])
    refused("order, layout or scaling out of range", dict(good, order=0), ups={})
    refused("order, layout or scaling out of range", dict(good, order=5), ups={})
    refused("order, layout or scaling out of range", dict(good, layout=2))
    refused("order, layout or scaling out of range", dict(good, scaling=3))
    refused("order, layout or scaling out of range", dict(good, spatialize=3))
    cfg4 = ac.device_cfg(4, False, 2)
    refused("FuMa layout and scaling reach order 3", dict(good, order=4, is_2d=True, layout=ac.FUMA), cfg4, ups={(4, True): ac.UPSAMPLERS[(4, True)]})
    refused("FuMa layout and scaling reach order 3", dict(good, order=4, scaling=ac.S_FUMA), cfg4, ups={})
    refused("needs an upsampler", good, ups={})
    refused("needs an upsampler", dict(good, order=3, is_2d=True), ups={(3, False): ac.UPSAMPLERS[(3, False)]})      # (the 2D-into-3D rule)
    bad = sc.source(); bad["send"][1][0] = cfg["num_slots"]
    refused("send slot out of range", dict(good, src=bad))
    refused("bad arguments", good, dict(cfg, hrtf=True))
    refused("bad arguments", good, dict(cfg, ambi_order=5))
    # a third-order 3D source on the third-order device needs none
    oalgpu.ambi_source_params_host(sc.context_desc(cfg), sc.listener_struct(lis), ac.sources_array([dict(good, order=3)]), cfg["frequency"], 3,
                                   False, {}, slots=sc.env_array(env, cfg), dry_map=cfg["dry_map"])


def test_a_fresh_near_field_filter_is_not_adjusted_to_zero():
    """why near-field contexts refuse ambisonic sources (include/oalgpu.h): NfcFilter::init(w1) leaves the pass-through -- b = a(w1),
    a0 = 1, which adjust(w1) reproduces -- and adjust(0) leaves b = 0, a0 = mBaseGain < 1 (core/filters/nfc.cpp:56-83): a voice the
    reference never adjusted does not hold what adjust(0) would give it"""
    w1 = float(np.float32(343.3) / np.float32(1.5) / np.float32(48000.0))
    zero, through = oalgpu.nfc_adjust_host(w1, 0.0), oalgpu.nfc_adjust_host(w1, w1)
    assert not zero[4:].any() and (zero[:4] > 0.0).all() and (zero[:4] < 0.999).all(), zero
    assert np.abs(through[:4] - 1.0).max() <= 2.0 ** -22 and (through[4:] > 0.0).all(), through
    assert not np.array_equal(zero, through)
