"""The near-field half of the source stage compiled for the host (oalgpu_channel_source_nfc_host: csrc/dev_source_nfc.hpp's
arithmetic, the same functions SourceNfcKernel compiles for the device) against the numpy restatement of
tests/nfc_source_cases.py, bit for bit: the w0 and the fourteen coefficients of every case, at 48 000 and at 44 100 Hz; and
against the library's own NfcFilter::init + adjust as oalgpu_voice_set_nfc runs it (oalgpu_nfc_adjust_host) at the same w0."""
import numpy as np
import pytest

import channel_source_cases as cc
import nfc_source_cases as nc
import oalgpu
import source_param_cases as sc

CFG = dict(hrtf=False, sample_rate=48000, frequency=44100, num_dry=5, num_real=0, num_sends=0, num_slots=0, wet_channels=4)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host(cs, lis, rate, avg=nc.AVG_SPEAKER_DIST):
    desc = sc.context_desc(dict(CFG, sample_rate=rate))
    w0, coeffs = oalgpu.channel_source_nfc_host(desc, sc.listener_struct(lis), cc.sources_array([cs]), CFG["frequency"], avg)
    return w0[0], coeffs[0]


def test_the_table_reaches_every_branch():
    seen = {}
    for tag, lis, cs, _ in nc.CASES:
        seen.setdefault(nc.expected(cs, nc.LISTENERS[lis])[2], []).append(tag)
    assert set(seen) == {"identity", "clamp", "distance"}, seen
    by_tag = {tag: (nc.LISTENERS[lis], cs, nc.expected(cs, nc.LISTENERS[lis])[2]) for tag, lis, cs, _ in nc.CASES}
    # a source at the listener, head-relative and in world coordinates under the rotated, translated listener
    assert by_tag["at_listener_head_relative"][2] == "identity" and by_tag["at_listener_world"][2] == "identity"
    # distance * NfcScale below AvgSpeakerDist / 4: by the distance, and by the scale alone
    assert by_tag["within_quarter_distance"][2] == "clamp" and by_tag["on_the_clamp_side_scaled"][2] == "clamp"
    assert float(nc.distance(by_tag["on_the_clamp_side_scaled"][1], nc.SCALED)) > nc.AVG_SPEAKER_DIST / 4
    assert by_tag["ordinary"][2] == "distance" and by_tag["nfc_scale_down"][2] == "distance" and by_tag["nfc_scale_up"][2] == "distance"
    for tag in ("ordinary_head_relative_rotated", "world_rotated"):
        lis, cs, branch = by_tag[tag]
        assert branch == "distance" and lis["matrix"] != nc.PLAIN["matrix"], tag
    # the rotation and the translation matter to the world position and not to the head-relative one
    lis, cs, _ = by_tag["world_rotated"]
    assert nc.distance(cs, lis) != nc.distance(cs, nc.PLAIN)
    lis, cs, _ = by_tag["ordinary_head_relative_rotated"]
    assert nc.distance(cs, lis) == nc.distance(cs, nc.PLAIN)
    # CalcNonAttnVoiceParams' route: distance 0 whatever the position
    for tag in ("stereo_off", "stereo_auto", "mono_off"):
        assert by_tag[tag][2] == "identity" and not cc.attenuated(by_tag[tag][1]), tag
    assert by_tag["x51_with_lfe"][1]["channels"] == cc.X51 and [c[3] for c in nc.CASES if c[0] == "x51_with_lfe"] == [None]
    assert [c[3] for c in nc.CASES if c[0] == "x71_without_lfe_and_rears"] == [(3, 4, 5)]
    assert {lis for _, lis, _, _ in nc.CASES} == set(nc.LISTENERS)


@pytest.mark.parametrize("rate", [48000, 44100])
@pytest.mark.parametrize("case", nc.CASES, ids=[c[0] for c in nc.CASES])
def test_host_function_equals_the_restatement_bit_for_bit(case, rate):
    tag, lis_name, cs, _ = case
    lis = nc.LISTENERS[lis_name]
    want_w0, want, branch = nc.expected(cs, lis, rate=rate)
    got_w0, got = _host(cs, lis, rate)
    print(tag, rate, branch, float(want_w0), [float(x) for x in want])
    assert _bits([got_w0])[0] == _bits([want_w0])[0], (tag, float(got_w0), float(want_w0))
    assert np.array_equal(_bits(got), _bits(want)), (tag, got, want)
    # the existing path at the same w0: oalgpu_voice_set_nfc's NfcInit + NfcAdjust
    w1 = float(nc.device_w1(nc.AVG_SPEAKER_DIST, rate))
    assert np.array_equal(_bits(oalgpu.nfc_adjust_host(w1, float(got_w0))), _bits(got)), tag
    # the identity filter is one: every a0 is 1 to rounding and b equals the device filter's a
    if branch == "identity":
        assert np.allclose(got[:4], 1.0, rtol=0, atol=3e-7), got[:4]


def test_a_closer_source_boosts_the_bass_more():
    """w0 grows as the source approaches, down to the clamp, and a0 (the filter's gain at DC relative to the device's) with it"""
    lis = nc.PLAIN
    prev_w0, prev_a0 = 0.0, 0.0
    for z in (-8.0, -3.0, -1.5, -0.8, -0.4):
        w0, coeffs = _host(cc.channel_source(sc.source(position=[0.0, 0.0, z]), cc.MONO, cc.ON), lis, 48000)
        assert w0 > prev_w0 and coeffs[0] > prev_a0, z
        prev_w0, prev_a0 = w0, coeffs[0]
    clamp = _host(cc.channel_source(sc.source(position=[0.0, 0.0, -0.375]), cc.MONO, cc.ON), lis, 48000)
    closer = _host(cc.channel_source(sc.source(position=[0.0, 0.0, -0.01]), cc.MONO, cc.ON), lis, 48000)
    assert _bits([clamp[0]])[0] == _bits([closer[0]])[0] and np.array_equal(_bits(clamp[1]), _bits(closer[1]))


def test_refusals():
    desc = sc.context_desc(CFG)
    lis = sc.listener_struct(nc.PLAIN)
    good = cc.channel_source(sc.source(), cc.MONO, cc.ON)
    for avg in (0.0, -1.0):
        with pytest.raises(oalgpu.OalgpuError, match="bad arguments"):
            oalgpu.channel_source_nfc_host(desc, lis, cc.sources_array([good]), 44100, avg)
    with pytest.raises(oalgpu.OalgpuError, match="bad arguments"):
        oalgpu.channel_source_nfc_host(desc, lis, cc.sources_array([good]), 0, 1.5)
    with pytest.raises(oalgpu.OalgpuError, match="channels or spatialize out of range"):
        oalgpu.channel_source_nfc_host(desc, lis, cc.sources_array([dict(good, channels=7)]), 44100, 1.5)
    with pytest.raises(oalgpu.OalgpuError, match="bad arguments"):
        oalgpu.channel_source_nfc_host(sc.context_desc(sc.HRTF_CFG), lis, cc.sources_array([good]), 44100, 1.5)
