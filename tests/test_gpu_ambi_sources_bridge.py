"""The ambisonic source stage end to end against the compiled reference: the bridge in MODE_CPU renders
tests/test_bridge.py::render_ambi2's scene -- five mono sources and two first-order 2D B-Format sources (ACN / SN3D, turned by
OrientAt = {0.6, 0, -0.8}; one at the listener, one away) on the stereo device that mixes second-order 2D ambisonics -- with the
reference's own CalcVoiceParams, CalcAmbisonicPanning among it, Voice::mix and post-process.  A library context set up like
that device is fed ONLY source properties -- oalgpu_voice_set_source_props for the mono sources, oalgpu_voice_set_ambi_sources
with the fixture's FirstOrder2DUp for the B-Format sources' three channel voices each -- and must reproduce the frames within
2e-5 max(|want|) + 1e-7, the sources' state exactly.

The bridge's sources are spatialize Auto, so this pins the non-attenuated route (the source plays around the listener wherever
it is), the rotation's first-order block and band 2 as the 2D device reads it (the columns of ACN 4 and 8), and the 2D upsample.
The attenuated route rests on the numpy restatement and on CalcDirectionCoeffs for its panned W
(tests/test_ambi_sources_host.py).  Control distance 0 only: near-field contexts refuse ambisonic sources (include/oalgpu.h)."""
import numpy as np
import pytest

import ambi_source_cases as ac
import bridge_lib as bl
import oalgpu
import oracle_lib as ol
import source_param_cases as sc

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not bl.available(), reason="needs oracle/_ref/liboalbridge.so (the compiled reference)")]
UPDATES = 6
BFORMAT = (dict(looping=True, position=100, gain=0.3, pos=(0.0, 0.0, 0.0), resampler=bl.RS_LINEAR, pitch=1.0, gain_hf=1.0),
           dict(looping=False, position=5000, gain=0.25, pos=(0.3, 0.0, -1.0), resampler=bl.RS_BSINC24, pitch=1.1, gain_hf=0.6))
ORIENT_AT = (0.6, 0.0, -0.8)


def _mono(v, k):
    """source v in update k as render_ambi2 has it: (gain, position, resampler, gain_hf); the even ones move from update 1 on"""
    if k and v % 2 == 0:
        return 0.2 + 0.01 * k, (float(v - 2) * (1.0 - 0.1 * k), 0.1 * k, -2.0 + 0.3 * k), bl.RS_LINEAR, 1.0
    return 0.2, (float(v - 2), 0.0, -2.0 + 0.4 * v), bl.RS_BSINC24 if v % 2 else bl.RS_LINEAR, 0.5 if v == 1 else 1.0


def _data():
    rng = np.random.default_rng(0xB0F)
    mono = [rng.uniform(-1, 1, 20000).astype(np.float32) for _ in range(3)]
    bf = rng.uniform(-1, 1, (12000, 3)).astype(np.float32)
    return mono, [bf, bf[::-1].copy()]


def _props(gain, pos, rs, pitch, gain_hf):
    return sc.source(position=list(pos), gain=gain, pitch=pitch, resampler=rs, direct=[1.0, gain_hf, 5000.0, 1.0, 250.0])


def _library(with_bformat):
    mono, bformat = _data()
    api = oalgpu.Api(oalgpu.MATH_FAST)
    scene = oalgpu.Scene(api, sample_rate=48000, num_dry=5, num_real=2, max_voices=16, max_buffers=16)
    scene.set_ambi_map([int(i) for i in ac.TABLES["IndexFromACN2D"][:5]], [1.0] * 5)         # W, Y, X, V, U
    dec = np.zeros((2, oalgpu.MAX_AMBI), np.float32)
    dec[0, :5] = [5.00000000e-1, 2.88675135e-1, 5.52305643e-2, 3.1e-2, -1.7e-2]
    dec[1, :5] = [5.00000000e-1, -2.88675135e-1, 5.52305643e-2, -3.1e-2, -1.7e-2]
    scene.set_bformat_decoder(dec, None, 400.0 / 48000.0)
    scene.set_ambi_order(2, True)
    scene.set_ambi_upsampler(1, True, ac.TABLES["FirstOrder2DUp"])
    scene.set_listener(sc.listener_struct(sc.listener(distance_model=sc.INVERSE_CLAMPED)))      # the bridge's context (ref_bridge.cpp)
    handles = [scene.add_buffer(m, oalgpu.FMT_FLOAT) for m in mono]
    voices = [scene.add_voice(handles[v % 3], True, position=997 * v, frequency=44100) for v in range(5)]
    firsts = []
    if with_bformat:
        # Voice::prepare's HF scales of a first-order 2D source on the second-order 2D device (voice.cpp:1362-1385), by channel order
        hf, _, _ = ol.load("ref").ambi_upmix_info(2, horizontal=True)
        for d, b in zip(bformat, BFORMAT):
            first = scene.add_ambi_voice(scene.add_buffer(d, oalgpu.FMT_FLOAT, frame_step=3), 3, b["looping"], position=b["position"], frequency=44100)
            for c in range(3):
                scene.set_channel_ambi_scale(first, c, 400.0 / 48000.0, float(hf[0 if c == 0 else 1]), 1.0)
            firsts.append(first)
    out = []
    for k in range(UPDATES):
        moved = voices if k == 0 else voices[0:5:2]
        props = []
        for v in moved:
            gain, pos, rs, gain_hf = _mono(v, k)
            props.append(_props(gain, pos, rs, 1.0, gain_hf))
        scene.set_source_props(moved, sc.props_array(props))
        if k == 0 and with_bformat:
            css = [ac.ambi_source(_props(b["gain"], b["pos"], b["resampler"], b["pitch"], b["gain_hf"]), 1, True, ac.AUTO, ac.ACN, ac.S_SN3D,
                                  ORIENT_AT) for b in BFORMAT]
            scene.set_ambi_sources(ac.sources_array(css, [[f, f + 1, f + 2] for f in firsts]))
        if k == 4:
            scene.set_state(voices[1], oalgpu.VOICE_STOPPING)
        scene.mix(1024, post_process=True)
        out.append(scene.read_output(1024, frame_step=2).reshape(1024, 2).copy())
    states = [scene.voice_state(v) for v in voices + firsts]
    scene.close()
    return np.concatenate(out), [(s.play_state, s.position, s.position_frac) for s in states]


def test_bformat_sources_from_source_properties():
    import test_bridge
    want, wstate, _ = test_bridge.render_ambi2(bl.MODE_CPU, 0.0)
    got, gstate = _library(True)
    assert gstate == [tuple(s[:3]) for s in wstate], (gstate, wstate)
    err = float(np.abs(got.astype(np.float64) - want).max())
    bound = 2e-5 * float(np.abs(want).max()) + 1e-7
    print("second-order 2D device: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound, (err, bound)
    # the kind is audible: the same scene without its B-Format sources
    other, _, _ = test_bridge.render_ambi2(bl.MODE_CPU, 0.0, with_bformat=False)
    assert float(np.abs(other - want).max()) > 1e-3
    plain, _ = _library(False)
    assert float(np.abs(plain.astype(np.float64) - other).max()) <= 2e-5 * float(np.abs(other).max()) + 1e-7
