"""The near-field source stage end to end against the compiled reference: the bridge in MODE_CPU renders five mono sources and
one stereo source on its second-order 2D device with a control distance of 1.5 (InitNearFieldCtrl: AvgSpeakerDist, the
control filter; NumChannelsPerOrder 1, 2, 2) with the reference's own CalcVoiceParams -- CalcNormalPanning's w0 and
NFCtrlFilter.adjust among it -- Voice::mix (DoNfcMix) and post-process.  A library context set up like that device is fed ONLY
source properties plus oalgpu_context_set_nfc / oalgpu_context_set_nfc_distance and must reproduce the frames within
test_bridge.py's bound for this device, the sources' state exactly.  Among the moves: one that brings a source within
AvgSpeakerDist / 4 of the listener (the clamp) and one that puts a source at the listener (the identity filter)."""
import numpy as np
import pytest

import bridge_lib as bl
import channel_source_cases as cc
import oalgpu
import source_param_cases as sc

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not bl.available(), reason="needs oracle/_ref/liboalbridge.so (the compiled reference)")]
TODO = (1024, 1024, 700, 1024)
CONTROL_DISTANCE = 1.5
STEREO = dict(position=100, gain=0.3, pos=(0.5, 0.0, -1.0), pitch=1.07, gain_hf=0.8)


def _mono(v, k):
    """source v in update k: (gain, position, resampler, pitch, gain_hf); the even ones move -- source 0 to within a quarter of the
    control distance in update 2, source 2 onto the listener in update 1 and away again in update 3"""
    pos = (float(v - 2), 0.0, -2.0)
    if v % 2 == 0 and k:
        pos = (float(v - 2) * (1.0 - 0.1 * k), 0.1 * k, -2.0)
    if v == 0 and k >= 2:
        pos = (0.1, 0.05, -0.2) if k == 2 else (0.3, 0.0, -0.9)
    if v == 2 and k in (1, 2):
        pos = (0.0, 0.0, 0.0)
    if v == 2 and k == 3:
        pos = (0.4, 0.1, -1.0)
    return (0.2 + 0.01 * (k if v % 2 == 0 else 0), pos, bl.RS_LINEAR, 1.0 + 0.05 * v, 0.5 if v == 1 else 1.0)


def _reference(control_distance, mono, stereo):
    b = bl.Bridge(bl.MODE_CPU, ambi2=True, control_distance=control_distance)
    try:
        bufs = [b.add_buffer(m) for m in mono]
        srcs = []
        for v in range(5):
            gain, pos, rs, pitch, gain_hf = _mono(v, 0)
            srcs.append(b.add_source(bufs[v % 3], True, 997 * v, gain, pos, resampler=rs, pitch=pitch, gain_hf=gain_hf))
        st = b.add_source_stereo(b.add_buffer_interleaved(stereo, 2), True, STEREO["position"], STEREO["gain"], STEREO["pos"],
                                 resampler=bl.RS_LINEAR, pitch=STEREO["pitch"], gain_hf=STEREO["gain_hf"])
        out = []
        for k, n in enumerate(TODO):
            if k:
                for v in range(0, 5, 2):
                    gain, pos, rs, pitch, gain_hf = _mono(v, k)
                    b.update_source(srcs[v], gain, pos, resampler=rs, pitch=pitch, gain_hf=gain_hf)
            out.append(b.render(n))
        return np.concatenate(out), [tuple(b.source_state(h)[:3]) for h in srcs + [st]], [b.source_flags(h) for h in srcs + [st]]
    finally:
        b.close()


def _props(gain, pos, rs, pitch, gain_hf):
    return sc.source(position=list(pos), gain=gain, pitch=pitch, resampler=rs, direct=[1.0, gain_hf, 5000.0, 1.0, 250.0])


def test_near_field_sources_from_source_properties():
    rng = np.random.default_rng(0xC0FFEE)
    mono = [rng.uniform(-1, 1, 20000).astype(np.float32) for _ in range(3)]
    stereo = rng.uniform(-1, 1, (9000, 2)).astype(np.float32)
    want, wstate, wflags = _reference(CONTROL_DISTANCE, mono, stereo)

    api = oalgpu.Api(oalgpu.MATH_FAST)
    scene = oalgpu.Scene(api, sample_rate=48000, num_dry=5, num_real=2, max_voices=8, max_buffers=16)
    scene.set_ambi_map([0, 1, 3, 4, 8], [1.0] * 5)                          # AmbiIndex::FromACN2D: W, Y, X, V, U
    dec = np.zeros((2, oalgpu.MAX_AMBI), np.float32)
    dec[0, :5] = [5.00000000e-1, 2.88675135e-1, 5.52305643e-2, 3.1e-2, -1.7e-2]
    dec[1, :5] = [5.00000000e-1, -2.88675135e-1, 5.52305643e-2, -3.1e-2, -1.7e-2]
    scene.set_bformat_decoder(dec, None, 400.0 / 48000.0)
    # InitNearFieldCtrl as the bridge's device has it: w1 = 343.3f / AvgSpeakerDist / rate, channels per order 1, 2, 2
    w1 = float(np.float32(343.3) / np.float32(CONTROL_DISTANCE) / np.float32(48000.0))
    scene.set_nfc(w1, [1, 2, 2])
    scene.set_nfc_distance(CONTROL_DISTANCE)
    scene.set_listener(sc.listener_struct(sc.listener(distance_model=sc.INVERSE_CLAMPED)))      # the bridge's context (ref_bridge.cpp)
    handles = [scene.add_buffer(m, oalgpu.FMT_FLOAT) for m in mono]
    voices = [scene.add_voice(handles[v % 3], True, position=997 * v, frequency=44100) for v in range(5)]
    first = scene.add_ambi_voice(scene.add_buffer(stereo, oalgpu.FMT_FLOAT, frame_step=2), 2, True, position=STEREO["position"], frequency=44100)
    out = []
    for k, n in enumerate(TODO):
        moved = voices if k == 0 else voices[0::2]
        scene.set_source_props(moved, sc.props_array([_props(*_mono(v, k)) for v in moved]))
        if k == 0:
            src = cc.channel_source(_props(STEREO["gain"], STEREO["pos"], bl.RS_LINEAR, STEREO["pitch"], STEREO["gain_hf"]), cc.STEREO, cc.AUTO)
            scene.set_channel_sources(cc.sources_array([src], [[first, first + 1]]))
        scene.mix(n, post_process=True)
        out.append(scene.read_output(n, frame_step=2).reshape(n, 2).copy())
    got = np.concatenate(out)
    every = voices + [first, first + 1]
    states = [scene.voice_state(v) for v in every]
    gstate = [(s.play_state, s.position, s.position_frac) for s in states]
    nfc = [scene.voice_nfc(v)[0] for v in every]
    scene.close()
    assert gstate[:5] == wstate[:5] and gstate[5] == wstate[5] and gstate[6] == wstate[5], (gstate, wstate)
    # every voice is near-field compensated (VoiceFlag::HasNfc: CalcNormalPanning sets it on both of its legs), and what the
    # bridge reports of the reference's voice flags -- a buffer, not fading -- is what the library's voices show
    assert all(nfc), nfc
    for s, f in zip(states, wflags[:5] + [wflags[5], wflags[5]]):
        assert (1 if s.has_buffer else 0, 1 if s.fading else 0) == tuple(f[:2]), (f, s.has_buffer, s.fading)
    err = float(np.abs(got.astype(np.float64) - want).max())
    bound = 2e-5 * float(np.abs(want).max()) + 1e-7
    print("near-field device: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound, (err, bound)
    # the filter is audible: the same scene on the device without a control distance
    plain, pstate, _ = _reference(0.0, mono, stereo)
    assert pstate == wstate
    assert float(np.abs(plain - want).max()) > 1e-4
