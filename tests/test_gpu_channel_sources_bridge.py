"""The channel source stage end to end against the compiled reference: the bridge in MODE_CPU renders five mono sources and one
stereo source (spatialize Auto: CalcNonAttnVoiceParams, the stereo legs of CalcNormalPanning / CalcHrtfPanning) with the
reference's own CalcVoiceParams, Voice::mix and post-process, on the stereo device and on the HRTF device; a library context set
up like the device is fed ONLY source properties -- oalgpu_voice_set_source_props for the mono sources,
oalgpu_voice_set_channel_sources for the stereo source's two channel voices -- and must reproduce the frames within the bound
test_bridge.py uses for this scene, the sources' state exactly."""
import numpy as np
import pytest

import bridge_lib as bl
import channel_source_cases as cc
import oalgpu
import source_param_cases as sc
from oalgpu import synth

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not bl.available(), reason="needs oracle/_ref/liboalbridge.so (the compiled reference)")]
TODO = (1024, 1024, 700, 1024)
STEREO = dict(position=100, gain=0.3, pos=(0.5, 0.0, -1.0), pitch=1.07, gain_hf=0.8)


def _mono(v, k, hrtf):
    """source v in update k: (gain, position, resampler, pitch, gain_hf); the even ones move"""
    moved = k if v % 2 == 0 else 0
    return (0.2 + 0.01 * moved, (float(v - 2) * (1.0 - 0.1 * moved), 0.1 * moved, -2.0), bl.RS_BSINC24 if hrtf else bl.RS_LINEAR,
            1.0 + 0.05 * v, 0.5 if v == 1 else 1.0)


def _reference(hrtf, mono, stereo):
    b = bl.Bridge(bl.MODE_CPU, hrtf=hrtf, num_sends=0)
    try:
        bufs = [b.add_buffer(m) for m in mono]
        srcs = []
        for v in range(5):
            gain, pos, rs, pitch, gain_hf = _mono(v, 0, hrtf)
            srcs.append(b.add_source(bufs[v % 3], True, 997 * v, gain, pos, resampler=rs, pitch=pitch, gain_hf=gain_hf))
        st = b.add_source_stereo(b.add_buffer_interleaved(stereo, 2), True, STEREO["position"], STEREO["gain"], STEREO["pos"],
                                 resampler=bl.RS_LINEAR, pitch=STEREO["pitch"], gain_hf=STEREO["gain_hf"])
        out = []
        for k, n in enumerate(TODO):
            if k:
                for v in range(0, 5, 2):
                    gain, pos, rs, pitch, gain_hf = _mono(v, k, hrtf)
                    b.update_source(srcs[v], gain, pos, resampler=rs, pitch=pitch, gain_hf=gain_hf)
            out.append(b.render(n))
        return np.concatenate(out), [tuple(b.source_state(h)[:3]) for h in srcs + [st]]
    finally:
        b.close()


def _props(gain, pos, rs, pitch, gain_hf):
    return sc.source(position=list(pos), gain=gain, pitch=pitch, resampler=rs, direct=[1.0, gain_hf, 5000.0, 1.0, 250.0])


@pytest.mark.parametrize("hrtf", [False, True], ids=["stereo-device", "hrtf-device"])
def test_mono_and_stereo_sources_from_source_properties(hrtf):
    rng = np.random.default_rng(0xC0FFEE)
    mono = [rng.uniform(-1, 1, 20000).astype(np.float32) for _ in range(3)]
    stereo = rng.uniform(-1, 1, (9000, 2)).astype(np.float32)
    want, wstate = _reference(hrtf, mono, stereo)

    api = oalgpu.Api(oalgpu.MATH_FAST)
    if hrtf:
        api.hrtf_load(bl.GOLDEN + "/default_hrtf.mhr")
        scene = oalgpu.Scene(api, sample_rate=48000, num_dry=4, num_real=2, hrtf=True, max_voices=8, max_buffers=16)
        scene.set_direct_hrtf_from_store(synth.AMBI_POINTS_1O, synth.AMBI_MATRIX_1O, synth.AMBI_ORDER_HF_GAIN_1O, 700.0)
    else:
        scene = oalgpu.Scene(api, sample_rate=48000, num_dry=3, num_real=2, max_voices=8, max_buffers=16)
        scene.set_ambi_map([0, 1, 3], [1.0, 1.0, 1.0])                  # AmbiIndex::FromACN2D: W, Y, X
        dec = np.zeros((2, oalgpu.MAX_AMBI), np.float32)
        dec[0, :3] = [5.00000000e-1, 2.88675135e-1, 5.52305643e-2]
        dec[1, :3] = [5.00000000e-1, -2.88675135e-1, 5.52305643e-2]
        scene.set_bformat_decoder(dec, None, 400.0 / 48000.0)
    scene.set_listener(sc.listener_struct(sc.listener(distance_model=sc.INVERSE_CLAMPED)))      # the bridge's context (ref_bridge.cpp)
    handles = [scene.add_buffer(m, oalgpu.FMT_FLOAT) for m in mono]
    voices = [scene.add_voice(handles[v % 3], True, position=997 * v, frequency=44100) for v in range(5)]
    first = scene.add_ambi_voice(scene.add_buffer(stereo, oalgpu.FMT_FLOAT, frame_step=2), 2, True, position=STEREO["position"], frequency=44100)
    out = []
    for k, n in enumerate(TODO):
        moved = voices if k == 0 else voices[0::2]
        scene.set_source_props(moved, sc.props_array([_props(*_mono(v, k, hrtf)) for v in moved]))
        if k == 0:
            src = cc.channel_source(_props(STEREO["gain"], STEREO["pos"], bl.RS_LINEAR, STEREO["pitch"], STEREO["gain_hf"]), cc.STEREO, cc.AUTO)
            scene.set_channel_sources(cc.sources_array([src], [[first, first + 1]]))
        scene.mix(n, post_process=True)
        out.append(scene.read_output(n, frame_step=2).reshape(n, 2).copy())
    got = np.concatenate(out)
    states = [scene.voice_state(v) for v in voices + [first, first + 1]]
    gstate = [(s.play_state, s.position, s.position_frac) for s in states]
    scene.close()
    assert gstate[:5] == wstate[:5] and gstate[5] == wstate[5] and gstate[6] == wstate[5], (gstate, wstate)
    err = float(np.abs(got.astype(np.float64) - want).max())
    bound = 2e-5 * float(np.abs(want).max()) + 1e-7
    print("%s device: max err %.3e, bound %.3e" % ("HRTF" if hrtf else "stereo", err, bound))
    assert err <= bound, (err, bound)
