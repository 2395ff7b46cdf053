"""The source parameter stage end to end against the compiled reference: the bridge in MODE_CPU renders test_bridge.py's scenes
(the stereo device; the HRTF device with a send into an EAX reverb slot) with the reference's own CalcVoiceParams, Voice::mix and
post-process; a library context set up like the device is fed ONLY source properties (oalgpu_voice_set_source_props) and must
reproduce the frames within the tolerance test_bridge.py uses for the same scenes, the sources' state exactly.

The stereo device's scene runs without a slot: the library's EAX reverb pans for first-order ACN lines in order (the HRTF
device's), not for the stereo device's 2D lines."""
import numpy as np
import pytest

import bridge_lib as bl
import oalgpu
import oracle_lib as ol
import source_param_cases as sc
from oalgpu import synth

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not bl.available(), reason="needs oracle/_ref/liboalbridge.so (built where /root/reference is mounted)")]


class Recorder:
    """stands in for bridge_lib.Bridge while bridge_lib's scene builders run: the buffers and the sources' properties they hand over"""

    def __init__(self):
        self.buffers, self.sources, self.updates = [], [], {}

    def add_buffer(self, data, loop_start=0, loop_end=None):
        self.buffers.append(np.ascontiguousarray(data, np.float32))
        return len(self.buffers) - 1

    def add_source_ex(self, buffer, looping, position, gain, pos, resampler, pitch, gain_hf, send_slot, send_gain, send_gain_hf):
        self.sources.append(dict(buffer=buffer, looping=looping, position=position))
        self.update_source_ex(len(self.sources) - 1, gain, pos, resampler, pitch, gain_hf, send_slot, send_gain, send_gain_hf)
        return len(self.sources) - 1

    def add_source(self, buffer, looping, position, gain, pos, resampler=bl.RS_LINEAR, pitch=1.0, gain_hf=1.0):
        return self.add_source_ex(buffer, looping, position, gain, pos, resampler, pitch, gain_hf, -1, 1.0, 1.0)

    def update_source_ex(self, source, gain, pos, resampler, pitch, gain_hf, send_slot, send_gain, send_gain_hf):
        s = sc.source(position=list(pos), gain=gain, pitch=pitch, resampler=resampler, direct=[1.0, gain_hf, 5000.0, 1.0, 250.0])
        if send_slot >= 0:
            s["send"][0] = [send_slot, send_gain, send_gain_hf, 5000.0, 1.0, 250.0]
        self.updates[source] = s                # FillProps: the defaults of a new AL source with these fields

    def update_source(self, source, gain, pos, resampler=bl.RS_LINEAR, pitch=1.0, gain_hf=1.0):
        self.update_source_ex(source, gain, pos, resampler, pitch, gain_hf, -1, 1.0, 1.0)

    def take(self):
        u, self.updates = self.updates, {}
        return sorted(u), [u[k] for k in sorted(u)]


def _run_library(scene, rec, todo, move):
    scene.set_listener(sc.listener_struct(sc.listener(distance_model=sc.INVERSE_CLAMPED)))      # the bridge's context (ref_bridge.cpp)
    handles = [scene.add_buffer(b, oalgpu.FMT_FLOAT) for b in rec.buffers]
    for s in rec.sources:
        scene.add_voice(handles[s["buffer"]], s["looping"], position=s["position"], frequency=44100)
    out = []
    for k, n in enumerate(todo):
        if k:
            move(k)
        voices, srcs = rec.take()
        if voices:
            scene.set_source_props(voices, sc.props_array(srcs))
        scene.mix(n, post_process=True)
        out.append(scene.read_output(n, frame_step=2).reshape(n, 2).copy())
    states = [scene.voice_state(v) for v in range(len(rec.sources))]
    return np.concatenate(out), [(s.play_state, s.position, s.position_frac) for s in states]


@pytest.mark.parametrize("mode", [oalgpu.MATH_FAST, oalgpu.MATH_EXACT], ids=["fast", "exact"])
def test_stereo_device_from_source_properties(mode):
    todo = (1024, 1024, 700, 1024, 1024)
    b = bl.Bridge(bl.MODE_CPU)
    srcs = bl.build_config1(b, filtered=True)
    want = []
    for k, n in enumerate(todo):
        if k:
            bl.move_some(b, srcs, k)
        want.append(b.render(n))
    want = np.concatenate(want)
    wstate = [b.source_state(v)[:3] for v in srcs]
    b.close()

    rec = Recorder()
    rsrcs = bl.build_config1(rec, filtered=True)
    scene = oalgpu.Scene(oalgpu.Api(mode), sample_rate=48000, num_dry=3, num_real=2, max_voices=64, max_buffers=16)
    scene.set_ambi_map([0, 1, 3], [1.0, 1.0, 1.0])                      # AmbiIndex::FromACN2D: W, Y, X
    dec = np.zeros((2, oalgpu.MAX_AMBI), np.float32)
    dec[0, :3] = [5.00000000e-1, 2.88675135e-1, 5.52305643e-2]
    dec[1, :3] = [5.00000000e-1, -2.88675135e-1, 5.52305643e-2]
    scene.set_bformat_decoder(dec, None, 400.0 / 48000.0)
    got, gstate = _run_library(scene, rec, todo, lambda k: bl.move_some(rec, rsrcs, k))
    scene.close()
    assert gstate == [tuple(s) for s in wstate]
    err = float(np.abs(got.astype(np.float64) - want).max())
    bound = 2e-5 * float(np.abs(want).max()) + 1e-7
    print("stereo device: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound, (err, bound)


def test_hrtf_device_with_a_reverb_slot_from_source_properties():
    todo = (1024, 1024, 640, 1024)
    nsources = 256
    b = bl.Bridge(bl.MODE_CPU, hrtf=True, num_sends=1)
    slot = b.add_reverb_slot(ol.ReverbProps.make(), 1.0)
    srcs = bl.build_config3(b, nsources, slot=slot)
    want = []
    for k, n in enumerate(todo):
        if k:
            bl.move_config3(b, srcs, k, slot=slot)
        want.append(b.render(n))
    want = np.concatenate(want)
    wstate = [b.source_state(v)[:3] for v in srcs]
    b.close()

    rec = Recorder()
    rsrcs = bl.build_config3(rec, nsources, slot=0)
    api = oalgpu.Api(oalgpu.MATH_FAST)
    api.hrtf_load(bl.GOLDEN + "/default_hrtf.mhr")
    scene = oalgpu.Scene(api, sample_rate=48000, num_dry=4, num_real=2, num_sends=1, num_slots=1, wet_channels=4, hrtf=True,
                         max_voices=nsources, max_buffers=16)
    scene.set_direct_hrtf_from_store(synth.AMBI_POINTS_1O, synth.AMBI_MATRIX_1O, synth.AMBI_ORDER_HF_GAIN_1O, 700.0)
    props = oalgpu.ReverbProps.make()
    rev = oalgpu.Reverb(4)
    rev.update(props, 1.0)
    scene.set_slot_reverb(0, rev)
    scene.set_slot_send_environment(0, True, props.room_rolloff_factor, props.decay_time, props.air_absorption_gain_hf)
    got, gstate = _run_library(scene, rec, todo, lambda k: bl.move_config3(rec, rsrcs, k, slot=0))
    scene.close()
    assert gstate == [tuple(s) for s in wstate], [(i, a, c) for i, (a, c) in enumerate(zip(gstate, wstate)) if a != tuple(c)][:4]
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("HRTF device: max err %.3e, bound %.3e" % (err, 4e-5 * scale + 1e-7))
    assert err <= 4e-5 * scale + 1e-7, (err, scale)       # (the FAST reverb's block scans against the reference's serial filters: test_bridge.py)
