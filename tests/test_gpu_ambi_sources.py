"""Source parameters of B-Format sources computed on the GPU (oalgpu_voice_set_ambi_sources,
oalgpu_param_block_create_from_ambi_sources: AmbiParamsKernel, csrc/source_ambi_kernels.hip) against the host compilation of the
same arithmetic (oalgpu_ambi_source_params_host, which tests/test_ambi_sources_host.py holds against the numpy restatement).

A / B on one device: context A is fed ambisonic sources only; context B gets oalgpu_voice_set_params with the host compilation's
records, one per channel voice.  One source per group of ambi_source_cases.GROUPS, three updates of 1024 / 1024 / 700 frames
under the group's three spatialize modes with another orientation each, so that every gain ramps.  After every update the voices'
state (play state, position, fraction, the samples kept; the reached gains too where the route has no transcendental function)
must be equal and the buses within the project's sum tolerance, 2e-5 max + 1e-7."""
import numpy as np
import pytest

import ambi_source_cases as ac
import oalgpu
import source_param_cases as sc
from oalgpu import synth

pytestmark = pytest.mark.gpu
NO_VOICE = oalgpu.NO_VOICE
TODO = (1024, 1024, 700)
FRAMES = 6000


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(cfg, mode, sources, flags=0, missing=()):
    """a context of `cfg` told its order and given the upsamplers `sources` need, with one voice per channel of every source over
    channel views of an interleaved buffer; source i gets no voice for the channels in missing.get(i) -> (scene, voices per source)"""
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    api = oalgpu.Api(mode, ctx_flags=flags)
    total = sum(ac.channels_of(cs["order"], cs["is_2d"]) for cs in sources)
    s = oalgpu.Scene(api, sample_rate=cfg["sample_rate"], num_dry=cfg["num_dry"], num_real=cfg["num_real"], num_sends=cfg["num_sends"],
                     num_slots=cfg["num_slots"], wet_channels=cfg["wet_channels"], hrtf=False, max_voices=total + 8, max_buffers=total + 16)
    s.set_ambi_map(*cfg["dry_map"])
    s.set_ambi_order(cfg["ambi_order"], cfg["mix_2d"])
    for (order, is_2d), m in ac.upsamplers_for(cfg, sources).items():
        s.set_ambi_upsampler(order, is_2d, m)
    lcg = synth.Lcg(0x5EED0074)
    oalgpu.lib.oalgpu_buffer_channel_view.argtypes = [oalgpu.C.c_void_p, oalgpu.C.c_int, oalgpu.C.c_uint32]
    voices = []
    for i, cs in enumerate(sources):
        nch = ac.channels_of(cs["order"], cs["is_2d"])
        data = np.array([lcg.uniform(-1.0, 1.0) for _ in range(FRAMES * nch)], np.float32)
        buf = s.add_buffer(data, oalgpu.FMT_FLOAT, frame_step=nch)
        mine = []
        for ch in range(nch):
            if ch in dict(missing).get(i, ()):
                mine.append(NO_VOICE)
                continue
            view = oalgpu.lib.oalgpu_buffer_channel_view(s.h, buf, ch)
            oalgpu.check(min(view, 0), "oalgpu_buffer_channel_view")
            mine.append(s.add_voice(view, True, position=(i * 397 + 11) % FRAMES, frequency=cfg["frequency"]))
        voices.append(mine)
    return s, voices


def _set_env(scene, env, cfg):
    for i in range(cfg["num_slots"]):
        e = env[i]
        scene.set_slot_send_environment(i, e["active"], e["room_rolloff"], e["decay_time"], e["air_absorption_gain_hf"])


def _feed_host(scene, voices, css, lis, env, cfg):
    """context B: oalgpu_voice_set_params with the host compilation's record of every channel voice"""
    out, _, _ = ac.params_host(cfg, lis, env, css)
    ids, recs = [], []
    for i, mine in enumerate(voices):
        for ch, v in enumerate(mine):
            if v != NO_VOICE:
                ids.append(v); recs.append(out[i * oalgpu.MAX_AMBI_CHANNELS + ch])
    scene.set_params_batch(ids, (oalgpu.VoiceParams * len(ids))(*recs))


def _sum_close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bound = 2e-5 * float(np.abs(b).max()) + 1e-7
    err = float(np.abs(a - b).max())
    assert err <= bound, (what, err, bound)


def _state(s, v, gains=True):
    """where the voice is, what it holds of its buffer and -- gains -- the gains it has reached"""
    x = s.voice_state(v)
    out = (x.play_state, x.position, x.position_frac, _bits(x.prev_samples).tobytes())
    return out + ((_bits(x.dry_current).tobytes(), _bits(x.send_current).tobytes()) if gains else ())


def _group_cases(group):
    """the group's kept cases with two sends, one per spatialize mode as far as the nudge rule kept them (else with fewer sends)"""
    kept, _ = ac.table()
    out = []
    for mode in (ac.ON, ac.AUTO, ac.OFF):
        pool = sorted((c for c in kept if c["group"] == group and c["cs"]["spatialize"] == mode), key=lambda c: -c["sends"])
        if pool:
            out.append(pool[0])
    assert len(out) >= 2, group
    return out


@pytest.mark.parametrize("mode", [oalgpu.MATH_FAST, oalgpu.MATH_EXACT], ids=["fast", "exact"])
@pytest.mark.parametrize("group", list(ac.GROUPS))
def test_ambi_sources_against_host_fed_parameters(group, mode):
    cases = _group_cases(group)
    cfg = ac.device_cfg(cases[0]["dev"][0], cases[0]["dev"][1], 1 if cases[0]["dev"][0] == 4 else 2)      # (at most 32 mixing lines)
    lis, env = sc.LISTENERS[0], sc.ENVIRONMENTS[0]
    css = [ac.for_cfg(c["cs"], cfg) for c in cases]
    missing = {0: (ac.MISSING_CHANNEL,)} if group == "missing_voice" else {}
    a, voices = _scene(cfg, mode, css[:1], missing=missing)
    b, voices_b = _scene(cfg, mode, css[:1], missing=missing)
    assert voices == voices_b and (NO_VOICE in voices[0]) == (group == "missing_voice")
    for s in (a, b):
        s.set_listener(sc.listener_struct(lis)); _set_env(s, env, cfg)
    loud = 0.0
    for u, n in enumerate(TODO):
        cs = css[u % len(css)]
        a.set_ambi_sources(ac.sources_array([cs], voices))
        _feed_host(b, voices, [cs], lis, env, cfg)
        a.mix(n); b.mix(n)
        what = "%s update %d" % (group, u)
        _sum_close(a.dry(), b.dry(), what + ": dry bus")
        loud = max(loud, float(np.abs(b.dry()).max()))
        for k in range(cfg["num_slots"]):
            _sum_close(a.wet(k), b.wet(k), what + ": wet bus %d" % k)
        # (on the ON route the gains pass through pow / acos / asin, the device's against glibc's: not bit-identical; on the other
        # the reached gains are the targets, which host and device form alike)
        for v in voices[0]:
            if v != NO_VOICE:
                assert _state(a, v, not ac.attenuated(cs)) == _state(b, v, not ac.attenuated(cs)), (what, v)
    assert loud > 1e-4, group                               # the comparison is not of silence
    a.close(); b.close()


@pytest.mark.parametrize("how", ["apply", "run"])
def test_block_from_ambi_sources_equals_the_synchronous_call(how):
    """oalgpu_param_block_create_from_ambi_sources through oalgpu_param_block_apply and through oalgpu_mix_update_run against
    oalgpu_voice_set_ambi_sources, update by update: buses and every channel voice's state bit for bit.  Three sources of two
    formats in one call (ragged record offsets), one of them without one of its channel voices"""
    kept, _ = ac.table()
    pool = [c for c in kept if c["dev"] == (4, False) and c["sends"] >= 1]
    third = [c for c in pool if c["cs"]["order"] == 3][:4]
    fourth = [c for c in pool if c["cs"]["order"] == 4][:2]
    assert len(third) == 4 and len(fourth) == 2
    cfg = ac.device_cfg(4, False, 1)                        # (25 dry lines and one slot's 4: at most 32 mixing lines)
    lis, env = sc.LISTENERS[0], sc.ENVIRONMENTS[0]
    shape = [ac.for_cfg(c["cs"], cfg) for c in (third[0], fourth[0], third[1])]
    missing = {2: (ac.MISSING_CHANNEL,)}
    a, voices = _scene(cfg, oalgpu.MATH_FAST, shape, missing=missing)
    b, _ = _scene(cfg, oalgpu.MATH_FAST, shape, missing=missing)
    for s in (a, b):
        s.set_listener(sc.listener_struct(lis)); _set_env(s, env, cfg)
    arrs = []
    for u in range(3):
        css = [ac.for_cfg(c["cs"], cfg) for c in (third[u % 4], fourth[u % 2], third[(u + 1) % 4])]
        arrs.append(ac.sources_array(css, voices))
    blocks = [a.param_block_from_ambi_sources(arr) for arr in arrs]
    for u, n in enumerate(TODO):
        if how == "run":
            a.mix_run([blocks[u]], n)
        else:
            a.apply_block(blocks[u])
            a.mix(n)
        b.set_ambi_sources(arrs[u])
        b.mix(n)
        assert np.array_equal(_bits(a.dry()), _bits(b.dry())), u
        assert np.abs(b.dry()).max() > 1e-4
        for k in range(cfg["num_slots"]):
            assert np.array_equal(_bits(a.wet(k)), _bits(b.wet(k))), (u, k)
        for mine in voices:
            for v in mine:
                if v != NO_VOICE:
                    assert _state(a, v) == _state(b, v), (u, v)
    for blk in blocks:
        oalgpu.lib.oalgpu_param_block_destroy(blk)
    a.close(); b.close()


def test_refusals_leave_the_context_usable():
    cfg = ac.device_cfg(2, True, 2)
    good = ac.for_cfg(ac.ambi_source(sc.source(), 1, True), cfg)
    s, voices = _scene(cfg, oalgpu.MATH_FAST, [good, good])
    C, L = oalgpu.C, oalgpu.lib
    one = ac.sources_array([good], [voices[0]])
    blk = C.c_void_p()
    L.oalgpu_voice_set_ambi_sources.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.oalgpu_param_block_create_from_ambi_sources.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.oalgpu_voice_set_ambi_sources(None, one, 1) == -2 and L.oalgpu_voice_set_ambi_sources(s.h, None, 1) == -2
    assert L.oalgpu_param_block_create_from_ambi_sources(s.h, one, 1, None) == -2
    assert L.oalgpu_param_block_create_from_ambi_sources(s.h, one, 0, C.byref(blk)) == -2
    L.oalgpu_context_set_ambi_order.argtypes = [C.c_void_p, C.c_uint32, C.c_int32]
    assert L.oalgpu_context_set_ambi_order(s.h, 0, 0) == -2 and L.oalgpu_context_set_ambi_order(s.h, 5, 0) == -2
    with pytest.raises(oalgpu.OalgpuError, match="rows"):
        s.set_ambi_upsampler(2, False, ac.UPSAMPLERS[(1, False)])
    before = _bits(s.dry()).copy()
    calls = (s.set_ambi_sources, s.param_block_from_ambi_sources)

    def refused(match, css, vs):
        for call in calls:
            with pytest.raises(oalgpu.OalgpuError, match=match):
                call(ac.sources_array(css, vs))
    refused("bad voice index", [good], [[voices[0][0], 1000]])
    bad = sc.source(); bad["send"][1][0] = cfg["num_slots"]
    refused("send slot out of range", [dict(good, src=bad)], [voices[0]])
    refused("order, layout or scaling out of range", [dict(good, order=0)], [voices[0]])
    refused("order, layout or scaling out of range", [dict(good, order=5)], [voices[0]])
    refused("order, layout or scaling out of range", [dict(good, layout=-1)], [voices[0]])
    refused("order, layout or scaling out of range", [dict(good, scaling=3)], [voices[0]])
    refused("order, layout or scaling out of range", [dict(good, spatialize=-1)], [voices[0]])
    refused("needs an upsampler", [dict(good, is_2d=False)], [voices[0] + [voices[1][0]]])
    refused("a voice named twice", [good], [[voices[0][0], voices[0][0]]])
    refused("a voice named twice", [good, good], [voices[0], [voices[1][0], voices[0][1]]])
    refused("a source without a channel voice", [good], [[NO_VOICE] * 3])
    odd = s.add_voice(0, True, frequency=22050)
    refused("different frequencies", [good], [[voices[0][0], odd]])
    queue = s.add_queue_voice(0, True)
    refused("no frequency", [good], [[voices[0][0], queue]])
    cb = s.add_callback_voice(np.zeros(4096, np.float32), oalgpu.FMT_FLOAT)
    refused("callback voices", [good], [[voices[0][0], cb]])
    s.set_state(cb, 0); s.set_state(queue, 0); s.set_state(odd, 0)
    assert np.array_equal(_bits(s.dry()), before)
    # the context still works
    s.set_ambi_sources(ac.sources_array([good, good], voices))
    s.mix(256)
    assert np.abs(s.dry()).max() > 1e-4
    s.close()
    # a fourth-order device: FuMa reaches order 3
    cfg4 = ac.device_cfg(4, False, 0)
    f, fvoices = _scene(cfg4, oalgpu.MATH_FAST, [ac.ambi_source(sc.source(), 4, True)])
    for call in (f.set_ambi_sources, f.param_block_from_ambi_sources):
        with pytest.raises(oalgpu.OalgpuError, match="FuMa layout and scaling reach order 3"):
            call(ac.sources_array([ac.ambi_source(sc.source(), 4, True, layout=ac.FUMA)], fvoices))
    f.close()
    # a context that was not told its order
    api = oalgpu.Api(oalgpu.MATH_FAST)
    n = oalgpu.Scene(api, sample_rate=48000, num_dry=5, num_real=2, max_voices=8, max_buffers=8)
    nv = [n.add_voice(n.add_buffer(np.zeros(64, np.float32), oalgpu.FMT_FLOAT), True) for _ in range(3)]
    plain = ac.ambi_source(sc.source(), 1, True)
    for call in (n.set_ambi_sources, n.param_block_from_ambi_sources):
        with pytest.raises(oalgpu.OalgpuError, match="has not been told its ambisonic order"):
            call(ac.sources_array([plain], [nv]))
    # a context with near-field control
    n.set_ambi_order(1, True)
    n.set_nfc(343.3 / (1.0 * 48000.0), [1, 2, 2])
    for call in (n.set_ambi_sources, n.param_block_from_ambi_sources):
        with pytest.raises(oalgpu.OalgpuError, match="near-field control"):
            call(ac.sources_array([plain], [nv]))
    n.close()
    # an HRTF context, with a message that says why
    desc = sc.context_desc(sc.HRTF_CFG, max_voices=8)
    h = C.c_void_p()
    oalgpu.check(L.oalgpu_context_create(C.byref(desc), C.byref(h)), "oalgpu_context_create")
    hone = ac.sources_array([plain], [[0, 1, 2]])
    assert L.oalgpu_voice_set_ambi_sources(h, hone, 1) == -2
    assert "mix only through the FIR" in oalgpu.lib.oalgpu_last_error().decode()
    assert L.oalgpu_param_block_create_from_ambi_sources(h, hone, 1, C.byref(blk)) == -2
    L.oalgpu_context_destroy(h)
