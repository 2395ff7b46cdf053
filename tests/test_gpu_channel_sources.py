"""Source parameters of multi-channel and non-spatialized sources computed on the GPU (oalgpu_voice_set_channel_sources,
oalgpu_param_block_create_from_channel_sources: ChannelParamsKernel, csrc/source_channel_kernels.hip) against the reference side
of tests/channel_source_cases.py.

A / B on one device: context A is fed channel sources only; context B gets oalgpu_voice_set_params with the numpy
restatement's records, one per channel voice.  After every update the voices' positions and fractions must be equal and the
buses (on HRTF contexts the accumulated output too) within the project's sum tolerance, 2e-5 max + 1e-7."""
import os

import numpy as np
import pytest

import bridge_lib as bl
import channel_source_cases as cc
import oalgpu
import source_param_cases as sc
from oalgpu import synth

pytestmark = pytest.mark.gpu
MHR_PATH = os.path.join(bl.GOLDEN, "default_hrtf.mhr")
MHR = open(MHR_PATH, "rb").read()
NO_VOICE = oalgpu.NO_VOICE
LFE_CHANNEL = 3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(cfg, mode, layouts, flags=0, without_lfe=()):
    """a context of `cfg` with one source per entry of `layouts`, one voice per channel over channel views of an interleaved buffer
    (as Scene.add_ambi_voice starts them); the sources in `without_lfe` get no voice for their LFE channel.  -> (scene, voices per source)"""
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    api = oalgpu.Api(mode, ctx_flags=flags)
    if cfg["hrtf"]:
        api.hrtf_load(MHR_PATH)
    total = sum(oalgpu.SOURCE_CHANNEL_COUNT[l] for l in layouts)
    s = oalgpu.Scene(api, sample_rate=cfg["sample_rate"], num_dry=cfg["num_dry"], num_real=cfg["num_real"], num_sends=cfg["num_sends"],
                     num_slots=cfg["num_slots"], wet_channels=cfg["wet_channels"], hrtf=cfg["hrtf"], max_voices=total + 8,
                     max_buffers=total + 16)
    if cfg["hrtf"]:
        s.set_direct_hrtf_from_store(synth.AMBI_POINTS_1O, synth.AMBI_MATRIX_1O, synth.AMBI_ORDER_HF_GAIN_1O, 400.0)
    else:
        s.set_ambi_map(*cfg["dry_map"])
    lcg = synth.Lcg(0x5EED0063)
    frames = 3000
    bufs = {}
    for nch in sorted(set(oalgpu.SOURCE_CHANNEL_COUNT)):
        data = np.array([lcg.uniform(-1.0, 1.0) for _ in range(frames * nch)], np.float32)
        bufs[nch] = s.add_buffer(data, oalgpu.FMT_FLOAT, frame_step=nch)
    oalgpu.lib.oalgpu_buffer_channel_view.argtypes = [oalgpu.C.c_void_p, oalgpu.C.c_int, oalgpu.C.c_uint32]
    voices = []
    for i, layout in enumerate(layouts):
        nch = oalgpu.SOURCE_CHANNEL_COUNT[layout]
        mine = []
        for ch in range(nch):
            if i in without_lfe and ch == LFE_CHANNEL:
                mine.append(NO_VOICE)
                continue
            view = bufs[nch] if nch == 1 else oalgpu.lib.oalgpu_buffer_channel_view(s.h, bufs[nch], ch)
            oalgpu.check(min(view, 0), "oalgpu_buffer_channel_view")
            mine.append(s.add_voice(view, True, position=(i * 397) % frames, frequency=cfg["frequency"]))
        voices.append(mine)
    return s, voices


def _set_env(scene, env, cfg):
    for i in range(cfg["num_slots"]):
        e = env[i]
        scene.set_slot_send_environment(i, e["active"], e["room_rolloff"], e["decay_time"], e["air_absorption_gain_hf"])


def _feed_b(scene, voices, css, lis, env, cfg):
    """context B: oalgpu_voice_set_params with the restatement's record of every channel voice"""
    ids, recs = [], []
    for mine, cs in zip(voices, css):
        base, channels = cc.calc(cs, lis, env, cfg)
        for v, ch in zip(mine, channels):
            if v != NO_VOICE:
                ids.append(v); recs.append(cc.voice_params(base, ch, cs["src"], cfg))
    arr = (oalgpu.VoiceParams * len(ids))(*recs)
    scene.set_params_batch(ids, arr)


def _sum_close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bound = 2e-5 * float(np.abs(b).max()) + 1e-7
    err = float(np.abs(a - b).max())
    assert err <= bound, (what, err, bound)


def _compare(a, b, cfg, voices, what):
    _sum_close(a.dry(), b.dry(), what + ": dry bus")
    top = float(np.abs(b.dry()).max())
    for s in range(cfg["num_slots"]):
        _sum_close(a.wet(s), b.wet(s), what + ": wet bus %d" % s)
        assert float(np.abs(b.wet(s)).max()) > 1e-4, (what, s)
    if cfg["hrtf"]:
        _sum_close(a.hrtf_accum(), b.hrtf_accum(), what + ": HRTF accumulator")
        top = max(top, float(np.abs(b.hrtf_accum()).max()))
    assert top > 1e-4, what                                  # the comparison is not of silence
    for mine in voices:
        for v in mine:
            if v == NO_VOICE:
                continue
            x, y = a.voice_state(v), b.voice_state(v)
            assert (x.play_state, x.position, x.position_frac) == (y.play_state, y.position, y.position_frac), (what, v)


def _cases(env, n, salt):
    """n kept cases of listener 0 and environment `env`, case i of layout i % 7 whatever the salt (the ceiling cases left out: their
    gain of 1000 would be the bound of every other voice)"""
    kept = [c for c in cc.table()[0] if c["lis"] == 0 and c["env"] == env and c["tag"] != "gain_mix_max"]
    by_layout = {l: [c for c in kept if c["cs"]["channels"] == l] for l in range(7)}
    out = []
    for i in range(n):
        pool = by_layout[i % 7]
        out.append(pool[(i * 5 + salt * 3) % len(pool)])
    return out


@pytest.mark.parametrize("mode", [oalgpu.MATH_FAST, oalgpu.MATH_EXACT], ids=["fast", "exact"])
@pytest.mark.parametrize("which", ["dry_lines", "hrtf"])
def test_channel_sources_against_host_fed_parameters(which, mode):
    """37 sources of all seven layouts in one call (ragged record offsets), among them a 5.1 source without an LFE voice and 5.1 /
    6.1 / 7.1 sources with one, which stays silent; then a call of one source; then a third of the sources: three 256-sample
    updates on the dry-line context with two sends and on the HRTF context with one"""
    cfg = sc.DRY_CFG if which == "dry_lines" else sc.HRTF_CFG
    lis = cc.LISTENERS[0]
    first = _cases(0, 37, 0)
    layouts = [c["cs"]["channels"] for c in first]
    assert set(layouts) == set(range(7))
    no_lfe = [i for i, l in enumerate(layouts) if l == cc.X51][:1]
    a, voices = _scene(cfg, mode, layouts, without_lfe=no_lfe)
    b, voices_b = _scene(cfg, mode, layouts, without_lfe=no_lfe)
    assert voices == voices_b and any(NO_VOICE in v for v in voices)
    a.set_listener(sc.listener_struct(lis))
    for u in range(3):
        env = sc.ENVIRONMENTS[u % 2]
        picked = list(range(37)) if u == 0 else ([11] if u == 1 else [i for i in range(37) if i % 3 == 1])
        pool = first if u == 0 else _cases(u % 2, 37, u)
        css = [cc.for_cfg(pool[i]["cs"], cfg) for i in picked]
        _set_env(a, env, cfg)
        a.set_channel_sources(cc.sources_array(css, [voices[i] for i in picked]))
        _feed_b(b, [voices[i] for i in picked], css, lis, env, cfg)
        a.mix(256, post_process=cfg["hrtf"]); b.mix(256, post_process=cfg["hrtf"])
        _compare(a, b, cfg, voices, "%s update %d" % (which, u))
    lfe = [mine[LFE_CHANNEL] for mine, l in zip(voices, layouts) if l >= cc.X51 and mine[LFE_CHANNEL] != NO_VOICE]
    assert len(lfe) >= 3
    for v in lfe:                                           # an LFE voice plays on and adds nothing
        st = a.voice_state(v)
        assert st.play_state == a.voice_state(v - 1).play_state and st.position == a.voice_state(v - 1).position, v
        assert st.hrtf_old_gain == 0.0 and not any(st.dry_current), v
        assert not any(any(row) for row in st.send_current), v
    a.close(); b.close()


@pytest.mark.parametrize("which", ["dry_lines", "hrtf"])
def test_mono_auto_equals_the_mono_stage_on_the_device(which):
    """MONO / AUTO through oalgpu_voice_set_channel_sources against oalgpu_voice_set_source_props: buses bit for bit"""
    cfg, nv = (sc.DRY_CFG if which == "dry_lines" else sc.HRTF_CFG), 64
    lis, env = sc.LISTENERS[0], sc.ENVIRONMENTS[0]
    cases = [c for c in sc.table(MHR)[0] if c["lis"] == 0 and c["env"] == 0 and not c["tag"].startswith("gain_mix_max")]
    a, voices = _scene(cfg, oalgpu.MATH_FAST, [cc.MONO] * nv)
    b, _ = _scene(cfg, oalgpu.MATH_FAST, [cc.MONO] * nv)
    for s in (a, b):
        s.set_listener(sc.listener_struct(lis)); _set_env(s, env, cfg)
    for u in range(2):
        srcs = [sc.for_cfg(cases[(v * 7 + u * 13) % len(cases)]["src"], cfg) for v in range(nv)]
        a.set_channel_sources(cc.sources_array([cc.channel_source(s, cc.MONO, cc.AUTO, (0.2, -0.9), -0.5) for s in srcs], voices))
        b.set_source_props([v[0] for v in voices], sc.props_array(srcs))
        a.mix(256, post_process=cfg["hrtf"]); b.mix(256, post_process=cfg["hrtf"])
        assert np.array_equal(_bits(a.dry()), _bits(b.dry())), u
        for s in range(cfg["num_slots"]):
            assert np.array_equal(_bits(a.wet(s)), _bits(b.wet(s))), (u, s)
        if cfg["hrtf"]:
            assert np.array_equal(_bits(a.hrtf_accum()), _bits(b.hrtf_accum())), u
            assert np.abs(b.hrtf_accum()).max() > 1e-4
        else:
            assert np.abs(b.dry()).max() > 1e-4
    a.close(); b.close()


def _same_bits(a, b, cfg, voices, what):
    """buses, output and the state of EVERY channel voice (a wrong place in the ragged record order would show in a later channel)"""
    assert np.array_equal(_bits(a.dry()), _bits(b.dry())), what
    for s in range(cfg["num_slots"]):
        assert np.array_equal(_bits(a.wet(s)), _bits(b.wet(s))), (what, s)
        assert np.abs(b.wet(s)).max() > 1e-4
    if cfg["hrtf"]:
        assert np.array_equal(_bits(a.read_output(256)), _bits(b.read_output(256))), what
        assert np.abs(b.read_output(256)).max() > 1e-4
    else:
        assert np.abs(b.dry()).max() > 1e-4
    for mine in voices:
        for v in mine:
            x, y = a.voice_state(v), b.voice_state(v)
            assert (x.play_state, x.position, x.position_frac) == (y.play_state, y.position, y.position_frac), (what, v)
            assert np.array_equal(_bits(x.prev_samples), _bits(y.prev_samples)) and np.array_equal(_bits(x.dry_current), _bits(y.dry_current)), (what, v)
            assert np.array_equal(_bits(x.send_current), _bits(y.send_current)), (what, v)
            if cfg["hrtf"]:
                assert _bits([x.hrtf_old_gain])[0] == _bits([y.hrtf_old_gain])[0] and tuple(x.hrtf_old_delay) == tuple(y.hrtf_old_delay), (what, v)
                assert np.array_equal(_bits(x.hrtf_history), _bits(y.hrtf_history)), (what, v)


UPDATES = 5


def _block_scenes(cfg, flags, flags_b=0):
    """context A (blocks) and B (synchronous calls) with 24 sources of all layouts, and per update the sources that move"""
    lis, env = cc.LISTENERS[0], sc.ENVIRONMENTS[0]
    layouts = [c["cs"]["channels"] for c in _cases(0, 24, 1)]
    a, voices = _scene(cfg, oalgpu.MATH_FAST, layouts, flags=flags)
    b, _ = _scene(cfg, oalgpu.MATH_FAST, layouts, flags=flags_b)
    for s in (a, b):
        s.set_listener(sc.listener_struct(lis)); _set_env(s, env, cfg)
    arrs = []
    for u in range(UPDATES):
        picked = list(range(24)) if u == 0 else [i for i in range(24) if i % 3 == u % 3]
        later = _cases(0, 24, 1 + u)
        arrs.append(cc.sources_array([cc.for_cfg(later[i]["cs"], cfg) for i in picked], [voices[i] for i in picked]))
    return a, b, voices, arrs


@pytest.mark.parametrize("which,how", [("dry_lines", "apply"), ("dry_lines", "run"), ("hrtf", "apply"), ("hrtf", "run")])
def test_block_from_channel_sources_equals_the_synchronous_call(which, how):
    """oalgpu_param_block_create_from_channel_sources through oalgpu_param_block_apply and through oalgpu_mix_update_run against
    oalgpu_voice_set_channel_sources, update by update: buses, output and every channel voice's state bit for bit"""
    cfg = sc.DRY_CFG if which == "dry_lines" else sc.HRTF_CFG
    a, b, voices, arrs = _block_scenes(cfg, 0)
    blocks = [a.param_block_from_channel_sources(arr) for arr in arrs]
    for u in range(3):
        if how == "run":
            a.mix_run([blocks[u]], 256, post_process=cfg["hrtf"])
        else:
            a.apply_block(blocks[u])
            a.mix(256, post_process=cfg["hrtf"])
        b.set_channel_sources(arrs[u])
        b.mix(256, post_process=cfg["hrtf"])
        _same_bits(a, b, cfg, voices, "update %d" % u)
    for blk in blocks:
        oalgpu.lib.oalgpu_param_block_destroy(blk)
    a.close(); b.close()


@pytest.mark.parametrize("how", ["apply", "run"])
@pytest.mark.parametrize("which", ["one_send_wave_pairs", "no_sends"])
def test_block_from_channel_sources_installed_by_the_voice_kernel(which, how):
    """a pipelined HRTF context (OALGPU_CTX_APPLY_IN_VOICE_KERNEL): oalgpu_mix_update is submitted with the NEXT call on the
    context, and when that call applies a block the update's own voice kernel installs the block's records, so the kernel's
    epilogue reads what ChannelParamsKernel wrote.  For that the blocks exist before the first update (creating one submits a
    deferred update without a block) and nothing reads the context between the updates (a read submits it too): blocks 1 .. 4 ride
    in the voice kernels of updates 0 .. 3.  Two kernels install records: the two-voices-per-wavefront kernel (with the send:
    OALGPU_CTX_WAVE_PAIRS, since an HRTF context with sends otherwise runs the voice-per-wavefront kernel with a row mixer, which
    does not) and the voice-per-wavefront kernel without sends.  The path leaves no trace outside the library; what can be
    asserted is what the library checks before it takes it -- the flag, FAST, a voice kernel that installs records -- and that
    the end state equals the synchronous form's bit for bit."""
    cfg = sc.HRTF_CFG if which == "one_send_wave_pairs" else dict(sc.HRTF_CFG, num_sends=0, num_slots=0)
    pairs = oalgpu.CTX_WAVE_PAIRS if which == "one_send_wave_pairs" else 0
    a, b, voices, arrs = _block_scenes(cfg, oalgpu.CTX_APPLY_IN_VOICE_KERNEL | pairs, pairs)
    name = a.voice_kernel_name()
    assert name.startswith("VoiceWave") and "sends" not in name and name == b.voice_kernel_name(), name     # WaveKernelAppliesRecords
    blocks = [a.param_block_from_channel_sources(arr) for arr in arrs]
    if how == "run":
        a.mix_run(blocks, 256, post_process=True)
    else:
        for u in range(UPDATES):
            a.apply_block(blocks[u])
            a.mix(256, post_process=True)
    for u in range(UPDATES):
        b.set_channel_sources(arrs[u])
        b.mix(256, post_process=True)
    _same_bits(a, b, cfg, voices, "%s %s (%s)" % (which, how, name))
    for blk in blocks:
        oalgpu.lib.oalgpu_param_block_destroy(blk)
    a.close(); b.close()


def test_refusals_leave_the_context_usable():
    cfg = sc.DRY_CFG
    s, voices = _scene(cfg, oalgpu.MATH_FAST, [cc.STEREO, cc.X51, cc.MONO])
    C, L = oalgpu.C, oalgpu.lib
    good = cc.for_cfg(cc.channel_source(sc.source(), cc.STEREO), cfg)
    one = cc.sources_array([good], [voices[0]])
    blk = C.c_void_p()
    L.oalgpu_voice_set_channel_sources.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.oalgpu_param_block_create_from_channel_sources.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.oalgpu_voice_set_channel_sources(None, one, 1) == -2 and L.oalgpu_voice_set_channel_sources(s.h, None, 1) == -2
    assert L.oalgpu_param_block_create_from_channel_sources(s.h, one, 1, None) == -2
    assert L.oalgpu_param_block_create_from_channel_sources(s.h, one, 0, C.byref(blk)) == -2
    calls = (s.set_channel_sources, s.param_block_from_channel_sources)

    def refused(match, css, vs):
        for call in calls:
            with pytest.raises(oalgpu.OalgpuError, match=match):
                call(cc.sources_array(css, vs))
    refused("bad voice index", [good], [[voices[0][0], 1000]])
    bad = sc.source(); bad["send"][1][0] = cfg["num_slots"]
    refused("send slot out of range", [cc.channel_source(bad, cc.STEREO)], [voices[0]])
    bad = sc.source(resampler=10)
    refused("resampler, distance model or send slot out of range", [cc.channel_source(bad, cc.STEREO)], [voices[0]])
    refused("channels or spatialize out of range", [dict(good, channels=7)], [voices[0]])
    refused("channels or spatialize out of range", [dict(good, spatialize=-1)], [voices[0]])
    refused("a voice named twice", [good], [[voices[0][0], voices[0][0]]])
    refused("a voice named twice", [good, good], [voices[0], [voices[2][0], voices[0][1]]])
    refused("a source without a channel voice", [good], [[NO_VOICE, NO_VOICE]])
    # channel voices of one source with different frequencies, and one without a frequency
    odd = s.add_voice(0, True, frequency=22050)
    refused("different frequencies", [good], [[voices[0][0], odd]])
    queue = s.add_queue_voice(0, True)
    refused("no frequency", [good], [[voices[0][0], queue]])
    cb = s.add_callback_voice(np.zeros(4096, np.float32), oalgpu.FMT_FLOAT)
    refused("callback voices", [good], [[voices[0][0], cb]])
    # the context still works
    s.set_state(cb, 0); s.set_state(queue, 0); s.set_state(odd, 0)
    s.set_channel_sources(cc.sources_array([good, cc.for_cfg(cc.channel_source(sc.source(), cc.X51), cfg)], [voices[0], voices[1]]))
    s.mix(256)
    assert np.abs(s.dry()).max() > 1e-4
    s.close()
    # a context with near-field control
    n, nvoices = _scene(dict(cfg, num_sends=0, num_slots=0), oalgpu.MATH_FAST, [cc.STEREO])
    n.set_nfc(343.3 / (1.0 * 48000.0), [1, 2, 2])
    for call in (n.set_channel_sources, n.param_block_from_channel_sources):
        with pytest.raises(oalgpu.OalgpuError, match="near-field control"):
            call(cc.sources_array([good], [nvoices[0]]))
    n.close()
    # an HRTF context without a data set
    api = oalgpu.Api(oalgpu.MATH_FAST)
    desc = sc.context_desc(sc.HRTF_CFG, max_voices=8)
    h = C.c_void_p()
    oalgpu.check(L.oalgpu_context_create(C.byref(desc), C.byref(h)), "oalgpu_context_create")
    hone = cc.sources_array([cc.for_cfg(good, sc.HRTF_CFG)], [[0, 1]])
    assert L.oalgpu_voice_set_channel_sources(h, hone, 1) == -4
    assert L.oalgpu_param_block_create_from_channel_sources(h, hone, 1, C.byref(blk)) == -4
    L.oalgpu_context_destroy(h)
