"""3D source parameters computed on the GPU (oalgpu_voice_set_source_props, oalgpu_param_block_create_from_sources:
SourceParamsKernel, csrc/source_kernels.hip) against the reference side of tests/source_param_cases.py.

A / B on one device: context A is fed source properties only; context B gets oalgpu_voice_set_params + oalgpu_voice_set_pan
with the numpy restatement's results for the same sources.  After every update the voices' positions, fractions and play
states must be equal, the buses and the output within the project's sum tolerance (2e-5 max + 1e-7), gains and biquad
targets within the tolerances source_param_cases derives from the reference's own rounding noise."""
import os

import numpy as np
import pytest

import bridge_lib as bl
import oalgpu
import source_param_cases as sc
from oalgpu import synth

pytestmark = pytest.mark.gpu
MHR_PATH = os.path.join(bl.GOLDEN, "default_hrtf.mhr")
MHR = open(MHR_PATH, "rb").read()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(cfg, mode, nv, flags=0, output=True):
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    api = oalgpu.Api(mode, ctx_flags=flags)
    if cfg["hrtf"]:
        api.hrtf_load(MHR_PATH)
    s = oalgpu.Scene(api, sample_rate=cfg["sample_rate"], num_dry=cfg["num_dry"], num_real=cfg["num_real"], num_sends=cfg["num_sends"],
                     num_slots=cfg["num_slots"], wet_channels=cfg["wet_channels"], hrtf=cfg["hrtf"], max_voices=nv, max_buffers=8)
    if cfg["hrtf"]:
        if output:
            s.set_direct_hrtf_from_store(synth.AMBI_POINTS_1O, synth.AMBI_MATRIX_1O, synth.AMBI_ORDER_HF_GAIN_1O, 400.0)
    else:
        s.set_ambi_map(*cfg["dry_map"])
        if output:
            dec = np.zeros((cfg["num_real"], oalgpu.MAX_AMBI), np.float32)
            dec[0, :5] = [0.5, 0.288675135, 0.0552305643, 0.031, -0.017]
            dec[1, :5] = [0.5, -0.288675135, 0.0552305643, -0.031, -0.017]
            s.set_bformat_decoder(dec)
    lcg = synth.Lcg(0x5EED0053)
    bufs = [s.add_buffer(np.array([lcg.uniform(-1.0, 1.0) for _ in range(6000)], np.float32), oalgpu.FMT_FLOAT) for _ in range(4)]
    for v in range(nv):
        s.add_voice(bufs[v % 4], True, position=(v * 797) % 6000, frequency=cfg["frequency"])
    return s


def _set_env(scene, env, cfg):
    for i in range(cfg["num_slots"]):
        e = env[i]
        scene.set_slot_send_environment(i, e["active"], e["room_rolloff"], e["decay_time"], e["air_absorption_gain_hf"])


def _feed_b(scene, voices, srcs, lis, env, cfg):
    """context B: oalgpu_voice_set_params + oalgpu_voice_set_pan with the restatement's results"""
    arr = (oalgpu.VoiceParams * len(voices))()
    pans = []
    for i, s in enumerate(srcs):
        arr[i], pan = sc.voice_params(sc.calc(s, lis, env, cfg), s, cfg)
        pans.append(pan)
    scene.set_params_batch(voices, arr)
    scene.set_pan(voices, pans)


def _sum_close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bound = 2e-5 * float(np.abs(b).max()) + 1e-7
    err = float(np.abs(a - b).max())
    assert err <= bound, (what, err, bound)


def _compare(a, b, cfg, nv, samples, what):
    top = 0.0
    _sum_close(a.dry(), b.dry(), what + ": dry bus")
    top = max(top, float(np.abs(b.dry()).max()))
    for s in range(cfg["num_slots"]):
        _sum_close(a.wet(s), b.wet(s), what + ": wet bus %d" % s)
    if cfg["hrtf"]:
        _sum_close(a.hrtf_accum(), b.hrtf_accum(), what + ": HRTF accumulator")
        top = max(top, float(np.abs(b.hrtf_accum()).max()))
    _sum_close(a.read_output(samples), b.read_output(samples), what + ": output")
    assert top > 1e-4, what                                  # the comparison is not of silence
    for v in range(nv):
        x, y = a.voice_state(v), b.voice_state(v)
        assert (x.play_state, x.position, x.position_frac) == (y.play_state, y.position, y.position_frac), (what, v)
        gx, gy = np.array(x.dry_current[:cfg["num_dry"]]), np.array(y.dry_current[:cfg["num_dry"]])
        scale = max(1e-3, float(np.abs(gy).max()))
        assert float(np.abs(gx - gy).max()) <= sc.TOLERANCE["pan"] * scale, (what, v, gx, gy)
        for i in range(cfg["num_sends"]):
            wx, wy = np.array(x.send_current[i][:cfg["wet_channels"]]), np.array(y.send_current[i][:cfg["wet_channels"]])
            assert float(np.abs(wx - wy).max()) <= sc.TOLERANCE["pan"] * max(1e-3, float(np.abs(wy).max())), (what, v, i)
        if cfg["hrtf"]:
            assert abs(x.hrtf_old_gain - y.hrtf_old_gain) <= sc.TOLERANCE["gain"] * max(1e-3, abs(y.hrtf_old_gain)), (what, v)
            assert tuple(x.hrtf_old_delay) == tuple(y.hrtf_old_delay), (what, v)
        filters = [(x.direct_lp, y.direct_lp), (x.direct_hp, y.direct_hp)]
        filters += [(x.send_lp[i], y.send_lp[i]) for i in range(cfg["num_sends"])] + [(x.send_hp[i], y.send_hp[i]) for i in range(cfg["num_sends"])]
        for fx, fy in filters:
            for k in ("tb0", "tb1", "tb2", "ta1", "ta2"):
                p, q = getattr(fx, k), getattr(fy, k)
                assert abs(p - q) <= sc.TOLERANCE["coeff"] * max(1.0, abs(q)), (what, v, k, p, q)


def _cases(lis, env):
    kept, _ = sc.table(MHR)
    return [c for c in kept if c["lis"] == lis and c["env"] == env]


@pytest.mark.parametrize("mode", [oalgpu.MATH_FAST, oalgpu.MATH_EXACT], ids=["fast", "exact"])
@pytest.mark.parametrize("which,nv,samples", [("dry_lines", 96, 256), ("dry_lines", 320, 1024), ("hrtf", 64, 1024), ("hrtf", 160, 256)])
def test_source_props_against_resolved_parameters(which, nv, samples, mode):
    """three updates, a quarter of the voices with new source properties between them, the slots' environments changing with them"""
    cfg = sc.DRY_CFG if which == "dry_lines" else sc.HRTF_CFG
    a, b = _scene(cfg, mode, nv), _scene(cfg, mode, nv)
    lis = sc.LISTENERS[0]
    a.set_listener(sc.listener_struct(lis))
    for u in range(3):
        env = sc.ENVIRONMENTS[u % 2]
        cases = _cases(0, u % 2)
        voices = list(range(nv)) if u == 0 else [v for v in range(nv) if v % 4 == u % 4]
        srcs = [sc.for_cfg(cases[(v * 7 + u * 13) % len(cases)]["src"], cfg) for v in voices]
        _set_env(a, env, cfg)
        a.set_source_props(voices, sc.props_array(srcs))
        _feed_b(b, voices, srcs, lis, env, cfg)
        a.mix(samples, post_process=True); b.mix(samples, post_process=True)
        _compare(a, b, cfg, nv, samples, "%s update %d" % (which, u))
    a.close(); b.close()


def test_every_listener_and_context_distance_model():
    """the listeners whose context names the distance model, and the one that outruns sound: one update each"""
    cfg, nv = sc.DRY_CFG, 64
    a, b = _scene(cfg, oalgpu.MATH_FAST, nv), _scene(cfg, oalgpu.MATH_FAST, nv)
    for li in range(1, len(sc.LISTENERS)):
        lis, env = sc.LISTENERS[li], sc.ENVIRONMENTS[li % 2]
        cases = [c for c in sc.table(MHR)[0] if c["lis"] == li]
        assert cases, li
        voices = list(range(nv))
        srcs = [sc.for_cfg(cases[v % len(cases)]["src"], cfg) for v in voices]
        a.set_listener(sc.listener_struct(lis))
        _set_env(a, env, cfg)
        a.set_source_props(voices, sc.props_array(srcs))
        _feed_b(b, voices, srcs, lis, env, cfg)
        a.mix(256, post_process=True); b.mix(256, post_process=True)
        _compare(a, b, cfg, nv, 256, "listener %d" % li)
    a.close(); b.close()


def test_record_counts_and_a_voice_named_twice():
    """1, 63, 64, 65 and 300 records in one call; then a call and a block that name a voice twice: the last record wins"""
    cfg, nv = sc.DRY_CFG, 320
    a, b = _scene(cfg, oalgpu.MATH_FAST, nv), _scene(cfg, oalgpu.MATH_FAST, nv)
    lis, env = sc.LISTENERS[0], sc.ENVIRONMENTS[0]
    cases = _cases(0, 0)
    a.set_listener(sc.listener_struct(lis)); _set_env(a, env, cfg)
    allv = list(range(nv))
    first = [sc.for_cfg(cases[v % len(cases)]["src"], cfg) for v in allv]
    a.set_source_props(allv, sc.props_array(first)); _feed_b(b, allv, first, lis, env, cfg)
    for u, count in enumerate((1, 63, 64, 65, 300)):
        voices = [(v * 3 + u) % nv for v in range(count)]
        assert len(set(voices)) == count
        srcs = [sc.for_cfg(cases[(v * 11 + u * 5 + 1) % len(cases)]["src"], cfg) for v in voices]
        a.set_source_props(voices, sc.props_array(srcs)); _feed_b(b, voices, srcs, lis, env, cfg)
        a.mix(256, post_process=True); b.mix(256, post_process=True)
        _compare(a, b, cfg, nv, 256, "%d records" % count)
    twice = [5, 9, 5, 200, 9, 5]
    srcs = [sc.for_cfg(cases[(i * 17 + 3) % len(cases)]["src"], cfg) for i in range(len(twice))]
    a.set_source_props(twice, sc.props_array(srcs))
    _feed_b(b, [200, 9, 5], [srcs[3], srcs[4], srcs[5]], lis, env, cfg)
    a.mix(256, post_process=True); b.mix(256, post_process=True)
    _compare(a, b, cfg, nv, 256, "a call naming a voice twice")
    srcs = [sc.for_cfg(cases[(i * 19 + 8) % len(cases)]["src"], cfg) for i in range(len(twice))]
    blk = a.param_block_from_sources(twice, sc.props_array(srcs))
    a.apply_block(blk)
    _feed_b(b, [200, 9, 5], [srcs[3], srcs[4], srcs[5]], lis, env, cfg)
    a.mix(256, post_process=True); b.mix(256, post_process=True)
    _compare(a, b, cfg, nv, 256, "a block naming a voice twice")
    oalgpu.lib.oalgpu_param_block_destroy(blk)
    a.close(); b.close()


@pytest.mark.parametrize("which", ["dry_lines", "hrtf"])
def test_block_from_sources_equals_the_synchronous_call(which):
    """oalgpu_param_block_create_from_sources + oalgpu_param_block_apply against oalgpu_voice_set_source_props: buses and voice state
    bit for bit"""
    cfg, nv = (sc.DRY_CFG if which == "dry_lines" else sc.HRTF_CFG), 128
    a, b = _scene(cfg, oalgpu.MATH_FAST, nv), _scene(cfg, oalgpu.MATH_FAST, nv)
    lis, env = sc.LISTENERS[0], sc.ENVIRONMENTS[0]
    cases = _cases(0, 0)
    blocks = []
    for s in (a, b):
        s.set_listener(sc.listener_struct(lis)); _set_env(s, env, cfg)
    for u in range(3):
        voices = list(range(nv)) if u == 0 else [v for v in range(nv) if v % 4 == u]
        props = sc.props_array([sc.for_cfg(cases[(v * 5 + u * 3) % len(cases)]["src"], cfg) for v in voices])
        blocks.append(a.param_block_from_sources(voices, props))
        a.apply_block(blocks[-1])
        b.set_source_props(voices, props)
        a.mix(1024, post_process=True); b.mix(1024, post_process=True)
        assert np.array_equal(_bits(a.dry()), _bits(b.dry())), u
        for s in range(cfg["num_slots"]):
            assert np.array_equal(_bits(a.wet(s)), _bits(b.wet(s))), (u, s)
        if cfg["hrtf"]:
            assert np.array_equal(_bits(a.hrtf_accum()), _bits(b.hrtf_accum())), u
        assert np.abs(b.dry()).max() > 1e-4 or cfg["hrtf"]
        for v in range(0, nv, 7):
            x, y = a.voice_state(v), b.voice_state(v)
            assert (x.play_state, x.position, x.position_frac) == (y.play_state, y.position, y.position_frac), (u, v)
            assert np.array_equal(_bits(x.prev_samples), _bits(y.prev_samples)) and np.array_equal(_bits(x.dry_current), _bits(y.dry_current)), (u, v)
    for blk in blocks:
        oalgpu.lib.oalgpu_param_block_destroy(blk)
    a.close(); b.close()


def test_blocks_from_sources_through_the_resident_update_run():
    """a pipelined HRTF context with OALGPU_CTX_RESIDENT, its blocks made from source properties, driven by oalgpu_mix_update_run: the
    output equals the launched form's bit for bit (what test_gpu_pipeline.py claims for host-built blocks)"""
    cfg = dict(sc.HRTF_CFG, num_sends=0, num_slots=0)
    nv, updates = 2304, 6
    lis = sc.LISTENERS[0]
    cases = [c for c in _cases(0, 0) if not c["tag"].startswith("gain_mix_max")]

    def run(flags):
        s = _scene(cfg, oalgpu.MATH_FAST, nv, flags=flags)
        s.set_listener(sc.listener_struct(lis))
        allv = list(range(nv))
        s.set_source_props(allv, sc.props_array([sc.for_cfg(cases[v % len(cases)]["src"], cfg) for v in allv]))
        moving = [v for v in allv if v % 4 == 1]
        blocks = [s.param_block_from_sources(moving, sc.props_array([sc.for_cfg(cases[(v + 3 * u + 1) % len(cases)]["src"], cfg) for v in moving]))
                  for u in range(updates)]
        outs = []
        if flags:
            s.resident_set_short_run(0)
            tickets = []
            for u in range(updates):
                s.mix_run([blocks[u]], 1024, post_process=True)
                tickets.append(s.read_output_async())
                if u >= 2:                                  # (collected two updates late: three tickets may be outstanding)
                    outs.append(s.output_wait(tickets[u - 2]).copy())
            outs += [s.output_wait(t).copy() for t in tickets[-2:]]
        else:
            for u in range(updates):
                s.apply_block(blocks[u])
                s.mix(1024, post_process=True)
                t = s.read_output_async()
                outs.append(s.output_wait(t).copy())
        stats = s.resident_stats() if flags else None
        for blk in blocks:
            oalgpu.lib.oalgpu_param_block_destroy(blk)
        s.close()
        return outs, stats
    want, _ = run(0)
    got, stats = run(oalgpu.CTX_RESIDENT)
    assert stats["enabled"] == 1 and stats["failed"] == 0 and stats["updates"] == updates, stats     # the doorbell carried them
    for u in range(updates):
        assert np.array_equal(_bits(got[u]), _bits(want[u])), u
        assert np.abs(want[u]).max() > 1e-4


def test_refusals_leave_the_context_usable():
    cfg, nv = sc.DRY_CFG, 16
    s = _scene(cfg, oalgpu.MATH_FAST, nv, output=False)
    good = sc.for_cfg(sc.source(), cfg)
    one = sc.props_array([good])
    C = oalgpu.C
    u32 = (C.c_uint32 * 1)(3)
    L = oalgpu.lib
    L.oalgpu_voice_set_source_props.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.oalgpu_param_block_create_from_sources.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    blk = C.c_void_p()
    # null arguments
    assert L.oalgpu_voice_set_source_props(None, u32, one, 1) == -2
    assert L.oalgpu_voice_set_source_props(s.h, None, one, 1) == -2 and L.oalgpu_voice_set_source_props(s.h, u32, None, 1) == -2
    assert L.oalgpu_param_block_create_from_sources(s.h, u32, one, 1, None) == -2
    assert L.oalgpu_param_block_create_from_sources(s.h, u32, one, 0, C.byref(blk)) == -2
    # a voice index and a send slot out of range
    with pytest.raises(oalgpu.OalgpuError, match="bad voice index"):
        s.set_source_props([nv], one)
    bad = sc.source(); bad["send"][1][0] = cfg["num_slots"]
    for call in (s.set_source_props, s.param_block_from_sources):
        with pytest.raises(oalgpu.OalgpuError, match="send slot out of range"):
            call([3], sc.props_array([bad]))
    # a callback voice: its step is mirrored on the host
    s.add_callback_voice(np.zeros(4096, np.float32), oalgpu.FMT_FLOAT, voice=5)
    for call in (s.set_source_props, s.param_block_from_sources):
        with pytest.raises(oalgpu.OalgpuError, match="callback voices"):
            call([5], one)
    # the context still works
    s.set_state(5, 0)                                       # (Stopped: the callback voice never got a step)
    s.set_source_props([3], one)
    s.mix(256)
    assert np.abs(s.dry()).max() > 1e-4
    s.close()
    # a context with near-field control
    n = _scene(dict(cfg, num_sends=0, num_slots=0), oalgpu.MATH_FAST, 8, output=False)
    n.set_nfc(343.3 / (1.0 * 48000.0), [1, 2, 2])
    for call in (n.set_source_props, n.param_block_from_sources):
        with pytest.raises(oalgpu.OalgpuError, match="near-field control"):
            call([0], one)
    n.close()
    # an HRTF context without a data set
    api = oalgpu.Api(oalgpu.MATH_FAST)
    desc = sc.context_desc(sc.HRTF_CFG, max_voices=8)
    h = C.c_void_p()
    oalgpu.check(L.oalgpu_context_create(C.byref(desc), C.byref(h)), "oalgpu_context_create")
    hone = sc.props_array([sc.for_cfg(sc.source(), sc.HRTF_CFG)])
    assert L.oalgpu_voice_set_source_props(h, u32, hone, 1) == -4
    assert L.oalgpu_param_block_create_from_sources(h, u32, hone, 1, C.byref(blk)) == -4
    L.oalgpu_context_destroy(h)
