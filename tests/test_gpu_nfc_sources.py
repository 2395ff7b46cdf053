"""Source parameters on near-field contexts (oalgpu_context_set_nfc + oalgpu_context_set_nfc_distance): the four source entry
points compute every voice's w0 and NfcFilter adjust on the GPU (SourceNfcKernel, ApplyNfcKernel: csrc/source_nfc_kernels.hip).

A / B on one device, the bridge's second-order 2D device (five dry lines, channels per order 1, 2, 2, control distance 1.5):
context A is fed source properties only; context B gets the records the host compilations produce (oalgpu_source_params_host /
oalgpu_channel_source_params_host through oalgpu_voice_set_params) and oalgpu_voice_set_nfc with
oalgpu_channel_source_nfc_host's w0 -- the path a host had to take before.  Eight voices, 20 000-sample buffers, updates of
1024 / 1024 / 700 / 1024 samples, the sources of tests/nfc_source_cases.py moving between them.  After every update: the
voices' positions and fractions equal, VoiceFlag::HasNfc set and the fourteen adjusted coefficients bit-identical in both, and
the buses compared as EXACT_BUSES says."""
import numpy as np
import pytest

import channel_source_cases as cc
import nfc_source_cases as nc
import oalgpu
import source_param_cases as sc

pytestmark = pytest.mark.gpu
NO_VOICE = oalgpu.NO_VOICE
TODO = (1024, 1024, 700, 1024)
CPO = [1, 2, 2]
AVG = nc.AVG_SPEAKER_DIST
FRAMES = 20000
LISTENER_OF_UPDATE = ("rotated", "plain", "scaled", "rotated_scaled")
ENV = [dict(active=1, room_rolloff=0.3, decay_time=1.49, air_absorption_gain_hf=0.9943)]
SEND = [0, 0.7, 1.0, 5000.0, 1.0, 250.0]

# The buses of A and B.  Both contexts run the same voice kernel on the same samples with bit-identical NFC coefficients and the
# same carried filter history, so they differ only where ChannelParamsKernel's / SourceParamsKernel's gains differ from the
# host compilation's in the last bit (the device math library against glibc: the stereo map's sin / cos, the wet path's pow).
# True: compared bit for bit; False: within the bound the channel-source GPU tests use for this comparison, 2e-5 max + 1e-7.
# Measured on the MI355X over every case of this file (116 bus comparisons, FAST and EXACT, with and without the send, 48 000 and
# 44 100 Hz): all bit-identical -- these scenes' gains pass through no function on which the two math libraries differ -- so the
# comparison is the exact one.
EXACT_BUSES = True


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cfg(sends, rate=48000):
    return dict(hrtf=False, sample_rate=rate, frequency=44100, num_dry=5, num_real=0, num_sends=sends, num_slots=sends, wet_channels=4,
                dry_map=([0, 1, 3, 4, 8], [1.0] * 5))


def _scene(cfg, mode, layouts, missing=(), distance=True):
    """a near-field context of `cfg` with one source per layout, a voice per channel but the (source, channel) pairs in `missing`
    -> (scene, voices per source)"""
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    api = oalgpu.Api(mode)
    s = oalgpu.Scene(api, sample_rate=cfg["sample_rate"], num_dry=cfg["num_dry"], num_real=cfg["num_real"], num_sends=cfg["num_sends"],
                     num_slots=cfg["num_slots"], wet_channels=cfg["wet_channels"], max_voices=8, max_buffers=24)
    s.set_ambi_map(*cfg["dry_map"])
    s.set_nfc(float(nc.device_w1(AVG, cfg["sample_rate"])), CPO)
    if distance:
        s.set_nfc_distance(AVG)
    for i in range(cfg["num_slots"]):
        s.set_slot_send_environment(i, ENV[i]["active"], ENV[i]["room_rolloff"], ENV[i]["decay_time"], ENV[i]["air_absorption_gain_hf"])
    rng = np.random.default_rng(0x5EED0077)
    bufs = {}
    for nch in sorted({oalgpu.SOURCE_CHANNEL_COUNT[l] for l in layouts}):
        bufs[nch] = s.add_buffer(rng.uniform(-1.0, 1.0, FRAMES * nch).astype(np.float32), oalgpu.FMT_FLOAT, frame_step=nch)
    oalgpu.lib.oalgpu_buffer_channel_view.argtypes = [oalgpu.C.c_void_p, oalgpu.C.c_int, oalgpu.C.c_uint32]
    voices = []
    for i, layout in enumerate(layouts):
        nch = oalgpu.SOURCE_CHANNEL_COUNT[layout]
        mine = []
        for ch in range(nch):
            if (i, ch) in missing:
                mine.append(NO_VOICE)
                continue
            view = bufs[nch] if nch == 1 else oalgpu.lib.oalgpu_buffer_channel_view(s.h, bufs[nch], ch)
            oalgpu.check(min(view, 0), "oalgpu_buffer_channel_view")
            mine.append(s.add_voice(view, True, position=(i * 997 + ch * 31) % FRAMES, frequency=cfg["frequency"]))
        voices.append(mine)
    assert s.nvoices == 8
    return s, voices


# the scenes: per source its layout, the channels without a voice, and the cases (by tag) it moves through
MONO_TAGS = ["at_listener_head_relative", "at_listener_world", "within_quarter_distance", "on_the_clamp_side_scaled", "ordinary",
             "ordinary_head_relative_rotated", "world_rotated", "nfc_scale_down"]
SCENES = {
    "mono8": [(cc.MONO, (), MONO_TAGS[i:] + MONO_TAGS[:i]) for i in range(8)],
    "x51_stereo": [(cc.X51, (), ["x51_with_lfe"]), (cc.STEREO, (), ["stereo_off", "nfc_scale_up", "stereo_auto"])],
    "x71_ragged": [(cc.X71, (3, 4, 5), ["x71_without_lfe_and_rears"]), (cc.MONO, (), ["mono_off", "ordinary", "within_quarter_distance"]),
                   (cc.STEREO, (), ["nfc_scale_up", "stereo_auto"])],
    "quad_monos": [(cc.QUAD, (), ["quad_near"]), (cc.STEREO, (), ["stereo_auto", "nfc_scale_up"]), (cc.MONO, (), ["at_listener_world", "ordinary"]),
                   (cc.MONO, (), ["within_quarter_distance", "world_rotated"])],
}
BY_TAG = {c[0]: c for c in nc.CASES}


def _sources(name, u, cfg):
    """the channel sources of scene `name` in update u: source i at its case u of its list, pushed outwards with u"""
    out = []
    for layout, _, tags in SCENES[name]:
        cs = BY_TAG[tags[u % len(tags)]][2]
        assert cs["channels"] == layout
        src = dict(cs["src"])
        src["position"] = [float(np.float32(x) * np.float32(1.0 + 0.5 * (u // len(tags)))) for x in src["position"]]
        src["gain"] = 0.25
        if cfg["num_sends"]:
            src["send"] = [list(SEND)] + [list(x) for x in src["send"][1:]]
        out.append(dict(cs, src=src))
    return out


def _layouts(name):
    return [l for l, _, _ in SCENES[name]], {(i, ch) for i, (_, miss, _) in enumerate(SCENES[name]) for ch in miss}


def _host_feed(b, cfg, lis, css, voices):
    """context B: the host compilations' records through oalgpu_voice_set_params, oalgpu_voice_set_nfc with the host function's w0
    -> {voice: the host function's fourteen coefficients}"""
    desc, ls = sc.context_desc(cfg), sc.listener_struct(lis)
    slots = sc.env_array(ENV, cfg) if cfg["num_slots"] else None
    arr = cc.sources_array(css)
    if all(cs["channels"] == cc.MONO and cs["spatialize"] != cc.OFF for cs in css):
        recs = oalgpu.source_params_host(desc, ls, sc.props_array([cs["src"] for cs in css]), cfg["frequency"], slots=slots, dry_map=cfg["dry_map"])
        rec_of = lambda i, ch: recs[i]
    else:
        recs = oalgpu.channel_source_params_host(desc, ls, arr, cfg["frequency"], slots=slots, dry_map=cfg["dry_map"])
        rec_of = lambda i, ch: recs[i * oalgpu.MAX_SOURCE_CHANNELS + ch]
    w0, coeffs = oalgpu.channel_source_nfc_host(desc, ls, arr, cfg["frequency"], AVG, slots=slots)
    ids, params, want = [], [], {}
    for i, mine in enumerate(voices):
        for ch, v in enumerate(mine):
            if v != NO_VOICE:
                ids.append(v); params.append(rec_of(i, ch)); want[v] = (float(w0[i]), coeffs[i])
    b.set_params_batch(ids, (oalgpu.VoiceParams * len(ids))(*params))
    for v in ids:
        b.set_voice_nfc(v, want[v][0])
    return {v: c for v, (_, c) in want.items()}


def _feed_a(a, name, css, voices):
    if name == "mono8":                                     # the mono entry point
        a.set_source_props([v[0] for v in voices], sc.props_array([cs["src"] for cs in css]))
    else:
        a.set_channel_sources(cc.sources_array(css, voices))


def _compare_buses(x, y, what, exact):
    x, y = np.asarray(x), np.asarray(y)
    same = np.array_equal(_bits(x), _bits(y))
    err = float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max())
    bound = 2e-5 * float(np.abs(y).max()) + 1e-7
    print("%s: %s, max err %.3e (bound %.3e)" % (what, "bit-identical" if same else "DIFFERENT BITS", err, bound))
    if exact:
        assert same, (what, err)
    assert err <= bound, (what, err, bound)


def _compare(a, b, cfg, voices, want, n, what, exact=None):
    exact = EXACT_BUSES if exact is None else exact
    _compare_buses(a.dry()[:, :n], b.dry()[:, :n], what + ": dry bus", exact)
    assert float(np.abs(b.dry()[:, :n]).max()) > 1e-3, what                 # not a comparison of silence
    for s in range(cfg["num_slots"]):
        _compare_buses(a.wet(s)[:, :n], b.wet(s)[:, :n], what + ": wet bus %d" % s, exact)
        assert float(np.abs(b.wet(s)[:, :n]).max()) > 1e-4, what
    for mine in voices:
        for v in mine:
            if v == NO_VOICE:
                continue
            x, y = a.voice_state(v), b.voice_state(v)
            assert (x.play_state, x.position, x.position_frac) == (y.play_state, y.position, y.position_frac), (what, v)
            (ha, ca), (hb, cb) = a.voice_nfc(v), b.voice_nfc(v)
            assert ha and hb, (what, v)
            assert np.array_equal(_bits(ca), _bits(cb)), (what, v, ca, cb)
            if want is not None:
                assert np.array_equal(_bits(ca), _bits(want[v])), (what, v, ca, want[v])


def _run_ab(name, mode, sends, rate=48000, feed_on=(0, 1, 2, 3)):
    cfg = _cfg(sends, rate)
    layouts, missing = _layouts(name)
    a, voices = _scene(cfg, mode, layouts, missing)
    b, voices_b = _scene(cfg, mode, layouts, missing)
    assert voices == voices_b
    branches = set()
    for u, n in enumerate(TODO):
        if u in feed_on:
            lis = nc.LISTENERS[LISTENER_OF_UPDATE[u]]
            css = _sources(name, u, cfg)
            branches |= {nc.expected(cs, lis, rate=rate)[2] for cs in css}
            a.set_listener(sc.listener_struct(lis))
            _feed_a(a, name, css, voices)
            want = _host_feed(b, cfg, lis, css, voices)
        a.mix(n); b.mix(n)
        _compare(a, b, cfg, voices, want, n, "%s update %d" % (name, u))
    a.close(); b.close()
    return branches


def test_a_near_field_context_with_its_distance_accepts_the_four_entry_points():
    """today they raise: "not for contexts with near-field control"; without oalgpu_context_set_nfc_distance they still do"""
    cfg = _cfg(0)
    layouts, missing = _layouts("quad_monos")
    css = _sources("quad_monos", 0, cfg)
    monos = [cs["src"] for cs in css[2:]]
    for distance in (False, True):
        s, voices = _scene(cfg, oalgpu.MATH_FAST, layouts, missing, distance=distance)
        mono_voices = [v[0] for v in voices[2:]]
        calls = [lambda: s.set_source_props(mono_voices, sc.props_array(monos)),
                 lambda: s.param_block_from_sources(mono_voices, sc.props_array(monos)),
                 lambda: s.set_channel_sources(cc.sources_array(css, voices)),
                 lambda: s.param_block_from_channel_sources(cc.sources_array(css, voices))]
        for call in calls:
            if distance:
                blk = call()
                if blk is not None:
                    oalgpu.lib.oalgpu_param_block_destroy(blk)
            else:
                with pytest.raises(oalgpu.OalgpuError, match="near-field control"):
                    call()
        if distance:
            assert all(s.voice_nfc(v)[0] for mine in voices for v in mine)
            # everything else stays refused
            with pytest.raises(oalgpu.OalgpuError, match="bad voice index"):
                s.set_source_props([1000], sc.props_array(monos[:1]))
            with pytest.raises(oalgpu.OalgpuError, match="a voice named twice"):
                s.set_channel_sources(cc.sources_array(css[2:], [voices[2], voices[2]]))
            s.mix(256)
            assert np.abs(s.dry()).max() > 1e-4
        else:
            assert not any(s.voice_nfc(v)[0] for mine in voices for v in mine)
        s.close()
    # the setter's own refusals: before oalgpu_context_set_nfc, and a distance that is none
    api = oalgpu.Api(oalgpu.MATH_FAST)
    plain = oalgpu.Scene(api, num_dry=5, max_voices=8, max_buffers=8)
    with pytest.raises(oalgpu.OalgpuError, match="oalgpu_context_set_nfc first"):
        plain.set_nfc_distance(1.5)
    plain.set_nfc(float(nc.device_w1(AVG, 48000)), CPO)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(oalgpu.OalgpuError, match="bad arguments"):
            plain.set_nfc_distance(bad)
    plain.set_nfc_distance(1.5); plain.set_nfc_distance(2.0)               # may be called again
    plain.close()


AB_CASES = ([(name, mode, sends) for name in ("mono8", "x51_stereo") for mode in ("fast", "exact") for sends in (0, 1)]
            + [(name, mode, sends) for name in ("x71_ragged", "quad_monos") for mode, sends in (("fast", 0), ("exact", 1))])


@pytest.mark.parametrize("name,mode,sends", AB_CASES, ids=["%s-%s-%dsend" % c for c in AB_CASES])
def test_source_properties_against_host_fed_parameters_and_set_nfc(name, mode, sends):
    branches = _run_ab(name, oalgpu.MATH_FAST if mode == "fast" else oalgpu.MATH_EXACT, sends)
    assert "identity" in branches and (name not in ("mono8", "x71_ragged", "quad_monos") or branches == {"identity", "clamp", "distance"}), branches


def test_source_properties_at_44100_hz():
    assert _run_ab("mono8", oalgpu.MATH_FAST, 0, rate=44100) == {"identity", "clamp", "distance"}


@pytest.mark.parametrize("name", ["mono8", "x51_stereo"])
def test_history_is_kept_when_a_source_moves_mid_stream(name):
    """the sources are set before update 0 and moved once, before update 2: NfcState::z is carried across the new coefficients as
    NfcFilter::adjust carries it, so the move produces no discontinuity the set_params + set_nfc path does not produce"""
    _run_ab(name, oalgpu.MATH_FAST, 0, feed_on=(0, 2))


def _same_state(a, b, cfg, voices, n, what):
    _compare(a, b, cfg, voices, None, n, what, exact=True)
    for mine in voices:
        for v in mine:
            if v == NO_VOICE:
                continue
            x, y = a.voice_state(v), b.voice_state(v)
            assert np.array_equal(_bits(x.prev_samples), _bits(y.prev_samples)) and np.array_equal(_bits(x.dry_current), _bits(y.dry_current)), (what, v)
            assert np.array_equal(_bits(x.send_current), _bits(y.send_current)), (what, v)


@pytest.mark.parametrize("how", ["apply", "run"])
@pytest.mark.parametrize("name", ["mono8", "x71_ragged"])
def test_blocks_equal_the_synchronous_calls(name, how):
    """oalgpu_param_block_create_from_sources (mono8) / _from_channel_sources through oalgpu_param_block_apply and through
    oalgpu_mix_update_run against the synchronous calls over four updates: buses, voice state and the voices' NFC coefficients
    bit for bit (both sides are the same kernels' results)"""
    cfg = _cfg(1)
    layouts, missing = _layouts(name)
    a, voices = _scene(cfg, oalgpu.MATH_FAST, layouts, missing)
    b, _ = _scene(cfg, oalgpu.MATH_FAST, layouts, missing)
    lis = sc.listener_struct(nc.LISTENERS["rotated"])
    a.set_listener(lis); b.set_listener(lis)
    per_update = [_sources(name, u, cfg) for u in range(len(TODO))]
    if name == "mono8":
        ids = [v[0] for v in voices]
        blocks = [a.param_block_from_sources(ids, sc.props_array([cs["src"] for cs in css])) for css in per_update]
    else:
        blocks = [a.param_block_from_channel_sources(cc.sources_array(css, voices)) for css in per_update]
    for u, n in enumerate(TODO):
        if how == "run":
            a.mix_run([blocks[u]], n)
        else:
            a.apply_block(blocks[u])
            a.mix(n)
        _feed_a(b, name, per_update[u], voices)
        b.mix(n)
        _same_state(a, b, cfg, voices, n, "%s %s update %d" % (name, how, u))
    for blk in blocks:
        oalgpu.lib.oalgpu_param_block_destroy(blk)
    a.close(); b.close()


def test_a_block_that_names_a_voice_twice_installs_the_last():
    cfg = _cfg(0)
    layouts, missing = _layouts("mono8")
    s, voices = _scene(cfg, oalgpu.MATH_FAST, layouts, missing)
    lis = nc.LISTENERS["plain"]
    s.set_listener(sc.listener_struct(lis))
    far = cc.channel_source(sc.source(position=[0.0, 0.0, -6.0]), cc.MONO, cc.ON)
    near = cc.channel_source(sc.source(position=[0.0, 0.0, -0.5]), cc.MONO, cc.ON)
    v, other = voices[0][0], voices[1][0]
    blk = s.param_block_from_sources([v, other, v], sc.props_array([far["src"], far["src"], near["src"]]))
    s.apply_block(blk)
    s.mix(256)
    has, got = s.voice_nfc(v)
    assert has and np.array_equal(_bits(got), _bits(nc.expected(near, lis)[1])), got
    has, got = s.voice_nfc(other)
    assert has and np.array_equal(_bits(got), _bits(nc.expected(far, lis)[1])), got
    assert not np.array_equal(_bits(nc.expected(near, lis)[1]), _bits(nc.expected(far, lis)[1]))
    # the synchronous call likewise
    s.set_source_props([other, other], sc.props_array([far["src"], near["src"]]))
    assert np.array_equal(_bits(s.voice_nfc(other)[1]), _bits(nc.expected(near, lis)[1]))
    oalgpu.lib.oalgpu_param_block_destroy(blk)
    s.close()
