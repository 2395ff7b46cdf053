"""The bs2b crossfeed (oalgpu_set_crossfeed) against the compiled reference's own bs2b_processor::cross_feed (core/bs2b.cpp).

The same stereo scene runs three times:
  (a) decoder on, the dedicated effect's gains zero: the real lines are the decoded feeds (adding to zero is exact);
  (b) decoder off, the dedicated effect on: the real lines are the direct signal;
  (c) decoder, dedicated effect and crossfeed on.
Bs2bPostProcess (alc/alu.cpp:407-434) keeps the direct signal out of the filter, so the expected lines of (c) are
cross_feed(decoded feeds of (a)) + direct lines of (b), bit for bit -- in EXACT contexts (serial post-process) and in FAST ones
(overlapped path), since the crossfeed is pinned on the GPU's own decoded feeds.  Updates are ragged."""
import numpy as np
import pytest

import bridge_lib as bl
import crossfeed_cases as cc
import limiter_cases as lc

pytestmark = pytest.mark.gpu


def _need():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    if not cc.available():
        pytest.skip("needs the compiled reference")


def _sizes(updates):
    return [cc.SIZES[k % len(cc.SIZES)] for k in range(updates)]


def _api(mode):
    import oalgpu
    return oalgpu.Api(oalgpu.MATH_EXACT if mode == "exact" else oalgpu.MATH_FAST)


def _check_kernel(scene, mode):
    """which voice kernel, and so which post-process path, ran: EXACT the serial one, FAST the overlapped one"""
    name = scene.voice_kernel_name()
    if mode == "exact":
        assert name == "VoiceMixKernel<true, LINES>", name
    else:
        assert name and not name.startswith("VoiceMixKernel"), name


def _run(mode, sizes, layout="stereo", rate=48000, decoder=True, level=None, dedicated="on", left=0, right=1, events=None,
         limiter=None, loud=1.0):
    """Every update's real lines (2 x n) of a fresh scene.  dedicated: "on", "zero" (the slot runs with zero gains) or None.
    events: {update: f(scene)} applied before that update."""
    gains = (0.0, 0.0) if dedicated == "zero" else ((0.7, -0.45) if left == 0 else (-0.45, 0.7))
    scene, fx, update = cc.build_scene(_api(mode), layout, rate, dedicated=dedicated is not None, dedicated_gains=gains,
                                       level=loud)
    nd = cc.LAYOUTS[layout]["num_dry"]
    if decoder:
        scene.set_bformat_decoder(*cc.decoder_matrices(layout, left, right))
    if level is not None:
        scene.set_crossfeed(level, left, right)
    if limiter is not None:
        scene.set_output_limiter(limiter)
    out = []
    for k, n in enumerate(sizes):
        if events and k in events:
            events[k](scene)
        update(k)
        scene.mix(n, post_process=True)
        out.append(np.array(scene.dry()[nd:, :n], np.float32))
    _check_kernel(scene, mode)
    scene.close()
    if fx is not None:
        fx.close()
    return out


def _expected(level, rate, decoded, direct, left=0, right=1, start=0):
    """cross_feed (fresh at update `start`) over the decoded feeds, + the direct lines.  The entries before `start` are not an
    expectation (without a crossfeed the decode accumulates onto the direct lines term by term): compare those updates with
    the plain run"""
    ref = cc.RefBs2b(level, rate)
    want = []
    for k, (a, b) in enumerate(zip(decoded, direct)):
        out = np.zeros_like(a)
        if k < start:
            fl, fr = a[left], a[right]
        else:
            fl, fr = ref.cross_feed(a[left], a[right])
        out[left] = cc.add_direct(fl, b[left] if b is not None else np.zeros_like(fl))
        out[right] = cc.add_direct(fr, b[right] if b is not None else np.zeros_like(fr))
        want.append(out)
    return want


def _equal_bits(got, want, tag, first=0):
    for k, (g, w) in enumerate(zip(got, want)):
        if k < first:
            continue
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (tag, k, float(np.abs(g - w).max()))


def _three_runs(mode, sizes, layout, rate, **kw):
    decoded = _run(mode, sizes, layout, rate, dedicated="zero", **kw)
    direct = _run(mode, sizes, layout, rate, decoder=False, **kw)
    assert max(float(np.abs(d).max()) for d in decoded) > 1e-2 and max(float(np.abs(d).max()) for d in direct) > 1e-2
    return decoded, direct


@pytest.mark.parametrize("rate", [44100, 48000])
@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("level", [1, 6])
def test_crossfeed_is_cross_feed_plus_direct_bit_for_bit(level, mode, rate):
    _need()
    sizes = _sizes(24)
    for layout in cc.LAYOUTS:
        decoded, direct = _three_runs(mode, sizes, layout, rate)
        got = _run(mode, sizes, layout, rate, level=level)
        _equal_bits(got, _expected(level, rate, decoded, direct), f"{mode} {layout} level {level} at {rate}")
        plain = _run(mode, sizes, layout, rate)                      # decoder and dedicated effect, no crossfeed
        assert any(not np.array_equal(g, p) for g, p in zip(got, plain))


@pytest.mark.parametrize("level", cc.LEVELS)
def test_every_level(level):
    _need()
    sizes = _sizes(24)
    decoded, direct = _three_runs("fast", sizes, "stereo", 48000)
    got = _run("fast", sizes, "stereo", 48000, level=level)
    _equal_bits(got, _expected(level, 48000, decoded, direct), f"level {level}")


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_without_a_dedicated_slot(mode):
    """silent direct lines: the crossfed lines are cross_feed of the decoder-only run's, exactly"""
    _need()
    sizes = _sizes(24)
    decoded = _run(mode, sizes, dedicated=None)
    got = _run(mode, sizes, dedicated=None, level=3)
    _equal_bits(got, _expected(3, 48000, decoded, [None] * len(sizes)), f"{mode} no slot")


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_left_and_right_lines_swapped(mode):
    """left = real line 1, right = real line 0: the layout is honoured (the two lines' histories and direct signals differ)"""
    _need()
    sizes = _sizes(24)
    decoded, direct = _three_runs(mode, sizes, "stereo dual band", 48000, left=1, right=0)
    got = _run(mode, sizes, "stereo dual band", 48000, level=2, left=1, right=0)
    _equal_bits(got, _expected(2, 48000, decoded, direct, left=1, right=0), f"{mode} swapped")
    # and it is the mirror image of the unswapped device
    straight = _run(mode, sizes, "stereo dual band", 48000, level=2)
    for k, (g, s) in enumerate(zip(got, straight)):
        assert np.array_equal(g[::-1].view(np.uint32), s.view(np.uint32)), k


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_removal_and_reinstall(mode):
    """removed: from that update on the lines are the plain decoder + dedicated run's, bit for bit; re-installed: cross_feed
    started fresh at that update"""
    _need()
    sizes = _sizes(20)
    decoded, direct = _three_runs(mode, sizes, "stereo", 48000)
    plain = _run(mode, sizes)
    removed = _run(mode, sizes, level=6, events={7: lambda s: s.set_crossfeed(None)})
    _equal_bits(removed, plain, f"{mode} removed", first=7)
    assert not np.array_equal(removed[3], plain[3])
    again = _run(mode, sizes, level=6, events={5: lambda s: s.set_crossfeed(None), 9: lambda s: s.set_crossfeed(4)})
    _equal_bits(again, plain[:9], f"{mode} off between", first=5)
    _equal_bits(again, _expected(4, 48000, decoded, direct, start=9), f"{mode} re-installed", first=9)
    later = _run(mode, sizes, events={6: lambda s: s.set_crossfeed(1)})
    _equal_bits(later, plain[:6], f"{mode} before the installation")
    _equal_bits(later, _expected(1, 48000, decoded, direct, start=6), f"{mode} installed at update 6", first=6)


def test_decoder_replaced_and_not_removed_while_set():
    """oalgpu_set_bformat_decoder with new matrices while a crossfeed is set: accepted, the filter histories kept; removing
    the decoder: refused until the crossfeed has gone"""
    import oalgpu
    _need()
    sizes = _sizes(16)
    hf, _ = cc.decoder_matrices("stereo")
    hf2 = hf * np.float32(0.8)

    def replace(s):
        with pytest.raises(oalgpu.OalgpuError):
            s.set_bformat_decoder(None)
        s.set_bformat_decoder(hf2)

    decoded = _run("exact", sizes, dedicated="zero", events={6: lambda s: s.set_bformat_decoder(hf2)})
    direct = _run("exact", sizes, decoder=False)
    got = _run("exact", sizes, level=5, events={6: replace})
    _equal_bits(got, _expected(5, 48000, decoded, direct), "decoder replaced")
    unchanged = _run("exact", sizes, level=5)
    assert not np.array_equal(got[8], unchanged[8])
    scene, fx, update = cc.build_scene(_api("fast"))
    scene.set_bformat_decoder(hf)
    scene.set_crossfeed(oalgpu.BS2B_LOW)
    scene.set_crossfeed(None)
    scene.set_bformat_decoder(None)                     # the decoder can go once the crossfeed has gone
    with pytest.raises(oalgpu.OalgpuError):
        scene.set_crossfeed(oalgpu.BS2B_LOW)
    scene.close()


def test_limiter_behind_the_crossfeed():
    """the limiter sees the crossfed lines: the reference Compressor over the expected lines, within the limiter tests' bound"""
    _need()
    if not lc.available():
        pytest.skip("needs the compiled reference")
    sizes = _sizes(24)
    params = lc.limiter_params(48000, "no automation")           # threshold -6 dB, 4:1: the scene drives it
    decoded, direct = _three_runs("fast", sizes, "stereo", 48000, loud=3.0)
    got = _run("fast", sizes, level=6, limiter=params, loud=3.0)
    want = _expected(6, 48000, decoded, direct)
    comp = lc.RefCompressor(params, 2)
    limited = [comp.process(w, w.shape[1]) for w in want]
    comp.close()
    top = np.max([np.abs(w).max(axis=1) for w in limited], axis=0)
    assert float(max(np.abs(w).max() for w in want)) > 0.5       # above the threshold
    for k, (g, w) in enumerate(zip(got, limited)):
        err = np.abs(g.astype(np.float64) - w).max(axis=1)
        assert np.all(err <= 1e-5 * top + 1e-30), (k, err, top)


def test_crossfed_pcm_matches_the_reference_output_stage():
    """oalgpu_read_output in s16: Write<short> of the reference (its bridge renders a stereo device's RealOut) on the expected
    lines"""
    import oalgpu
    _need()
    if not bl.available():
        pytest.skip("needs the reference bridge")
    sizes = _sizes(16)
    decoded, direct = _three_runs("fast", sizes, "stereo", 48000)
    want = _expected(6, 48000, decoded, direct)
    bridge = bl.Bridge(bl.MODE_CPU)
    bl.build_config1(bridge, nsources=1)
    scene, fx, update = cc.build_scene(_api("fast"), dedicated=True)
    scene.set_bformat_decoder(*cc.decoder_matrices("stereo"))
    scene.set_crossfeed(oalgpu.BS2B_HIGH_EASY)
    scene.set_output(oalgpu.OUT_I16, 0.0, 22222)
    for k, n in enumerate(sizes):
        update(k)
        scene.mix(n, post_process=True)
        lines = np.zeros((2, 1024), np.float32)
        lines[:, :n] = want[k]
        ref, _ = bridge.render_lines(lines, oalgpu.OUT_I16, 0.0, 22222, n, 2)
        got = scene.read_output(n, 2)
        assert np.array_equal(got, ref), k
    _check_kernel(scene, "fast")
    scene.close(); fx.close(); bridge.close()


def test_refused_arguments(synth_mhr):
    """every refusal leaves the context as it was: the run around them still matches"""
    import oalgpu
    _need()
    api = _api("fast")
    hf, _ = cc.decoder_matrices("stereo")
    # an HRTF context
    api.hrtf_load(synth_mhr)
    h = api.make_scene(num_dry=4, num_real=2, wet_channels=4, hrtf=True, max_voices=4)
    with pytest.raises(oalgpu.OalgpuError):
        h.set_crossfeed(oalgpu.BS2B_LOW)
    h.set_crossfeed(None)                               # (removing what is not there is no error)
    h.close()
    # no decoder set
    scene, fx, update = cc.build_scene(api)
    with pytest.raises(oalgpu.OalgpuError):
        scene.set_crossfeed(oalgpu.BS2B_LOW)
    scene.close()
    # a UHJ or TSME device: the encoder is the post-process
    u = api.make_scene(num_dry=3, num_real=2, wet_channels=4, hrtf=False, max_voices=4)
    u.set_uhj_encoder(oalgpu.UHJ_IIR)
    with pytest.raises(oalgpu.OalgpuError):
        u.set_crossfeed(oalgpu.BS2B_LOW)
    u.close()
    t = api.make_scene(num_dry=4, num_real=2, wet_channels=4, hrtf=False, max_voices=4)
    t.set_tsme_encoder(oalgpu.TSME_IIR)
    with pytest.raises(oalgpu.OalgpuError):
        t.set_crossfeed(oalgpu.BS2B_LOW)
    t.close()
    # a front stabilizer is set (three real lines), and the other way round
    s3 = api.make_scene(num_dry=3, num_real=3, wet_channels=4, hrtf=False, max_voices=4)
    hf3 = np.zeros((3, oalgpu.MAX_AMBI), np.float32)
    hf3[:2] = hf
    s3.set_bformat_decoder(hf3)
    s3.set_front_stabilizer(0, 1, 2, 5000.0 / 48000.0)
    with pytest.raises(oalgpu.OalgpuError):
        s3.set_crossfeed(oalgpu.BS2B_LOW)
    s3.set_front_stabilizer(None)
    s3.set_crossfeed(oalgpu.BS2B_LOW)
    with pytest.raises(oalgpu.OalgpuError):
        s3.set_front_stabilizer(0, 1, 2, 5000.0 / 48000.0)
    s3.close()
    # the level and line rules, and what a set crossfeed refuses, in the middle of a run
    sizes = _sizes(12)
    decoded, direct = _three_runs("exact", sizes, "stereo", 48000)

    def refusals(s):
        for bad in (-1, 7, 100):
            with pytest.raises(oalgpu.OalgpuError):
                s.set_crossfeed(bad)
        for bad in ((0, 0), (1, 1), (0, 2), (2, 1), (5, 9)):
            with pytest.raises(oalgpu.OalgpuError):
                s.set_crossfeed(oalgpu.BS2B_LOW, *bad)
        with pytest.raises(oalgpu.OalgpuError):
            s.set_bformat_decoder(None)                 # the crossfeed owns the decoder
        with pytest.raises(oalgpu.OalgpuError):
            s.set_uhj_encoder(oalgpu.UHJ_IIR)
        with pytest.raises(oalgpu.OalgpuError):
            s.set_tsme_encoder(oalgpu.TSME_IIR)
        with pytest.raises(oalgpu.OalgpuError):
            s.set_front_stabilizer(0, 1, 0, 5000.0 / 48000.0)

    got = _run("exact", sizes, level=2, events={4: refusals})
    _equal_bits(got, _expected(2, 48000, decoded, direct), "after refusals")
