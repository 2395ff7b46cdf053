"""The stereo TSME encoder (oalgpu_set_tsme_encoder) against the compiled reference's own TsmeEncoderIIR / TsmeEncoder<256> /
TsmeEncoder<512> (core/tsmefilter.cpp).

Two contexts run the same TSME device scene (4 dry lines W, Y, Z, X; 2 real lines; voices panned over the sphere, so Z carries
signal), one without the encoder and one with it.  Every update's plain W / Y / Z / X and real lines go through the reference
encoder, and the encoded context's real lines must match it: IIR bit for bit, FIR within tsme_cases.FIR_GPU_BOUND = 1.453e-6
of the run's line maximum.  That bound is ten times the 1.453e-7 by which a float64 direct-FIR restatement differs from the
reference on the CPU (tests/test_tsme_host.py: the rounding of the reference's own float32 FFT path).  The GPU sums the same
response directly in double, so it cannot sit closer to the reference than that; the factor absorbs the difference between
scenes.  The dry lines stay as they were.  Updates are ragged.  EXACT contexts post-process serially, FAST ones on the
overlapped path (wavefront voice kernel, post stream).

Measured on one MI355X (worst |err| / line max over the parametrised runs): FIR-256 1.478e-7, FIR-512 1.150e-7 (the
bound: 1.453e-6); IIR bit-identical."""
import numpy as np
import pytest

import bridge_lib as bl
import crossfeed_cases as cc
import limiter_cases as lc
import tsme_cases as tc

SIZES = (1024, 17, 47, 128, 129, 1000, 1, 1024)
QUALITIES = {"iir": 0, "fir256": 1, "fir512": 2}
ND = 4
pytestmark = pytest.mark.gpu


def _need():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    if not tc.available():
        pytest.skip("needs the compiled reference")


def _sizes(updates):
    return [SIZES[k % len(SIZES)] for k in range(updates)]


def _api(mode):
    import oalgpu
    return oalgpu.Api(oalgpu.MATH_EXACT if mode == "exact" else oalgpu.MATH_FAST)


def _check_kernel(sc, mode):
    """which voice kernel, and so which post-process path, ran: EXACT the serial one, FAST the overlapped one"""
    name = sc.voice_kernel_name()
    if mode == "exact":
        assert name == "VoiceMixKernel<true, LINES>", name
    else:
        assert name and not name.startswith("VoiceMixKernel"), name


def _run(mode, sizes, quality=None, dedicated=False, events=None, limiter=None, level=1.0):
    """Every update's bus lines (6 x n) of a fresh TSME scene.  events: {update: quality or None} applied before that
    update (set_tsme_encoder)."""
    sc, fx, update = tc.build_scene(_api(mode), dedicated=dedicated, level=level)
    if quality is not None:
        sc.set_tsme_encoder(quality)
    if limiter is not None:
        sc.set_output_limiter(limiter)
    out = []
    for k, n in enumerate(sizes):
        if events and k in events:
            sc.set_tsme_encoder(events[k])
        update(k)
        sc.mix(n, post_process=True)
        out.append(np.array(sc.dry()[:, :n], np.float32))
    _check_kernel(sc, mode)
    sc.close()
    if fx is not None:
        fx.close()
    return out


def _reference(quality, plain, start=0):
    """the reference encoder (fresh at update `start`) over the plain context's lines: the real lines it returns"""
    enc = tc.RefTsmeEncoder(quality)
    want = []
    for k, p in enumerate(plain):
        if k < start:
            want.append(None)
            continue
        left, right = enc.encode(p[0], p[1], p[2], p[3], p[4], p[5])
        want.append(np.stack([left, right]))
    return want


def _compare(quality, got, want, plain, tag):
    top = max(float(np.abs(w).max()) for w in want if w is not None)
    assert top > 1e-2, tag
    worst = 0.0
    for k, (g, w, p) in enumerate(zip(got, want, plain)):
        if w is None:
            continue
        assert np.array_equal(g[:ND].view(np.uint32), p[:ND].view(np.uint32)), (tag, k)   # the dry lines stay as they were
        if quality == 0:
            assert np.array_equal(g[ND:].view(np.uint32), w.view(np.uint32)), (tag, k, float(np.abs(g[ND:] - w).max()))
        else:
            worst = max(worst, float(np.abs(g[ND:].astype(np.float64) - w).max()) / top)
    print(f"{tag}: line max {top:.3f}, worst |err| / line max {worst:.3e} (bound {tc.FIR_GPU_BOUND:.3e})")
    assert worst <= tc.FIR_GPU_BOUND, (tag, worst, top)
    return worst


@pytest.mark.parametrize("quality", list(QUALITIES))
@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("dedicated", [False, True], ids=["silent real lines", "dedicated slot"])
def test_encoder_matches_the_reference(mode, quality, dedicated):
    _need()
    q = QUALITIES[quality]
    sizes = _sizes(24)
    plain = _run(mode, sizes, dedicated=dedicated)
    got = _run(mode, sizes, q, dedicated=dedicated)
    assert max(float(np.abs(p[2]).max()) for p in plain) > 1e-2             # Z carries signal
    if dedicated:
        assert max(float(np.abs(p[ND:]).max()) for p in plain) > 1e-2       # the direct input is not silent
    else:
        assert all(not np.any(p[ND:]) for p in plain)
    _compare(q, got, _reference(q, plain), plain, f"{mode} {quality} {'dedicated' if dedicated else 'silent'}")


@pytest.mark.parametrize("quality", list(QUALITIES))
def test_limiter_behind_the_encoder(quality):
    """the limiter sees the encoded lines: the reference Compressor of the reference encode, within the limiter tests' bound"""
    _need()
    if not lc.available():
        pytest.skip("needs the compiled reference")
    q = QUALITIES[quality]
    sizes = _sizes(24)
    params = lc.limiter_params(48000, "no automation")           # threshold -6 dB, 4:1: the scene drives it
    plain = _run("fast", sizes, dedicated=True, level=2.0)
    got = _run("fast", sizes, q, dedicated=True, limiter=params, level=2.0)
    want = _reference(q, plain)
    comp = lc.RefCompressor(params, 2)
    limited = [comp.process(w, w.shape[1]) for w in want]
    comp.close()
    top = np.max([np.abs(w).max(axis=1) for w in limited], axis=0)
    assert float(max(np.abs(w).max() for w in want)) > 0.5       # above the threshold
    for k, (g, w) in enumerate(zip(got, limited)):
        err = np.abs(g[ND:].astype(np.float64) - w).max(axis=1)
        assert np.all(err <= 1e-5 * top + 1e-30), (quality, k, err, top)


def test_encoded_pcm_matches_the_reference_output_stage():
    """oalgpu_read_output in s16: Write<short> of the reference (its bridge renders a stereo device's RealOut) on the
    reference-encoded lines"""
    import oalgpu
    _need()
    if not bl.available():
        pytest.skip("needs the reference bridge")
    sizes = _sizes(16)
    plain = _run("fast", sizes, dedicated=True)
    want = _reference(0, plain)
    bridge = bl.Bridge(bl.MODE_CPU)
    bl.build_config1(bridge, nsources=1)
    sc, fx, update = tc.build_scene(_api("fast"), dedicated=True)
    sc.set_tsme_encoder(oalgpu.TSME_IIR)
    sc.set_output(oalgpu.OUT_I16, 0.0, 22222)
    for k, n in enumerate(sizes):
        update(k)
        sc.mix(n, post_process=True)
        lines = np.zeros((2, 1024), np.float32)
        lines[:, :n] = want[k]
        ref, _ = bridge.render_lines(lines, oalgpu.OUT_I16, 0.0, 22222, n, 2)
        got = sc.read_output(n, 2)
        assert np.array_equal(got, ref), k
    _check_kernel(sc, "fast")
    sc.close(); fx.close(); bridge.close()


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_removal_and_reinstall(mode):
    """removed: from then on the lines are the plain context's, bit for bit; re-installed: a fresh state (the reference
    encoder started at that update)"""
    import oalgpu
    _need()
    sizes = _sizes(20)
    plain = _run(mode, sizes, dedicated=True)
    removed = _run(mode, sizes, oalgpu.TSME_IIR, dedicated=True, events={7: None})
    for k in range(7, len(sizes)):
        assert np.array_equal(removed[k].view(np.uint32), plain[k].view(np.uint32)), k
    assert not np.array_equal(removed[3][ND:], plain[3][ND:])
    for name, q in QUALITIES.items():
        again = _run(mode, sizes, q, dedicated=True, events={9: q})
        _compare(q, again[9:], _reference(q, plain[9:]), plain[9:], f"{mode} {name} re-installed")
    later = _run(mode, sizes, None, dedicated=True, events={5: oalgpu.TSME_FIR256})
    _compare(1, later[5:], _reference(1, plain[5:]), plain[5:], f"{mode} installed at update 5")


def test_refused_arguments(synth_mhr):
    import oalgpu
    _need()
    api = _api("fast")
    # an invalid quality, and a context that is not a stereo TSME device
    sc, fx, update = tc.build_scene(api)
    for bad in (3, 7):
        with pytest.raises(oalgpu.OalgpuError):
            sc.set_tsme_encoder(bad)
    sc.close()
    for kw in (dict(num_dry=3, num_real=2), dict(num_dry=4, num_real=0), dict(num_dry=4, num_real=3), dict(num_dry=9, num_real=2)):
        other = api.make_scene(wet_channels=4, hrtf=False, max_voices=4, **kw)
        with pytest.raises(oalgpu.OalgpuError):
            other.set_tsme_encoder(oalgpu.TSME_IIR)
        other.set_tsme_encoder(None)                    # (removing what is not there is no error)
        other.close()
    api.hrtf_load(synth_mhr)
    h = api.make_scene(num_dry=4, num_real=2, wet_channels=4, hrtf=True, max_voices=4)
    with pytest.raises(oalgpu.OalgpuError):
        h.set_tsme_encoder(oalgpu.TSME_IIR)
    h.close()
    # one post-process.  A decoder is set: the encoder refuses; with it a crossfeed or (three real lines needed: covered by the
    # line-count rule above) a stabilizer: the encoder refuses for the decoder already
    hf, lf = cc.decoder_matrices("stereo dual band")
    sc, fx, update = tc.build_scene(_api("fast"))
    sc.set_bformat_decoder(hf, lf)
    with pytest.raises(oalgpu.OalgpuError):
        sc.set_tsme_encoder(oalgpu.TSME_IIR)
    sc.set_crossfeed(oalgpu.BS2B_HIGH_EASY)
    with pytest.raises(oalgpu.OalgpuError):
        sc.set_tsme_encoder(oalgpu.TSME_IIR)
    sc.set_crossfeed(None)
    sc.set_bformat_decoder(None)
    sc.set_tsme_encoder(oalgpu.TSME_FIR512)
    sc.close()
    # a UHJ encoder is set (a 3-dry device: the TSME encoder refuses for the line count; the UHJ setter on a TSME device likewise)
    u = api.make_scene(num_dry=3, num_real=2, wet_channels=4, hrtf=False, max_voices=4)
    u.set_uhj_encoder(oalgpu.UHJ_IIR)
    with pytest.raises(oalgpu.OalgpuError):
        u.set_tsme_encoder(oalgpu.TSME_IIR)
    u.close()
    # what a set encoder refuses, in the middle of a run; a refusal changes nothing
    sizes = _sizes(12)
    plain = _run("fast", sizes, dedicated=True)
    sc, fx, update = tc.build_scene(_api("fast"), dedicated=True)
    sc.set_tsme_encoder(oalgpu.TSME_IIR)
    got = []
    for k, n in enumerate(sizes):
        if k == 4:
            with pytest.raises(oalgpu.OalgpuError):
                sc.set_bformat_decoder(hf, lf)
            with pytest.raises(oalgpu.OalgpuError):
                sc.set_uhj_encoder(oalgpu.UHJ_IIR)
            with pytest.raises(oalgpu.OalgpuError):
                sc.set_front_stabilizer(0, 1, 0, 5000.0 / 48000.0)
            with pytest.raises(oalgpu.OalgpuError):
                sc.set_crossfeed(oalgpu.BS2B_LOW)
            with pytest.raises(oalgpu.OalgpuError):
                sc.set_tsme_encoder(7)
        update(k)
        sc.mix(n, post_process=True)
        got.append(np.array(sc.dry()[:, :n], np.float32))
    _check_kernel(sc, "fast")
    sc.close(); fx.close()
    _compare(0, got, _reference(0, plain), plain, "after refusals")
