"""The stereo UHJ encoder (oalgpu_set_uhj_encoder) against the compiled reference's own UhjEncoderIIR / UhjEncoder<256> /
UhjEncoder<512> (core/uhjfilter.cpp).

Two contexts run the same UHJ device scene (3 dry lines W, X, Y; 2 real lines; voices panned around the circle), one
without the encoder and one with it.  Every update's plain W / X / Y and real lines go through the reference encoder, and
the encoded context's real lines must match it: IIR bit for bit, FIR within 2e-6 of the run's line maximum (the GPU sums
the phase-shift response directly where the reference convolves by FFT).  The dry lines stay as they were.  Updates are
ragged.  EXACT contexts post-process serially, FAST ones on the overlapped path (wavefront voice kernel, post stream)."""
import numpy as np
import pytest

import bridge_lib as bl
import limiter_cases as lc
import uhj_cases as uc

SIZES = (1024, 17, 47, 128, 129, 1000, 1, 1024)
QUALITIES = {"iir": 0, "fir256": 1, "fir512": 2}
pytestmark = pytest.mark.gpu


def _need():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    if not uc.available():
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


def _run(mode, sizes, quality=None, dedicated=False, events=None, limiter=None):
    """Every update's bus lines (5 x n) of a fresh UHJ scene.  events: {update: quality or None} applied before that
    update (set_uhj_encoder)."""
    sc, fx, update = uc.build_scene(_api(mode), dedicated=dedicated)
    if quality is not None:
        sc.set_uhj_encoder(quality)
    if limiter is not None:
        sc.set_output_limiter(limiter)
    out = []
    for k, n in enumerate(sizes):
        if events and k in events:
            sc.set_uhj_encoder(events[k])
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
    enc = uc.RefUhjEncoder(quality)
    want = []
    for k, p in enumerate(plain):
        if k < start:
            want.append(None)
            continue
        left, right = enc.encode(p[0], p[1], p[2], p[3], p[4])
        want.append(np.stack([left, right]))
    return want


def _compare(quality, got, want, plain, tag):
    top = max(float(np.abs(w).max()) for w in want if w is not None)
    assert top > 1e-2, tag
    worst = 0.0
    for k, (g, w, p) in enumerate(zip(got, want, plain)):
        if w is None:
            continue
        assert np.array_equal(g[:3].view(np.uint32), p[:3].view(np.uint32)), (tag, k)     # the dry lines stay as they were
        if quality == 0:
            assert np.array_equal(g[3:].view(np.uint32), w.view(np.uint32)), (tag, k, float(np.abs(g[3:] - w).max()))
        else:
            err = float(np.abs(g[3:].astype(np.float64) - w).max())
            worst = max(worst, err / top)
            assert err <= 2e-6 * top, (tag, k, err, top)
    print(f"{tag}: line max {top:.3f}, worst |err| / line max {worst:.2e}")
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
    if dedicated:
        assert max(float(np.abs(p[3:]).max()) for p in plain) > 1e-2         # the direct input is not silent
    else:
        assert all(not np.any(p[3:]) for p in plain)
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
    plain = _run("fast", sizes, dedicated=True)
    got = _run("fast", sizes, q, dedicated=True, limiter=params)
    want = _reference(q, plain)
    comp = lc.RefCompressor(params, 2)
    limited = [comp.process(w, w.shape[1]) for w in want]
    comp.close()
    top = np.max([np.abs(w).max(axis=1) for w in limited], axis=0)
    assert float(max(np.abs(w).max() for w in want)) > 0.5       # above the threshold
    for k, (g, w) in enumerate(zip(got, limited)):
        err = np.abs(g[3:].astype(np.float64) - w).max(axis=1)
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
    sc, fx, update = uc.build_scene(_api("fast"), dedicated=True)
    sc.set_uhj_encoder(oalgpu.UHJ_IIR)
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
    removed = _run(mode, sizes, oalgpu.UHJ_IIR, dedicated=True, events={7: None})
    for k in range(7, len(sizes)):
        assert np.array_equal(removed[k].view(np.uint32), plain[k].view(np.uint32)), k
    assert not np.array_equal(removed[3][3:], plain[3][3:])
    for name, q in QUALITIES.items():
        again = _run(mode, sizes, q, dedicated=True, events={9: q})
        _compare(q, again[9:], _reference(q, plain[9:]), plain[9:], f"{mode} {name} re-installed")
    later = _run(mode, sizes, None, dedicated=True, events={5: oalgpu.UHJ_FIR256})
    _compare(1, later[5:], _reference(1, plain[5:]), plain[5:], f"{mode} installed at update 5")


def test_refused_arguments(synth_mhr):
    import oalgpu
    _need()
    api = _api("fast")
    # an invalid quality, and a context that is not a stereo UHJ device
    sc, fx, update = uc.build_scene(api)
    with pytest.raises(oalgpu.OalgpuError):
        sc.set_uhj_encoder(3)
    sc.close()
    for kw in (dict(num_dry=4, num_real=2), dict(num_dry=3, num_real=0), dict(num_dry=3, num_real=3)):
        other = api.make_scene(wet_channels=4, hrtf=False, max_voices=4, **kw)
        with pytest.raises(oalgpu.OalgpuError):
            other.set_uhj_encoder(oalgpu.UHJ_IIR)
        other.set_uhj_encoder(None)                     # (removing what is not there is no error)
        other.close()
    api.hrtf_load(synth_mhr)
    h = api.make_scene(num_dry=3, num_real=2, wet_channels=4, hrtf=True, max_voices=4)
    with pytest.raises(oalgpu.OalgpuError):
        h.set_uhj_encoder(oalgpu.UHJ_IIR)
    h.close()
    # one post-process: the encoder and the B-Format decoder refuse each other, and a refusal changes nothing
    hf = np.zeros((2, oalgpu.MAX_AMBI), np.float32)
    hf[0, :3] = (0.5, 0.3, 0.4)
    hf[1, :3] = (0.5, 0.3, -0.4)
    sizes = _sizes(12)
    plain = _run("fast", sizes, dedicated=True)
    sc, fx, update = uc.build_scene(_api("fast"), dedicated=True)
    sc.set_bformat_decoder(hf)
    with pytest.raises(oalgpu.OalgpuError):
        sc.set_uhj_encoder(oalgpu.UHJ_IIR)
    sc.set_bformat_decoder(None)
    sc.set_uhj_encoder(oalgpu.UHJ_IIR)
    got = []
    for k, n in enumerate(sizes):
        if k == 4:
            with pytest.raises(oalgpu.OalgpuError):
                sc.set_bformat_decoder(hf)
            with pytest.raises(oalgpu.OalgpuError):
                sc.set_uhj_encoder(7)
        update(k)
        sc.mix(n, post_process=True)
        got.append(np.array(sc.dry()[:, :n], np.float32))
    _check_kernel(sc, "fast")
    sc.close(); fx.close()
    _compare(0, got, _reference(0, plain), plain, "after refusals")
