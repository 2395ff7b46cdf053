"""The front stabilizer (oalgpu_set_front_stabilizer) against the reference composition of tests/stabilizer_cases.py: the
reference's own BFormatDec, its own BandSplitter filters and libm's pan constants, glued as alu.cpp:329-405 glues them.

The same speaker scene runs several times: plain (no decoder: the bus block holds the dry lines and the direct real lines),
decoder only, and stabilized.  The reference composition runs over the plain run's lines.  EXACT contexts post-process
serially and must match bit for bit; FAST contexts post-process on the overlapped path, where the decode itself differs from
the reference's in the last bits, so there the stabilizer is pinned bit for bit on the GPU's own decoded feeds (silent direct
lines) and bounded by four times the decoder's own measured error where the direct lines carry signal.

Measured on one MI355X, FAST with the dedicated slot: 7.1 decoder error e = 3.6e-7 (bound 3.9e-5) and stabilized lines within
2.4e-7 = 0.67 e of the reference composition; the permuted 4-line layout e = 2.4e-7 and 2.5e-7 = 1.06 e."""
import numpy as np
import pytest

import limiter_cases as lc
import oracle_lib as ol
import stabilizer_cases as sc

pytestmark = pytest.mark.gpu
XOVER = 5000.0 / 48000.0


def _need():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    if not sc.available():
        pytest.skip("needs the compiled reference")


def _sizes(updates):
    return [sc.SIZES[k % len(sc.SIZES)] for k in range(updates)]


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


def _install(scene, layout, xover=XOVER):
    lay = sc.LAYOUTS[layout]
    scene.set_front_stabilizer(lay["left"], lay["right"], lay["center"], xover)


def _run(mode, sizes, layout, decoder=False, stabilizer=False, dedicated=False, events=None, limiter=None, level=1.0):
    """Every update's bus lines ((dry + real) x n) of a fresh scene.  events: {update: f(scene)} applied before that update."""
    scene, fx, update = sc.build_scene(_api(mode), layout, dedicated=dedicated, level=level)
    if decoder or stabilizer:
        scene.set_bformat_decoder(*sc.decoder_matrices(layout))
    if stabilizer:
        _install(scene, layout)
    if limiter is not None:
        scene.set_output_limiter(limiter)
    out = []
    for k, n in enumerate(sizes):
        if events and k in events:
            events[k](scene)
        update(k)
        scene.mix(n, post_process=True)
        out.append(np.array(scene.dry()[:, :n], np.float32))
    _check_kernel(scene, mode)
    scene.close()
    if fx is not None:
        fx.close()
    return out


def _reference(layout, plain, start=0, feeds=None, decoders=None):
    """The reference composition over the plain run's lines: -> per update the real lines (None before `start`, where only
    the decoder runs: its band splitters' state is older than a stabilizer installed later).  feeds: per update the decoded
    feeds to use in place of the reference decoder (the GPU's own, direct lines silent).  decoders: {update: (hf, lf)}, a
    fresh decoder from that update on."""
    lay = sc.LAYOUTS[layout]
    nd, nr = lay["num_dry"], lay["num_real"]
    L = ol.load("ref")
    L.L.oal_set_simd(1)
    dec = ol.BFormatDec(L, nd, *sc.decoder_matrices(layout))
    st = None
    want = []
    for k, p in enumerate(plain):
        n = p.shape[1]
        if decoders and k in decoders:
            dec.close()
            dec = ol.BFormatDec(L, nd, *decoders[k])
        dry = np.zeros((nd, 1024), np.float32)
        dry[:, :n] = p[:nd]

        def decode(out, k=k, n=n, dry=dry):
            if feeds is not None:
                out[:, :n] += feeds[k]
            else:
                dec.process(out, dry, n)

        if k < start:
            decode(np.zeros((nr, 1024), np.float32))
            want.append(None)
            continue
        if st is None:
            st = sc.RefStabilizer(nr, lay["left"], lay["right"], lay["center"], XOVER)
        want.append(st.process(p[nd:], n, decode))
    dec.close()
    return want


def _decoder_reference(layout, plain):
    """the reference decoder alone over the plain run's lines: per update direct + decoded real lines"""
    lay = sc.LAYOUTS[layout]
    nd, nr = lay["num_dry"], lay["num_real"]
    L = ol.load("ref")
    L.L.oal_set_simd(1)
    dec = ol.BFormatDec(L, nd, *sc.decoder_matrices(layout))
    out = []
    for p in plain:
        n = p.shape[1]
        dry = np.zeros((nd, 1024), np.float32)
        dry[:, :n] = p[:nd]
        only = np.zeros((nr, 1024), np.float32)
        only[:, :n] = p[nd:]
        dec.process(only, dry, n)
        out.append(only[:, :n].copy())
    dec.close()
    return out


def _equal_bits(layout, got, want, plain, tag):
    nd = sc.LAYOUTS[layout]["num_dry"]
    for k, (g, w, p) in enumerate(zip(got, want, plain)):
        if w is None:
            continue
        assert np.array_equal(g[:nd].view(np.uint32), p[:nd].view(np.uint32)), (tag, k)      # the dry lines stay as they were
        assert np.array_equal(g[nd:].view(np.uint32), w.view(np.uint32)), (tag, k, float(np.abs(g[nd:] - w).max()))


def _not_vacuous(layout, got, decoder_only, tag):
    lay = sc.LAYOUTS[layout]
    nd = lay["num_dry"]
    assert any(not np.array_equal(g[nd:], d[nd:]) for g, d in zip(got, decoder_only)), tag
    assert max(float(np.abs(g[nd + lay["center"]]).max()) for g in got) > 1e-3, tag


@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_exact_matches_the_reference_bit_for_bit(layout):
    """EXACT contexts, the real lines fed by a dedicated-effect slot: bit for bit, every update"""
    _need()
    nd = sc.LAYOUTS[layout]["num_dry"]
    sizes = _sizes(24)
    plain = _run("exact", sizes, layout, dedicated=True)
    assert max(float(np.abs(p[nd:]).max()) for p in plain) > 1e-2            # the direct lines are not silent
    got = _run("exact", sizes, layout, stabilizer=True, dedicated=True)
    _equal_bits(layout, got, _reference(layout, plain), plain, f"exact {layout} dedicated")
    _not_vacuous(layout, got, _run("exact", sizes, layout, decoder=True, dedicated=True), f"exact {layout}")


@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_exact_with_silent_real_lines(layout):
    _need()
    nd = sc.LAYOUTS[layout]["num_dry"]
    sizes = _sizes(24)
    plain = _run("exact", sizes, layout)
    assert all(not np.any(p[nd:]) for p in plain)
    got = _run("exact", sizes, layout, stabilizer=True)
    _equal_bits(layout, got, _reference(layout, plain), plain, f"exact {layout} silent")
    _not_vacuous(layout, got, _run("exact", sizes, layout, decoder=True), f"exact {layout} silent")


@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_fast_on_its_own_decoded_feeds_bit_for_bit(layout):
    """FAST contexts (overlapped path), silent real lines: the reference's filters and glue over the GPU's own decoded feeds"""
    _need()
    nd = sc.LAYOUTS[layout]["num_dry"]
    sizes = _sizes(24)
    plain = _run("fast", sizes, layout)
    assert all(not np.any(p[nd:]) for p in plain)
    decoder_only = _run("fast", sizes, layout, decoder=True)
    got = _run("fast", sizes, layout, stabilizer=True)
    feeds = [d[nd:] for d in decoder_only]
    _equal_bits(layout, got, _reference(layout, plain, feeds=feeds), plain, f"fast {layout} own feeds")
    _not_vacuous(layout, got, decoder_only, f"fast {layout}")


@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_fast_with_direct_lines_within_the_decoders_own_error(layout):
    """FAST with the dedicated slot: the FAST decode differs from the reference's, so the yardstick is that difference, measured
    here: decoder only against ol.BFormatDec (inside tests/test_output_stage.py's 2e-5 max + 1e-7) gives e; the stabilized lines
    may differ from the reference composition by 4 e (two decoded lines are summed into each of mid and side, every filter
    behind them is an all-pass or a complementary split, the combine halves; the factor leaves the filters' peak gain as margin)"""
    _need()
    nd = sc.LAYOUTS[layout]["num_dry"]
    sizes = _sizes(24)
    plain = _run("fast", sizes, layout, dedicated=True)
    assert max(float(np.abs(p[nd:]).max()) for p in plain) > 1e-2
    decoder_only = _run("fast", sizes, layout, decoder=True, dedicated=True)
    ref_decoded = _decoder_reference(layout, plain)
    top = max(float(np.abs(w).max()) for w in ref_decoded)
    e = max(float(np.abs(d[nd:].astype(np.float64) - w).max()) for d, w in zip(decoder_only, ref_decoded))
    print(f"fast {layout}: decoder-only error e = {e:.3e} (bound {2e-5 * top + 1e-7:.3e}, line max {top:.3f})")
    assert e <= 2e-5 * top + 1e-7
    got = _run("fast", sizes, layout, stabilizer=True, dedicated=True)
    want = _reference(layout, plain)
    worst = 0.0
    for k, (g, w, p) in enumerate(zip(got, want, plain)):
        assert np.array_equal(g[:nd].view(np.uint32), p[:nd].view(np.uint32)), k
        worst = max(worst, float(np.abs(g[nd:].astype(np.float64) - w).max()))
    print(f"fast {layout}: stabilized |err| {worst:.3e} = {worst / e if e else float('nan'):.2f} e")
    assert worst <= 4.0 * e, (worst, e)
    _not_vacuous(layout, got, decoder_only, f"fast {layout} dedicated")


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_removal_and_reinstall(mode):
    """removed: from that update on the lines are the decoder-only run's, bit for bit; re-installed: a reference composition
    started fresh at that update (the decoder's own state runs on)"""
    _need()
    layout = "7.1"
    nd = sc.LAYOUTS[layout]["num_dry"]
    sizes = _sizes(20)
    dedicated = mode == "exact"
    plain = _run(mode, sizes, layout, dedicated=dedicated)
    decoder_only = _run(mode, sizes, layout, decoder=True, dedicated=dedicated)
    removed = _run(mode, sizes, layout, stabilizer=True, dedicated=dedicated, events={7: lambda s: s.set_front_stabilizer(None)})
    for k in range(7, len(sizes)):
        assert np.array_equal(removed[k].view(np.uint32), decoder_only[k].view(np.uint32)), k
    assert not np.array_equal(removed[3][nd:], decoder_only[3][nd:])
    feeds = None if mode == "exact" else [d[nd:] for d in decoder_only]
    again = _run(mode, sizes, layout, stabilizer=True, dedicated=dedicated,
                 events={5: lambda s: s.set_front_stabilizer(None), 9: lambda s: _install(s, layout)})
    _equal_bits(layout, again[9:], _reference(layout, plain, start=9, feeds=feeds)[9:], plain[9:], f"{mode} re-installed")
    for k in range(5, 9):
        assert np.array_equal(again[k].view(np.uint32), decoder_only[k].view(np.uint32)), k
    later = _run(mode, sizes, layout, decoder=True, dedicated=dedicated, events={6: lambda s: _install(s, layout)})
    _equal_bits(layout, later[6:], _reference(layout, plain, start=6, feeds=feeds)[6:], plain[6:], f"{mode} installed at update 6")


def test_decoder_matrices_replaced_while_set():
    """oalgpu_set_bformat_decoder with new matrices while a stabilizer is set: a fresh decoder from that update on, the
    stabilizer's filter state kept"""
    _need()
    layout = "7.1"
    sizes = _sizes(16)
    hf, lf = sc.decoder_matrices(layout)
    hf2, lf2 = hf * np.float32(0.8), lf * np.float32(1.1)
    plain = _run("exact", sizes, layout, dedicated=True)
    got = _run("exact", sizes, layout, stabilizer=True, dedicated=True, events={6: lambda s: s.set_bformat_decoder(hf2, lf2)})
    _equal_bits(layout, got, _reference(layout, plain, decoders={6: (hf2, lf2)}), plain, "decoder replaced")
    unchanged = _reference(layout, plain)
    assert not np.array_equal(got[8][5:], unchanged[8])


def test_limiter_behind_the_stabilizer():
    """the limiter sees the stabilized lines: the reference Compressor over the reference composition, within the limiter
    tests' bound (an EXACT context, so that the limiter's input is the reference composition bit for bit)"""
    _need()
    if not lc.available():
        pytest.skip("needs the compiled reference")
    layout = "7.1"
    nd, nr = sc.LAYOUTS[layout]["num_dry"], sc.LAYOUTS[layout]["num_real"]
    sizes = _sizes(24)
    params = lc.limiter_params(48000, "no automation")           # threshold -6 dB, 4:1: the scene drives it
    plain = _run("exact", sizes, layout, dedicated=True, level=6.0)
    got = _run("exact", sizes, layout, stabilizer=True, dedicated=True, limiter=params, level=6.0)
    want = _reference(layout, plain)
    comp = lc.RefCompressor(params, nr)
    limited = [comp.process(w, w.shape[1]) for w in want]
    comp.close()
    top = np.max([np.abs(w).max(axis=1) for w in limited], axis=0)
    assert float(max(np.abs(w).max() for w in want)) > 0.5       # above the threshold
    for k, (g, w) in enumerate(zip(got, limited)):
        err = np.abs(g[nd:].astype(np.float64) - w).max(axis=1)
        assert np.all(err <= 1e-5 * top + 1e-30), (k, err, top)


def test_refused_arguments(synth_mhr):
    """every refusal leaves the context as it was: the run around them still matches the reference"""
    import oalgpu
    _need()
    layout = "7.1"
    api = _api("fast")
    # an HRTF context
    api.hrtf_load(synth_mhr)
    h = api.make_scene(num_dry=4, num_real=2, wet_channels=4, hrtf=True, max_voices=4)
    with pytest.raises(oalgpu.OalgpuError):
        h.set_front_stabilizer(0, 1, 2, XOVER)
    h.set_front_stabilizer(None)                        # (removing what is not there is no error)
    h.close()
    # no decoder set
    scene, fx, update = sc.build_scene(api, layout)
    with pytest.raises(oalgpu.OalgpuError):
        scene.set_front_stabilizer(0, 1, 2, XOVER)
    scene.close()
    # a UHJ device: the encoder is the post-process
    u = api.make_scene(num_dry=3, num_real=2, wet_channels=4, hrtf=False, max_voices=4)
    u.set_uhj_encoder(oalgpu.UHJ_IIR)
    with pytest.raises(oalgpu.OalgpuError):
        u.set_front_stabilizer(0, 1, 0, XOVER)
    u.close()
    # a three-line device whose decoder is set, then a UHJ encoder cannot be, and the stabilizer with one: covered above; here
    # the index and crossover rules, and what a set stabilizer refuses, in the middle of a run
    sizes = _sizes(12)
    plain = _run("exact", sizes, layout, dedicated=True)

    def refusals(s):
        for bad in ((0, 0, 2), (0, 1, 0), (2, 1, 2), (8, 1, 2), (0, 9, 2), (0, 1, 8)):
            with pytest.raises(oalgpu.OalgpuError):
                s.set_front_stabilizer(*bad, XOVER)
        for bad in (0.0, -0.2, 0.5, 0.9, float("nan")):
            with pytest.raises(oalgpu.OalgpuError):
                s.set_front_stabilizer(0, 1, 2, bad)
        with pytest.raises(oalgpu.OalgpuError):
            s.set_bformat_decoder(None)                 # the stabilizer owns the decoder
        with pytest.raises(oalgpu.OalgpuError):
            s.set_uhj_encoder(oalgpu.UHJ_IIR)           # a decoder is set

    got = _run("exact", sizes, layout, stabilizer=True, dedicated=True, events={4: refusals})
    _equal_bits(layout, got, _reference(layout, plain), plain, "after refusals")
    # the decoder can go once the stabilizer has gone
    scene, fx, update = sc.build_scene(_api("fast"), layout)
    scene.set_bformat_decoder(*sc.decoder_matrices(layout))
    _install(scene, layout)
    scene.set_front_stabilizer(None)
    scene.set_bformat_decoder(None)
    with pytest.raises(oalgpu.OalgpuError):
        _install(scene, layout)
    scene.close()
