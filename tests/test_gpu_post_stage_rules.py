"""Who may replace whom in the post stage: one post-process per context, as the reference keeps one PostProcess variant per
device (core/device.h: AmbiDec, Hrtf, Uhj, Tsme, Stablizer, Bs2b).

The expectations below are written out by hand from that model and the setters' documented rules (include/oalgpu.h); nothing
here asks the library what it would answer.  A context is brought to every kind its layout can reach, every request is issued
there, and after the request every request is issued once more: the answers are those of the kind the context must be in by
then -- the same kind after a refusal or a removal of what is not installed."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

XOVER = 5000.0 / 48000.0
REQUESTS = ("dec_on", "dec_off", "uhj_on", "tsme_on", "stab_on", "cf_on", "uhj_off", "tsme_off", "stab_off", "cf_off")
REMOVES = ("uhj_off", "tsme_off", "stab_off", "cf_off")

# kind -> the requests it accepts (the removals of REMOVES are accepted everywhere)
ACCEPTS = {
    "none":       {"dec_on", "dec_off", "uhj_on", "tsme_on"},
    "ambidec":    {"dec_on", "dec_off", "stab_on", "cf_on"},
    "stabilizer": {"dec_on", "stab_on"},
    "bs2b":       {"dec_on", "cf_on"},
    "uhj":        {"dec_off", "uhj_on"},
    "tsme":       {"dec_off", "tsme_on"},
}
# (kind, accepted request) -> the kind afterwards, where it is another one
MOVES = {
    ("none", "dec_on"): "ambidec", ("none", "uhj_on"): "uhj", ("none", "tsme_on"): "tsme",
    ("ambidec", "dec_off"): "none", ("ambidec", "stab_on"): "stabilizer", ("ambidec", "cf_on"): "bs2b",
    ("stabilizer", "stab_off"): "ambidec", ("bs2b", "cf_off"): "ambidec",
    ("uhj", "uhj_off"): "none", ("tsme", "tsme_off"): "none",
}
# (dry, real) lines -> the kinds the layout can reach, and the requests its line counts refuse whatever is installed: UHJ needs
# 3 dry and 2 real lines, TSME 4 dry and 2 real lines, the stabilizer three different real lines
LAYOUTS = {
    (3, 3): (("none", "ambidec", "stabilizer", "bs2b"), {"uhj_on", "tsme_on"}),
    (3, 2): (("none", "ambidec", "bs2b", "uhj"), {"tsme_on", "stab_on"}),
    (4, 2): (("none", "ambidec", "bs2b", "tsme"), {"uhj_on", "stab_on"}),
}
# how a context without a post-process gets to a kind
PATHS = {"none": (), "ambidec": ("dec_on",), "stabilizer": ("dec_on", "stab_on"), "bs2b": ("dec_on", "cf_on"),
         "uhj": ("uhj_on",), "tsme": ("tsme_on",)}
RESET = ("stab_off", "cf_off", "uhj_off", "tsme_off", "dec_off")


def _need():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    return oalgpu


def _accepted(kind, request, refused_by_layout):
    return request in REMOVES or (request in ACCEPTS[kind] and request not in refused_by_layout)


def _issue(sc, request):
    """True: accepted; False: refused with OALGPU_ERR_INVALID"""
    import oalgpu
    nreal = sc.desc.num_real_channels
    hf = np.zeros((nreal, oalgpu.MAX_AMBI), np.float32)
    hf[:, 0] = 0.5
    hf[:, 1] = np.linspace(-0.4, 0.4, nreal)
    call = {
        "dec_on": lambda: sc.set_bformat_decoder(hf),
        "dec_off": lambda: sc.set_bformat_decoder(None),
        "uhj_on": lambda: sc.set_uhj_encoder(oalgpu.UHJ_IIR),
        "tsme_on": lambda: sc.set_tsme_encoder(oalgpu.TSME_IIR),
        "stab_on": lambda: sc.set_front_stabilizer(0, 1, 2, XOVER),
        "cf_on": lambda: sc.set_crossfeed(oalgpu.BS2B_LOW, 0, 1),
        "uhj_off": lambda: sc.set_uhj_encoder(None),
        "tsme_off": lambda: sc.set_tsme_encoder(None),
        "stab_off": lambda: sc.set_front_stabilizer(None),
        "cf_off": lambda: sc.set_crossfeed(None),
    }[request]
    try:
        call()
    except oalgpu.OalgpuError as e:
        assert "(-2)" in str(e), e               # OALGPU_ERR_INVALID
        return False
    return True


def _bring(sc, kind):
    for r in RESET:
        assert _issue(sc, r), r
    for r in PATHS[kind]:
        assert _issue(sc, r), (kind, r)


@pytest.mark.parametrize("layout", list(LAYOUTS), ids=lambda l: f"{l[0]} dry {l[1]} real")
def test_every_request_at_every_kind(layout):
    oalgpu = _need()
    kinds, by_layout = LAYOUTS[layout]
    api = oalgpu.Api(oalgpu.MATH_EXACT)
    sc = api.make_scene(num_dry=layout[0], num_real=layout[1], hrtf=False, max_voices=1)
    for kind in kinds:
        for first in REQUESTS:
            want = _accepted(kind, first, by_layout)
            after = MOVES.get((kind, first), kind) if want else kind
            for second in REQUESTS:
                _bring(sc, kind)
                assert _issue(sc, first) == want, (layout, kind, first)
                # the context is in `after`: unchanged by a refusal or by the removal of what is not installed
                assert _issue(sc, second) == _accepted(after, second, by_layout), (layout, kind, first, after, second)
        # the limiter and distance compensation do not depend on the kind
        _bring(sc, kind)
        _, lim = oalgpu.limiter_device_params(48000, oalgpu.OUT_I16)
        sc.set_output_limiter(lim)
        sc.set_distance_comp([3, 0], [1.0, 0.5])
        for request in REQUESTS:
            _bring(sc, kind)
            assert _issue(sc, request) == _accepted(kind, request, by_layout), (layout, kind, request, "limiter, distance comp")
        sc.set_distance_comp(None)
        sc.set_output_limiter(None)
    sc.close()


def test_decoder_stays_while_the_stabilizer_or_the_crossfeed_decodes_with_it():
    """spelled out: the refused requests in between change nothing about it"""
    oalgpu = _need()
    sc = oalgpu.Api(oalgpu.MATH_EXACT).make_scene(num_dry=3, num_real=3, hrtf=False, max_voices=1)
    for kind, off in (("stabilizer", "stab_off"), ("bs2b", "cf_off")):
        _bring(sc, kind)
        for refused in ("dec_off", "uhj_on", "tsme_on", "cf_on" if kind == "stabilizer" else "stab_on", "dec_off"):
            assert not _issue(sc, refused), (kind, refused)
        assert _issue(sc, off) and _issue(sc, "dec_off")
        assert not _issue(sc, "stab_on") and not _issue(sc, "cf_on")        # no decoder any more
    sc.close()


def _uhj_scene(api):
    sc = api.make_scene(num_dry=3, num_real=2, hrtf=False, max_voices=1)
    rng = np.random.default_rng(7)
    buf = sc.add_buffer(rng.uniform(-1, 1, 2000).astype(np.float32), ol.FMT_FLOAT, loop_start=0, loop_end=2000)
    sc.add_voice(buf, looping=True)
    sc.set_params(0, ol.make_voice_params(60211, ol.RS_BSINC24, dry_gains=[0.5, 0.4, -0.3]))
    return sc


def test_removing_the_other_encoder_leaves_the_installed_one_alone():
    """TSME off while UHJ is installed (one kind field serves both encoders): the update encodes as in a context that never
    saw the call.  Without an encoder the real lines of this scene stay silent."""
    oalgpu = _need()
    api = oalgpu.Api(oalgpu.MATH_EXACT)
    got = []
    for remove in (True, False):
        sc = _uhj_scene(api)
        sc.set_uhj_encoder(oalgpu.UHJ_IIR)
        if remove:
            sc.set_tsme_encoder(None)
            sc.set_front_stabilizer(None)
            sc.set_crossfeed(None)
        sc.mix(64, post_process=True)
        got.append(np.array(sc.dry()[:, :64], np.float32))
        sc.close()
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    assert float(np.abs(got[1][3:]).max()) > 1e-2                           # the encoder ran
    plain = _uhj_scene(api)
    plain.mix(64, post_process=True)
    assert not np.any(plain.dry()[3:, :64])
    plain.close()


def test_hrtf_context(synth_mhr):
    """MixDirectHrtf is its post-process: every installation is refused, distance compensation too; the limiter is not"""
    oalgpu = _need()
    api = oalgpu.Api(oalgpu.MATH_EXACT)
    api.hrtf_load(synth_mhr)
    sc = api.make_scene(num_dry=4, num_real=2, hrtf=True, max_voices=1)
    for request in ("dec_on", "uhj_on", "tsme_on", "stab_on", "cf_on"):
        assert not _issue(sc, request), request
    for request in REMOVES:
        assert _issue(sc, request), request
    with pytest.raises(oalgpu.OalgpuError, match=r"\(-2\)"):
        sc.set_distance_comp([3, 0], [1.0, 0.5])
    _, lim = oalgpu.limiter_device_params(48000, oalgpu.OUT_I16)
    sc.set_output_limiter(lim)
    for request in ("dec_on", "uhj_on", "tsme_on", "stab_on", "cf_on"):
        assert not _issue(sc, request), request
    sc.set_output_limiter(None)
    sc.close()
