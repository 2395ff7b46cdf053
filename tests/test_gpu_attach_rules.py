"""oalgpu_context_attach / oalgpu_context_detach: what is refused (one message per rule, and a refused call changes
nothing), what an attached context may not be asked, and the lifetimes -- tiny contexts; the twins of the detach test are
the only ones held to audio."""
import ctypes as C
import os

import numpy as np
import pytest

import attach_cases as ac

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _api(mode=None):
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    return oalgpu, oalgpu.Api(oalgpu.MATH_FAST if mode is None else mode)


def _refused(oalgpu, call, text):
    with pytest.raises(oalgpu.OalgpuError) as err:
        call()
    assert text in str(err.value), str(err.value)
    assert "(-2)" in str(err.value), str(err.value)             # OALGPU_ERR_INVALID


def _works(*scenes):
    """an update of every scene that is not attached (the attached ones ride along), and their lines come back"""
    for sc in scenes:
        if sc._device_scene is None:
            sc.mix(64, post_process=True)
    for sc in scenes:
        assert np.isfinite(sc.dry()).all()


IDENT = [0, 1, 2, 3]


def test_attach_refusals(synth_mhr):
    """every rule of include/oalgpu.h, with its message; after each refusal both contexts still update"""
    oalgpu, api = _api()
    from oalgpu import synth
    dev = ac.build_lines(api, 2, 1, num_real=2, max_voices=2)
    cand = ac.build_lines(api, 2, 2, max_voices=2)
    other = ac.build_lines(api, 2, 3, num_real=2, max_voices=2)
    lib = oalgpu.lib
    lib.oalgpu_context_attach.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    m = (C.c_int32 * 4)(*IDENT)

    def raw(d, c, mp):
        oalgpu.check(lib.oalgpu_context_attach(d, c, mp), "oalgpu_context_attach")

    _refused(oalgpu, lambda: raw(None, cand.h, m), "null argument")
    _refused(oalgpu, lambda: raw(dev.h, None, m), "null argument")
    _refused(oalgpu, lambda: raw(dev.h, cand.h, None), "null argument")
    _refused(oalgpu, lambda: dev.attach(dev, [0, 1, 2, 3, 4, 5]), "cannot be attached to itself")
    _works(dev, cand)
    # a map entry out of range (the device context has 6 lines: 0 .. 5)
    _refused(oalgpu, lambda: dev.attach(cand, [0, 1, 2, 6]), "map entry 3 is out of range")
    _refused(oalgpu, lambda: dev.attach(cand, [0, -2, 2, 3]), "map entry 1 is out of range")
    # another sample rate; another device ordinal where the box has one
    slow = api.make_scene(sample_rate=44100, num_dry=4, max_voices=2)
    _refused(oalgpu, lambda: dev.attach(slow, IDENT), "different sample rates")
    slow.close()
    if oalgpu.device_count() > 1:
        far = oalgpu.Api(oalgpu.MATH_FAST, device=1).make_scene(num_dry=4, max_voices=2)
        _refused(oalgpu, lambda: dev.attach(far, IDENT), "different devices")
        far.close()
    # an HRTF context
    api.hrtf_load(synth_mhr)
    head = api.make_scene(num_dry=4, num_real=2, hrtf=True, max_voices=2)
    _refused(oalgpu, lambda: dev.attach(head, [0, 1, 2, 3, 4, 5]), "HRTF voices belong to the device context")
    head.close()
    _works(dev, cand)
    # what the device context does for its contexts: post-process kinds, limiter, distance compensation, output conversion
    out2 = ac.build_lines(api, 2, 4, num_real=2, max_voices=2)
    out2.set_bformat_decoder(synth.stereo_decoder()[0])
    _refused(oalgpu, lambda: dev.attach(out2, [0, 1, 2, 3, 4, 5]), "post-process installed")
    out2.set_bformat_decoder(None)
    uhj = api.make_scene(num_dry=3, num_real=2, max_voices=2)
    uhj.set_uhj_encoder(oalgpu.UHJ_IIR)
    _refused(oalgpu, lambda: dev.attach(uhj, [0, 1, 2, 4, 5]), "post-process installed")
    uhj.close()
    on, params = oalgpu.limiter_device_params(48000, oalgpu.OUT_I16)
    params.num_channels = 2
    out2.set_output_limiter(params)
    _refused(oalgpu, lambda: dev.attach(out2, [0, 1, 2, 3, 4, 5]), "output limiter")
    out2.set_output_limiter(None)
    out2.set_distance_comp([3, 0], [1.0, 0.5])
    _refused(oalgpu, lambda: dev.attach(out2, [0, 1, 2, 3, 4, 5]), "distance compensation")
    out2.set_distance_comp(None)
    out2.set_output(oalgpu.OUT_I16, 0.0, 1)
    _refused(oalgpu, lambda: dev.attach(out2, [0, 1, 2, 3, 4, 5]), "output conversion")
    out2.set_output(oalgpu.OUT_F32, 0.0, 1)
    dev.attach(out2, [0, 1, 2, 3, 4, 5])                    # ... and with all of it removed it is accepted
    out2.detach()
    _works(dev, out2)
    out2.close()
    # a collective on either side (the host-staged transport with a world of one rank)
    name = f"/oalgpu_attach_rules_{os.getpid()}"
    cand.comm_init_host(name, 0, 1)
    _refused(oalgpu, lambda: dev.attach(cand, IDENT), "collective")
    cand.comm_destroy()
    dev.comm_init_host(name, 0, 1)
    _refused(oalgpu, lambda: dev.attach(cand, IDENT), "collective")
    dev.comm_destroy()
    _works(dev, cand)
    # a caller-owned stream (here: one that belongs to a third context)
    cand.set_stream(other.bus_device_ptr()[2])
    _refused(oalgpu, lambda: dev.attach(cand, IDENT), "caller-owned stream")
    cand.set_stream(None)
    _works(dev, cand, other)
    # attached twice; nesting in both directions
    dev.attach(cand, IDENT)
    _refused(oalgpu, lambda: dev.attach(cand, IDENT), "already attached")
    _refused(oalgpu, lambda: other.attach(cand, IDENT), "already attached")
    third = ac.build_lines(api, 2, 5, max_voices=2)
    _refused(oalgpu, lambda: cand.attach(third, IDENT), "is itself attached (no nesting)")
    _refused(oalgpu, lambda: other.attach(dev, [0, 1, 2, 3, 4, 5]), "has attached contexts of its own (no nesting)")
    # ... and what an attachment refuses in turn
    _refused(oalgpu, lambda: cand.comm_init_host(name, 0, 1), "has, or is, an attachment")
    _refused(oalgpu, lambda: dev.comm_init_host(name, 0, 1), "has, or is, an attachment")
    _refused(oalgpu, lambda: cand.set_stream(other.bus_device_ptr()[2]), "stays on its own streams")
    _works(dev, cand, other, third)
    _refused(oalgpu, third.detach, "is not attached")
    for sc in (third, cand, other, dev):
        sc.close()


def test_mix_entry_points_are_refused_on_an_attached_context():
    oalgpu, api = _api()
    dev = ac.build_lines(api, 2, 1, num_real=2, max_voices=2)
    child = ac.build_lines(api, 2, 2, max_voices=2)
    dev.attach(child, IDENT)
    text = "its device context updates it"
    _refused(oalgpu, lambda: child.mix(64, post_process=True), text)
    _refused(oalgpu, lambda: child.mix(64, post_process=False), text)
    _refused(oalgpu, lambda: child.mix_run([None, None], 64, post_process=True), text)
    _refused(oalgpu, lambda: child.mix_voices(64), text)
    _refused(oalgpu, lambda: child.post_process(64), text)
    _refused(oalgpu, lambda: child.mix_voices_overlapped(64), text)
    _refused(oalgpu, lambda: child.post_process_overlapped(64), text)
    # an attached context has no post stage: what the attach refuses to find installed cannot be installed afterwards
    # (removals stay open), and a refusal changes nothing
    from oalgpu import synth
    stage = "its device context has the post stage"
    two = ac.build_lines(api, 2, 4, num_real=2, max_voices=2)
    dev.attach(two, [0, 1, 2, 3, 4, 5])
    _refused(oalgpu, lambda: two.set_bformat_decoder(synth.stereo_decoder()[0]), stage)
    _refused(oalgpu, lambda: two.set_tsme_encoder(oalgpu.TSME_IIR), stage)
    params = oalgpu.limiter_device_params(48000, oalgpu.OUT_I16)[1]
    params.num_channels = 2
    _refused(oalgpu, lambda: two.set_output_limiter(params), stage)
    _refused(oalgpu, lambda: two.set_distance_comp([3, 0], [1.0, 0.5]), stage)
    _refused(oalgpu, lambda: two.set_output(oalgpu.OUT_I16, 0.0, 1), stage)
    two.set_bformat_decoder(None); two.set_output_limiter(None); two.set_distance_comp(None); two.set_output(oalgpu.OUT_F32, 0.0, 1)
    two.detach()
    two.set_output_limiter(params)                      # ... and on its own again it takes them
    two.set_output_limiter(None)
    two.close()
    # every other setter is still there, and the device context's split entry points update the attached context too
    child.set_params(0, ac.ol.make_voice_params(60211, ac.ol.RS_BSINC24, dry_gains=[0.1, 0.2, 0.3, 0.4]))
    before = child.voice_state(0).position
    dev.mix_voices(64)
    assert child.voice_state(0).position != before
    merged_nothing = dev.dry()[:4].copy()
    dev.post_process(64)
    assert np.abs(dev.dry()[:4, :64] - merged_nothing[:, :64]).max() > 1e-3      # only the post-processing half merges
    child.close(); dev.close()


def test_detach_leaves_both_contexts_as_if_never_attached():
    """Four attached updates, then the detach: from there the device context's lines are a never-attached twin's bits, and
    the former attachment, updated by its own entry points, is its twin's bits (the twin mixed alone all along)."""
    oalgpu, api = _api()

    def pair():
        return ac.build_lines(api, 2, 1, num_real=2, max_voices=2), ac.build_lines(api, 3, 2, send=True, max_voices=3)

    dev, child = pair()
    dev_twin, child_twin = pair()
    dev.attach(child, IDENT)
    for n in (1024, 700, 1024, 24):
        dev.mix(n, post_process=True)
        dev_twin.mix(n, post_process=True)
        child_twin.mix(n, post_process=True)
    assert np.abs(dev.dry()[:4] - dev_twin.dry()[:4]).max() > 1e-2         # while attached the lines differ by the attachment
    child.detach()
    for n in (1024, 333, 1024):
        for sc in (dev, child, dev_twin, child_twin):
            sc.mix(n, post_process=True)
        assert np.array_equal(_bits(dev.dry()[:, :n]), _bits(dev_twin.dry()[:, :n])), n
        assert np.array_equal(_bits(child.dry()[:, :n]), _bits(child_twin.dry()[:, :n])), n
        assert np.array_equal(_bits(child.wet(0)[:, :n]), _bits(child_twin.wet(0)[:, :n])), n
        assert np.abs(child.dry()).max() > 1e-2
    for v in range(3):
        assert ac.int_state(child.voice_state(v)) == ac.int_state(child_twin.voice_state(v))
    dev.attach(child, IDENT)                                               # and it can be attached again
    dev.mix(1024, post_process=True)
    assert np.abs(dev.dry()[:4] - dev_twin.dry()[:4]).max() > 1e-2
    for sc in (child, dev, child_twin, dev_twin):
        sc.close()


@pytest.mark.parametrize("first", ["attached context", "device context"])
def test_destroy_orders(first):
    """either one may go first: the attached context's destroy detaches it and the device context updates on alone; the
    device context's destroy detaches its contexts, which live on as independent contexts"""
    oalgpu, api = _api()
    dev = ac.build_lines(api, 2, 1, num_real=2, max_voices=2)
    a = ac.build_lines(api, 2, 2, max_voices=2)
    b = ac.build_lines(api, 2, 3, max_voices=2)
    twin = ac.build_lines(api, 2, 1 if first == "attached context" else 2, num_real=2 if first == "attached context" else 0, max_voices=2)
    dev.attach(a, IDENT)
    dev.attach(b, IDENT)
    for sc in (dev, twin):
        sc.mix(1024, post_process=True)
    if first == "attached context":
        a.close()
        b.close()
        survivors = [dev]
    else:
        dev.close()
        survivors = [a, b]
    for sc in survivors + [twin]:
        sc.mix(1024, post_process=True)
    assert np.array_equal(_bits(survivors[0].dry()), _bits(twin.dry()))       # alone again: the never-attached twin's bits
    for sc in survivors:
        sc.mix(512, post_process=False)
        assert np.isfinite(sc.dry()).all()
    for sc in survivors + [twin] + ([a, b] if first == "device context" else []):
        sc.close()
