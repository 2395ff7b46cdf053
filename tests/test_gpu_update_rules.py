"""What the update entry points refuse (include/oalgpu.h): oalgpu_mix_voices, oalgpu_post_process, oalgpu_mix_update,
oalgpu_mix_voices_overlapped, oalgpu_post_process_overlapped and oalgpu_mix_update_run.  The return code and the text of
every refusal, which refusal wins where two reasons hold at once (sample count, then FAST context on its own streams, then
attached, then HRTF data set), and that refused calls between the updates of a scene leave it bit for bit a twin scene that
never made them.  No reference is needed: the scenes are compared with each other.  4 voices, updates of 1, 64 and 1024 samples.

The caller-owned stream of the FAST case is a third context's stream, as in tests/test_gpu_attach_rules.py, not a torch
stream: oalgpu_set_stream takes any hipStream_t of the device, and the test needs no second HIP runtime in its process."""
import ctypes as C

import numpy as np
import pytest

import attach_cases as ac

pytestmark = pytest.mark.gpu

OK, INVALID, NO_HRTF = 0, -2, -4
NV = 4
IDENT = [0, 1, 2, 3]
SAMPLES_TEXT = "samples_to_do must be 1..1024"
FAST_TEXT = "needs a FAST context"
ATTACHED_TEXT = "the context is attached"
DATA_SET_TEXT = "HRTF context without a data set"
REAL_LINES_TEXT = "HRTF post-process needs two real output lines"
SERIAL = ("oalgpu_mix_voices", "oalgpu_post_process", "oalgpu_mix_update")
OVERLAPPED = ("oalgpu_mix_voices_overlapped", "oalgpu_post_process_overlapped")
FIVE = SERIAL + OVERLAPPED


def _gpu():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    L = oalgpu.lib
    L.oalgpu_mix_voices_overlapped.argtypes = [C.c_void_p, C.c_uint32]
    L.oalgpu_post_process_overlapped.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    L.oalgpu_mix_update_run.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_int]
    return oalgpu


def _call(oalgpu, name, h, n):
    """one of the five entry points (or oalgpu_mix_update_run over two updates) -> (return code, oalgpu_last_error)"""
    L = oalgpu.lib
    if name == "oalgpu_mix_update_run":
        rc = L.oalgpu_mix_update_run(h, None, 2, n, 1)
    elif name in ("oalgpu_mix_update", "oalgpu_post_process_overlapped"):
        rc = getattr(L, name)(h, n, 1)
    else:
        rc = getattr(L, name)(h, n)
    return rc, L.oalgpu_last_error().decode()


def _refused(oalgpu, name, h, n, code, text):
    rc, msg = _call(oalgpu, name, h, n)
    print(f"{name}({n}) -> {rc}: {msg}")
    assert rc == code, (name, n, rc, msg)
    assert text in msg, (name, n, msg)
    return msg


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lines(api, seed=1):
    """a speaker context: 4 dry + 2 real lines, no sends (FAST: the wavefront kernel)"""
    return ac.build_lines(api, NV, seed, num_real=2, max_voices=NV)


def _bare_hrtf(oalgpu, mode, num_real=2):
    """an HRTF context without a data set (the Scene loads one: this context is made by hand)"""
    desc = oalgpu.ContextDesc(0, mode, 48000, 4, num_real, 0, 0, 4, 1, NV, 3, 0, 0)
    ctx = C.c_void_p()
    assert oalgpu.lib.oalgpu_context_create(C.byref(desc), C.byref(ctx)) == OK, oalgpu.lib.oalgpu_last_error().decode()
    return ctx


def _refuse_sample_counts(oalgpu, h):
    for name in FIVE:
        for n in (0, 1025):
            _refused(oalgpu, name, h, n, INVALID, SAMPLES_TEXT)


def test_sample_count_and_null_context():
    oalgpu = _gpu()
    sc = _lines(oalgpu.Api(oalgpu.MATH_FAST))
    _refuse_sample_counts(oalgpu, sc.h)
    for name in FIVE:                                           # a null context is the same refusal, whatever the count
        for n in (0, 64, 1025):
            _refused(oalgpu, name, None, n, INVALID, SAMPLES_TEXT)
    L = oalgpu.lib
    assert L.oalgpu_mix_update_run(sc.h, None, 0, 64, 1) == INVALID
    assert L.oalgpu_mix_update_run(None, None, 2, 64, 1) == INVALID
    assert L.oalgpu_mix_update_run(None, None, 0, 64, 1) == INVALID
    # a run whose count is fine passes the sample count on to its updates
    _refused(oalgpu, "oalgpu_mix_update_run", sc.h, 0, INVALID, SAMPLES_TEXT)
    _refused(oalgpu, "oalgpu_mix_update_run", sc.h, 1025, INVALID, SAMPLES_TEXT)
    for n in (1, 64, 1024):                                     # ... and the limits themselves are accepted
        for name in FIVE + ("oalgpu_mix_update_run",):
            assert _call(oalgpu, name, sc.h, n)[0] == OK, (name, n)
    assert np.isfinite(sc.dry()).all()
    sc.close()


def test_overlapped_calls_need_a_fast_context_on_its_own_streams():
    oalgpu = _gpu()
    exact = _lines(oalgpu.Api(oalgpu.MATH_EXACT))
    assert exact.voice_kernel_name().startswith("VoiceMixKernel")
    for name in OVERLAPPED:
        for n in (1, 64, 1024):
            msg = _refused(oalgpu, name, exact.h, n, INVALID, FAST_TEXT)
            assert msg.startswith(name + ":"), msg
        _refused(oalgpu, name, exact.h, 0, INVALID, SAMPLES_TEXT)       # (the sample count goes first)
    for name in SERIAL:
        assert _call(oalgpu, name, exact.h, 64)[0] == OK, name
    exact.close()
    fast = _lines(oalgpu.Api(oalgpu.MATH_FAST))
    assert not fast.voice_kernel_name().startswith("VoiceMixKernel")
    for name in OVERLAPPED:
        assert _call(oalgpu, name, fast.h, 64)[0] == OK, name
    owner = _lines(oalgpu.Api(oalgpu.MATH_FAST), 2)
    fast.set_stream(owner.bus_device_ptr()[2])
    for name in OVERLAPPED:
        msg = _refused(oalgpu, name, fast.h, 64, INVALID, FAST_TEXT)
        assert msg.startswith(name + ":"), msg
        _refused(oalgpu, name, fast.h, 1025, INVALID, SAMPLES_TEXT)
    for name in SERIAL:                                         # a caller-owned stream is never forked: one stream
        assert _call(oalgpu, name, fast.h, 64)[0] == OK, name
    fast.set_stream(None)
    for name in OVERLAPPED:
        assert _call(oalgpu, name, fast.h, 64)[0] == OK, name
    assert np.isfinite(fast.dry()).all()
    fast.close(); owner.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_an_attached_context_is_updated_by_its_device_context(mode):
    oalgpu = _gpu()
    api = oalgpu.Api(oalgpu.MATH_FAST if mode == "fast" else oalgpu.MATH_EXACT)
    dev, child = _lines(api, 1), ac.build_lines(api, NV, 2, max_voices=NV)
    dev.attach(child, IDENT)
    every = FIVE + ("oalgpu_mix_update_run",)
    for name in every:
        if mode == "exact" and name in OVERLAPPED:
            # the order of the refusals: the sample count, then the FAST context, then the attachment
            _refused(oalgpu, name, child.h, 64, INVALID, FAST_TEXT)
            _refused(oalgpu, name, child.h, 0, INVALID, SAMPLES_TEXT)
            continue
        for n in (1, 64, 1024):
            msg = _refused(oalgpu, name, child.h, n, INVALID, ATTACHED_TEXT)
            assert msg.startswith(name + ":"), msg
        if name != "oalgpu_mix_update_run":                     # (a run refuses the attachment itself, its updates the count)
            _refused(oalgpu, name, child.h, 0, INVALID, SAMPLES_TEXT)
            _refused(oalgpu, name, child.h, 1025, INVALID, SAMPLES_TEXT)
    dev.mix(64, post_process=True)                              # the device context still updates both
    child.detach()
    for name in every:
        if mode == "exact" and name in OVERLAPPED:
            continue
        assert _call(oalgpu, name, child.h, 64)[0] == OK, name
    assert np.isfinite(child.dry()).all() and np.abs(child.dry()).max() > 1e-3
    child.close(); dev.close()


def test_hrtf_context_without_a_data_set():
    oalgpu = _gpu()
    L = oalgpu.lib
    ctx = _bare_hrtf(oalgpu, oalgpu.MATH_FAST)
    try:
        for name in ("oalgpu_mix_voices", "oalgpu_mix_update", "oalgpu_mix_voices_overlapped", "oalgpu_mix_update_run"):
            for n in (1, 64, 1024):
                _refused(oalgpu, name, ctx, n, NO_HRTF, DATA_SET_TEXT)
            _refused(oalgpu, name, ctx, 0, INVALID, SAMPLES_TEXT)       # (the sample count goes first)
    finally:
        L.oalgpu_context_destroy(ctx)
    ctx = _bare_hrtf(oalgpu, oalgpu.MATH_EXACT)
    try:
        for name in ("oalgpu_mix_voices", "oalgpu_mix_update"):
            _refused(oalgpu, name, ctx, 64, NO_HRTF, DATA_SET_TEXT)
        # ... and the FAST context in front of the data set
        _refused(oalgpu, "oalgpu_mix_voices_overlapped", ctx, 64, INVALID, FAST_TEXT)
        _refused(oalgpu, "oalgpu_mix_voices_overlapped", ctx, 1025, INVALID, SAMPLES_TEXT)
    finally:
        L.oalgpu_context_destroy(ctx)


def test_hrtf_post_process_needs_two_real_lines():
    """oalgpu_context_create accepts an HRTF descriptor with fewer than two real lines: its post-process is what refuses"""
    oalgpu = _gpu()
    for num_real in (0, 1):
        ctx = _bare_hrtf(oalgpu, oalgpu.MATH_FAST, num_real=num_real)
        try:
            for name in ("oalgpu_post_process", "oalgpu_post_process_overlapped"):
                _refused(oalgpu, name, ctx, 64, INVALID, REAL_LINES_TEXT)
                _refused(oalgpu, name, ctx, 0, INVALID, SAMPLES_TEXT)
        finally:
            oalgpu.lib.oalgpu_context_destroy(ctx)


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("kind", ["speaker", "hrtf"])
def test_refused_updates_change_nothing(kind, mode, synth_mhr):
    """the refused calls between the updates of one scene only: its dry and real lines (speaker) or its two output lines
    (HRTF) stay a twin's bits after every update"""
    oalgpu = _gpu()
    api = oalgpu.Api(oalgpu.MATH_FAST if mode == "fast" else oalgpu.MATH_EXACT)
    if kind == "hrtf":
        api.hrtf_load(synth_mhr)
        scene, twin = (ac.build_hrtf_device(api, NV, 32, max_voices=NV) for _ in range(2))
        out = lambda sc, n: sc.dry()[4:6, :n]
    else:
        scene, twin = _lines(api), _lines(api)
        out = lambda sc, n: sc.dry()[:, :n]
    L = oalgpu.lib
    peak = 0.0
    for k, n in enumerate((64, 1, 1024, 64, 1, 1024)):
        _refuse_sample_counts(oalgpu, scene.h)
        assert L.oalgpu_mix_update_run(scene.h, None, 0, n, 1) == INVALID
        _refused(oalgpu, "oalgpu_mix_update_run", scene.h, 1025, INVALID, SAMPLES_TEXT)
        if mode == "exact":
            for name in OVERLAPPED:
                _refused(oalgpu, name, scene.h, n, INVALID, FAST_TEXT)
        for sc in (scene, twin):
            assert L.oalgpu_mix_update(sc.h, n, 1) == OK, L.oalgpu_last_error().decode()
        a, b = out(scene, n), out(twin, n)
        assert np.array_equal(_bits(a), _bits(b)), (k, n)
        peak = max(peak, float(np.abs(a).max()))
    print(f"{kind}/{mode}: peak output {peak:.3e}")
    assert peak > 1e-3                                          # not the equality of silence
    scene.close(); twin.close()
