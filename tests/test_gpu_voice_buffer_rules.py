"""What the buffer, voice-start and per-voice setter entry points refuse, and what a refused or a staged call leaves behind.

The expectations are written out by hand from include/oalgpu.h and the behaviour the library has had all along; nothing here
asks the library what it would answer.  Every refused call has exactly one thing wrong with it, and the return code is what is
asserted (the message is for people).  Contexts have 2 voices and 3 buffers, buffers 64 frames, updates 64 samples: the rules
are host rules, and the kernels behind them only have to show which records arrived."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

OK, INVALID, NO_HRTF, CAPACITY = 0, -2, -4, -5
FRAC_ONE = 1 << 16              # kFracOne (csrc/dev_math.hpp): MixerFracOne of the port, position_frac counts below it
N = 64
RAMP = ((np.arange(N) + 1) / 64.0).astype(np.float32)
u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
CALLBACK = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int32)


def _need():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    L = oalgpu.lib
    L.oalgpu_buffer_register_adpcm.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_uint32] * 5
    L.oalgpu_buffer_channel_view.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.oalgpu_buffer_queue_link.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.oalgpu_voice_init_queue.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int32, C.c_uint32]
    L.oalgpu_voice_queue_unqueue.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.oalgpu_voice_queue_state.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), u32p]
    L.oalgpu_voice_set_start_delay.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.oalgpu_voice_set_ambi_scale.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float]
    L.oalgpu_voice_set_nfc.argtypes = [C.c_void_p, C.c_uint32, C.c_float]
    L.oalgpu_context_set_nfc.argtypes = [C.c_void_p, C.c_float, u32p]
    L.oalgpu_voice_set_hrtf_targets.argtypes = [C.c_void_p, u32p, f32p, u32p, f32p, C.c_size_t]
    L.oalgpu_voice_move_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.oalgpu_voice_set_pan.argtypes = [C.c_void_p, u32p, f32p, C.c_size_t]
    L.oalgpu_voices_readback.argtypes = [C.c_void_p, u32p, C.c_size_t, C.c_void_p]
    return oalgpu


def _scene(oalgpu, mhr=None, mode=None, **kw):
    """2 voices, 3 buffers; mhr: an HRTF context on that data set"""
    api = oalgpu.Api(oalgpu.MATH_EXACT if mode is None else mode)
    if mhr:
        api.hrtf_load(mhr)
    shape = dict(num_dry=4, num_real=2, hrtf=True) if mhr else dict(num_dry=3, num_real=0, hrtf=False)
    return api.make_scene(max_voices=2, max_buffers=3, **shape, **kw)


def _register(sc, data=RAMP, fmt=ol.FMT_FLOAT, step=1, n=N, ls=0, le=N):
    import oalgpu
    data = np.ascontiguousarray(data)
    return oalgpu.lib.oalgpu_buffer_register(sc.h, data.ctypes.data_as(C.c_void_p), fmt, step, n, ls, le)


def _init(sc, voice, buffer, looping=0, position=0, frac=0):
    import oalgpu
    d = oalgpu.VoiceDesc(buffer, looping, position, frac, 44100)
    return oalgpu.lib.oalgpu_voice_init(sc.h, voice, C.byref(d))


def _init_queue(sc, voice, buffer, looping=0, position=0, frac=0):
    import oalgpu
    return oalgpu.lib.oalgpu_voice_init_queue(sc.h, voice, buffer, looping, position, frac)


def _params(line=0, gain=1.0, hrtf=None, **kw):
    if hrtf is not None:
        return ol.make_voice_params(65536, ol.RS_POINT, hrtf=hrtf, **kw)
    g = [0.0, 0.0, 0.0]
    g[line] = gain
    return ol.make_voice_params(65536, ol.RS_POINT, dry_gains=g, **kw)


def _set_params(sc, voices, params):
    """oalgpu_voice_set_params on a batch -> its return code"""
    import oalgpu
    arr = (type(params[0]) * len(params))(*params)
    v = np.ascontiguousarray(voices, np.uint32)
    return oalgpu.lib.oalgpu_voice_set_params(sc.h, v.ctypes.data_as(u32p), C.cast(arr, C.c_void_p), len(v))


def _set_pan(sc, voices, rows):
    import oalgpu
    v = np.ascontiguousarray(voices, np.uint32)
    p = np.ascontiguousarray(rows, np.float32).reshape(max(len(v), 1), 11)
    return oalgpu.lib.oalgpu_voice_set_pan(sc.h, v.ctypes.data_as(u32p), p.ctypes.data_as(f32p), len(v))


def _set_targets(sc, voices, coeffs, delays, gains):
    import oalgpu
    v = np.ascontiguousarray(voices, np.uint32)
    co = np.ascontiguousarray(coeffs, np.float32)
    de = np.ascontiguousarray(delays, np.uint32)
    ga = np.ascontiguousarray(gains, np.float32)
    return oalgpu.lib.oalgpu_voice_set_hrtf_targets(sc.h, v.ctypes.data_as(u32p), co.ctypes.data_as(f32p), de.ctypes.data_as(u32p),
                                                    ga.ctypes.data_as(f32p), len(v))


def _move(sc, moves):
    import oalgpu
    m = np.ascontiguousarray(moves, oalgpu.MOVE_DTYPE)
    return oalgpu.lib.oalgpu_voice_move_async(sc.h, m.ctypes.data_as(C.c_void_p), len(m))


def _update(sc):
    """one update of 64 samples -> the dry and real lines as bit patterns"""
    sc.mix(N, post_process=bool(sc.desc.hrtf))
    return np.array(sc.dry()[:, :N], np.float32).view(np.uint32)


def _held_released(sc, voice=0):
    """a buffer that is live but released: the voice slot started on it holds it"""
    h = _register(sc)
    assert h >= 0 and _init(sc, voice, h) == OK
    sc.release_buffer(h)
    assert sc.buffer_info(h) == (True, True, 1)
    return h


LOOP_REFUSALS = [(0, N + 1), (10, 10), (20, 10), (1, 0)]     # loop_end > sample_len; start >= end with end > 0 (twice); start > 0 with end == 0


# ---- registration ----------------------------------------------------------------------------------------------------------
def test_buffer_register_refusals_and_the_full_table():
    oalgpu = _need()
    sc = _scene(oalgpu)
    for fmt in (-1, oalgpu.FMT_ALAW + 1):
        assert _register(sc, fmt=fmt) == INVALID, fmt
    assert _register(sc, step=0) == INVALID
    assert _register(sc, n=0, le=0) == INVALID
    for ls, le in LOOP_REFUSALS:
        assert _register(sc, ls=ls, le=le) == INVALID, (ls, le)
    # none of the refusals took a place: three registrations, in handle order; the fourth live buffer is one too many
    assert [_register(sc) for _ in range(3)] == [0, 1, 2]
    assert _register(sc) == CAPACITY
    sc.release_buffer(1)                                       # nothing holds it: freed at once
    assert sc.buffer_info(1)[0] is False
    assert _register(sc) == 1                                  # ... and the freed handle comes back
    assert _register(sc) == CAPACITY
    sc.close()


def test_buffer_register_adpcm_refusals_and_the_full_table():
    oalgpu = _need()
    sc = _scene(oalgpu)
    data = np.zeros(1 << 17, np.uint8)
    IMA4, MS = 0, 1

    def reg(kind=IMA4, channels=1, spb=65, n=N, ls=0, le=N):
        return oalgpu.lib.oalgpu_buffer_register_adpcm(sc.h, data.ctypes.data_as(C.c_void_p), kind, channels, spb, n, ls, le)

    assert reg(kind=2) == INVALID and reg(kind=-1) == INVALID
    assert reg(channels=0) == INVALID and reg(channels=3) == INVALID
    assert reg(kind=IMA4, spb=1) == INVALID
    assert reg(kind=MS, spb=2) == INVALID
    assert reg(spb=65537) == INVALID
    for ls, le in LOOP_REFUSALS:
        assert reg(ls=ls, le=le) == INVALID, (ls, le)
    assert [reg(kind=IMA4), reg(kind=MS, spb=64), reg(channels=2)] == [0, 1, 2]
    assert reg() == CAPACITY
    sc.close()


def test_channel_view_refusals_leave_the_parents_count_alone():
    oalgpu = _need()
    view = oalgpu.lib.oalgpu_buffer_channel_view
    sc = _scene(oalgpu)
    stereo = np.arange(2 * N, dtype=np.float32) / 128.0
    h = _register(sc, data=stereo, step=2)
    assert h == 0 and sc.buffer_info(h) == (True, False, 0)
    assert view(sc.h, h, 2) == INVALID                         # channel == frame_step
    assert view(sc.h, 2, 0) == INVALID and view(sc.h, -1, 0) == INVALID      # dead handles
    assert sc.buffer_info(h) == (True, False, 0)
    released = _held_released(sc)                              # handle 1
    assert view(sc.h, released, 0) == INVALID
    assert sc.buffer_info(released) == (True, True, 1)
    v = view(sc.h, h, 1)
    assert v == 2 and sc.buffer_info(h) == (True, False, 1)    # the view holds its parent
    assert view(sc.h, h, 0) == CAPACITY                        # a view takes a place of the table
    assert sc.buffer_info(h) == (True, False, 1)
    sc.close()


# ---- voice starts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [_init, _init_queue], ids=["init", "init_queue"])
def test_voice_start_refusals(start):
    oalgpu = _need()
    sc = _scene(oalgpu)
    good = _register(sc)
    assert start(sc, 2, good) == INVALID                       # voice 2 of 2
    assert start(sc, 0, 2) == INVALID and start(sc, 0, -1) == INVALID        # dead handles
    released = _held_released(sc, voice=1)
    assert start(sc, 0, released) == INVALID
    assert start(sc, 0, good, frac=FRAC_ONE) == INVALID
    assert start(sc, 0, good, frac=FRAC_ONE - 1) == OK
    assert sc.buffer_info(good) == (True, False, 1)            # only the accepted start holds it
    no_loop = _register(sc, le=0)
    assert no_loop >= 0
    # a static voice loops between its buffer's loop points; a queue voice returns to its first buffer
    assert start(sc, 0, no_loop, looping=1) == (INVALID if start is _init else OK)
    sc.close()
    # an HRTF context without a data set (the Scene loads one: this context is made by hand)
    api = oalgpu.Api(oalgpu.MATH_EXACT)
    desc = oalgpu.ContextDesc(api.device, api.mode, 48000, 4, 2, 0, 0, 4, 1, 2, 3, 0, 0)
    ctx = C.c_void_p()
    assert oalgpu.lib.oalgpu_context_create(C.byref(desc), C.byref(ctx)) == OK

    class Bare:
        h = ctx
    try:
        b = _register(Bare)
        assert b == 0
        assert start(Bare, 0, b) == NO_HRTF
    finally:
        oalgpu.lib.oalgpu_context_destroy(ctx)


def _playing(oalgpu, mhr=None, **kw):
    """both voices looping over the ramp, voice v on dry line v (HRTF: from two directions)"""
    sc = _scene(oalgpu, mhr, **kw)
    h = _register(sc)
    for v in range(2):
        assert _init(sc, v, h, looping=1) == OK
        assert _set_params(sc, [v], [_params(hrtf=(0.2, 1.0 + v, 2.0, 0.0, 0.5)) if mhr else _params(line=v, gain=0.5)]) == OK
    return sc, h


def test_a_refused_start_changes_nothing():
    oalgpu = _need()
    refused = [lambda sc: _init(sc, 0, 2), lambda sc: _init(sc, 0, 0, frac=FRAC_ONE), lambda sc: _init(sc, 2, 0),
               lambda sc: _init_queue(sc, 0, -1), lambda sc: _init(sc, 0, 1, looping=1)]
    for call in refused:
        got = []
        for twin in (False, True):
            sc, h = _playing(oalgpu)
            assert _register(sc, le=0) == 1                    # (without loop points)
            first = _update(sc)
            if not twin:
                assert call(sc) == INVALID
            assert sc.buffer_info(h) == (True, False, 2) and sc.buffer_info(1) == (True, False, 0)
            got.append((first, _update(sc)))
            sc.close()
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
        assert np.any(got[0][1])                               # (the voices do play)


def test_two_starts_on_one_slot_before_an_update_play_the_second():
    """the second start replaces the first in the pending list: one record per slot reaches the device"""
    oalgpu = _need()
    sc = _scene(oalgpu)
    a, b = _register(sc), _register(sc, data=-RAMP)
    assert _init(sc, 0, a) == OK and sc.buffer_info(a)[2] == 1
    assert _init(sc, 0, b) == OK
    assert sc.buffer_info(a) == (True, False, 0) and sc.buffer_info(b) == (True, False, 1)
    assert _set_params(sc, [0], [_params()]) == OK
    sc.mix(N)
    assert np.array_equal(sc.dry()[0, :N], -RAMP)
    sc.close()


# ---- queues ----------------------------------------------------------------------------------------------------------------
def test_queue_link_and_unqueue():
    oalgpu = _need()
    L = oalgpu.lib
    sc = _scene(oalgpu)
    hs = [_register(sc, data=RAMP * (i + 1)) for i in range(3)]
    assert hs == [0, 1, 2]
    assert L.oalgpu_voice_queue_unqueue(sc.h, 0, 0) == OK      # a count of 0: at any time
    assert L.oalgpu_buffer_queue_link(sc.h, hs[0], hs[2]) == OK
    assert sc.buffer_info(hs[2]) == (True, False, 1)           # the link holds its target
    assert L.oalgpu_buffer_queue_link(sc.h, hs[0], -1) == OK   # the queue ends at buffer 0
    assert sc.buffer_info(hs[2]) == (True, False, 0)
    assert L.oalgpu_buffer_queue_link(sc.h, hs[0], hs[1]) == OK and L.oalgpu_buffer_queue_link(sc.h, hs[1], hs[2]) == OK
    assert _init_queue(sc, 0, hs[0]) == OK
    assert _set_params(sc, [0], [_params()]) == OK
    assert L.oalgpu_voice_queue_unqueue(sc.h, 0, 1) == INVALID    # nothing read back yet
    sc.mix(N)
    sc.mix(N)                                                  # 128 frames at 1:1: through buffers 0 and 1
    assert np.array_equal(sc.dry()[0, :N], RAMP * 2)
    assert L.oalgpu_voice_queue_unqueue(sc.h, 0, 1) == INVALID    # still nothing read back
    cur, done = sc.queue_state(0)
    print("queue state after two updates:", cur, done)
    assert (cur, done) == (hs[2], 2)
    assert L.oalgpu_voice_queue_unqueue(sc.h, 0, 0) == OK
    assert L.oalgpu_voice_queue_unqueue(sc.h, 0, done + 1) == INVALID        # more than it has reported
    assert L.oalgpu_voice_queue_unqueue(sc.h, 0, done) == OK
    assert L.oalgpu_voice_queue_unqueue(sc.h, 0, 1) == INVALID               # all of them given up already
    assert sc.buffer_info(hs[2]) == (True, False, 2)           # buffer 1's link and the voice's hold, which moved on to it
    # a released buffer cannot become a link's target
    sc.release_buffer(hs[2])
    assert sc.buffer_info(hs[2]) == (True, True, 2)
    assert L.oalgpu_buffer_queue_link(sc.h, hs[0], hs[2]) == INVALID
    assert sc.buffer_info(hs[2]) == (True, True, 2)
    sc.close()


# ---- single-voice setters ----------------------------------------------------------------------------------------------------
def test_single_voice_setter_refusals(synth_mhr):
    oalgpu = _need()
    L = oalgpu.lib
    sc, _ = _playing(oalgpu)
    assert L.oalgpu_voice_set_start_delay(sc.h, 0, 48000) == INVALID         # a second ahead: the context's sample rate
    assert L.oalgpu_voice_set_start_delay(sc.h, 0, 47999) == OK
    for xover in (0.0, 0.5):
        assert L.oalgpu_voice_set_ambi_scale(sc.h, 0, xover, 1.0, 1.0) == INVALID, xover
    assert L.oalgpu_voice_set_ambi_scale(sc.h, 0, 0.25, 1.0, 1.0) == OK
    for state in (oalgpu.VOICE_STOPPED - 1, oalgpu.VOICE_PENDING + 1):
        assert L.oalgpu_voice_set_state(sc.h, 0, state) == INVALID, state
    assert L.oalgpu_voice_set_nfc(sc.h, 0, 0.1) == INVALID                   # before oalgpu_context_set_nfc
    cpo = lambda *n: (C.c_uint32 * 5)(*n)
    assert L.oalgpu_context_set_nfc(sc.h, 0.1, cpo(2, 1, 0, 0, 0)) == INVALID    # order 0 is W alone
    assert L.oalgpu_context_set_nfc(sc.h, 0.1, cpo(1, 2, 0, 0, 0)) == OK
    assert L.oalgpu_context_set_nfc(sc.h, 0.1, cpo(1, 2, 0, 0, 0)) == INVALID    # a second time
    assert L.oalgpu_voice_set_nfc(sc.h, 0, 0.1) == OK
    # voice 2 of 2
    cur, done = C.c_int32(0), C.c_uint32(0)
    state = oalgpu.VoiceState()
    brief = (C.c_uint32 * 8)()
    two = (C.c_uint32 * 1)(2)
    assert L.oalgpu_voice_set_start_delay(sc.h, 2, 8) == INVALID
    assert L.oalgpu_voice_set_ambi_scale(sc.h, 2, 0.25, 1.0, 1.0) == INVALID
    assert L.oalgpu_voice_set_state(sc.h, 2, oalgpu.VOICE_PLAYING) == INVALID
    assert L.oalgpu_voice_set_nfc(sc.h, 2, 0.1) == INVALID
    assert L.oalgpu_voice_queue_state(sc.h, 2, C.byref(cur), C.byref(done)) == INVALID
    assert L.oalgpu_voice_queue_unqueue(sc.h, 2, 0) == INVALID
    assert L.oalgpu_voice_readback(sc.h, 2, C.byref(state)) == INVALID
    assert L.oalgpu_voices_readback(sc.h, two, 1, brief) == INVALID
    # a callback voice has no start to delay
    sc.add_callback_voice(np.zeros(4096, np.float32), oalgpu.FMT_FLOAT, voice=1)
    assert L.oalgpu_voice_set_start_delay(sc.h, 1, 8) == INVALID
    assert L.oalgpu_voice_set_start_delay(sc.h, 0, 8) == OK
    sc.close()
    hr = _scene(oalgpu, synth_mhr)
    assert L.oalgpu_context_set_nfc(hr.h, 0.1, cpo(1, 2, 0, 0, 0)) == INVALID    # HRTF voices mix through the HRTF path
    hr.close()


# ---- batch setters -----------------------------------------------------------------------------------------------------------
def _targets(rng, count):
    co = np.zeros((count, 128, 2), np.float32)
    co[:, :32] = rng.uniform(-0.3, 0.3, (count, 32, 2))
    return co, rng.integers(0, 64, (count, 2)).astype(np.uint32), rng.uniform(0.2, 0.8, count).astype(np.float32)


def _pan_rows(rng, count):
    rows = np.zeros((count, 11), np.float32)
    d = rng.normal(size=(count, 3))
    rows[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rows[:, 4] = rng.uniform(0.2, 0.8, count)
    return rows


def test_batch_setter_refusals(synth_mhr):
    oalgpu = _need()
    rng = np.random.default_rng(3)
    hr, _ = _playing(oalgpu, synth_mhr)
    p = _params(hrtf=(0.1, 0.2, 2.0, 0.0, 0.5))
    co, de, ga = _targets(rng, 3)
    moves = np.zeros(3, oalgpu.MOVE_DTYPE)
    moves["hrtf_dist"] = 2.0
    # an empty batch: nothing to do, but for the pan
    assert _set_params(hr, np.zeros(0, np.uint32), [p]) == OK
    assert _set_targets(hr, np.zeros(0, np.uint32), co, de, ga) == OK
    assert _move(hr, moves[:0]) == OK
    assert _set_pan(hr, np.zeros(0, np.uint32), np.zeros(11)) == INVALID
    bad = _params(hrtf=(0.1, 0.2, -2.0, 0.0, 0.5))              # negative distances but -1 are reserved
    assert _set_params(hr, [0], [bad]) == INVALID
    de64 = de.copy()
    de64[0, 1] = 64                                            # MaxHrirDelay is 63
    assert _set_targets(hr, [0], co[:1], de64[:1], ga[:1]) == INVALID
    assert _set_targets(hr, [0], co[:1], de[:1], ga[:1]) == OK
    assert _move(hr, moves) == INVALID                         # three records, two voices
    moves["voice"] = [0, 2, 0]
    assert _move(hr, moves[:2]) == INVALID                     # voice 2 of 2
    moves["voice"] = [0, 1, 0]
    assert _move(hr, moves[:2]) == OK
    hr.close()
    sc = _scene(oalgpu, num_sends=1, num_slots=1)
    assert _register(sc) == 0
    for rs in (-1, ol.RS_BSINC48 + 1):
        q = _params()
        q.resampler = rs
        assert _set_params(sc, [0], [q]) == INVALID, rs
    assert _set_params(sc, [2], [_params()]) == INVALID
    assert _set_params(sc, [0], [_params(sends=[(1, [0.5], None)])]) == INVALID      # slot 1 of 1
    assert _set_params(sc, [0], [_params(sends=[(0, [0.5], None)])]) == OK
    assert _set_targets(sc, [0], co[:1], de[:1], ga[:1]) == INVALID                  # HRTF contexts only
    sc.close()


@pytest.mark.parametrize("setter", ["set_params", "set_pan", "set_hrtf_targets"])
def test_a_batch_whose_second_record_is_bad_installs_nothing_of_its_first(setter, synth_mhr):
    oalgpu = _need()
    mhr = synth_mhr if setter == "set_hrtf_targets" else None
    rng = np.random.default_rng(5)
    co, de, ga = _targets(rng, 2)
    rows = _pan_rows(rng, 2)
    got = []
    for twin in (False, True):
        sc, _ = _playing(oalgpu, mhr)
        if setter == "set_pan":
            sc.set_ambi_map([0, 1, 2], [1.0, 1.0, 1.0])
        first = _update(sc)
        if not twin:
            voices = [0, 2]                                     # the second record names voice 2 of 2
            rc = {"set_params": lambda: _set_params(sc, voices, [_params(line=2, gain=0.9)] * 2),
                  "set_pan": lambda: _set_pan(sc, voices, rows),
                  "set_hrtf_targets": lambda: _set_targets(sc, voices, co, de, ga)}[setter]()
            assert rc == INVALID
        got.append((first, _update(sc)))
        sc.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert np.any(got[0][1])


@pytest.mark.parametrize("setter", ["set_params", "set_pan", "set_hrtf_targets"])
def test_staging_grows_and_is_reused(setter, synth_mhr):
    """1 record, then 2, then 1 on one context: every time the update equals that of a twin context which was given the same
    records one voice per call"""
    oalgpu = _need()
    mhr = synth_mhr if setter == "set_hrtf_targets" else None
    rng = np.random.default_rng(9)
    rounds = [[0], [0, 1], [1]]
    records = []
    for voices in rounds:
        if setter == "set_params":
            records.append([_params(line=int(rng.integers(0, 3)), gain=float(rng.uniform(0.2, 0.9))) for _ in voices])
        elif setter == "set_pan":
            records.append(_pan_rows(rng, len(voices)))
        else:
            records.append(_targets(rng, len(voices)))

    def issue(sc, voices, rec):
        if setter == "set_params":
            return _set_params(sc, voices, list(rec))
        if setter == "set_pan":
            return _set_pan(sc, voices, rec)
        return _set_targets(sc, voices, *rec)

    def one(rec, i):
        if setter == "set_params":
            return [rec[i]]
        if setter == "set_pan":
            return rec[i:i + 1]
        return tuple(a[i:i + 1] for a in rec)

    got = []
    for twin in (False, True):
        sc, _ = _playing(oalgpu, mhr)
        if setter == "set_pan":
            sc.set_ambi_map([0, 1, 2], [1.0, 0.5, 0.25])
        outs = []
        for voices, rec in zip(rounds, records):
            if twin:
                for i, v in enumerate(voices):
                    assert issue(sc, [v], one(rec, i)) == OK
            else:
                assert issue(sc, voices, rec) == OK
            outs.append(_update(sc))
        got.append(outs)
        sc.close()
    for k in range(len(rounds)):
        assert np.array_equal(got[0][k], got[1][k]), k
        assert np.any(got[0][k])
    assert not np.array_equal(got[0][0], got[0][1])             # (the records do arrive)


def test_three_starts_flushed_by_one_update():
    """three starts in front of one flush against three contexts with one start each.  Slot 0 is started twice: the host keeps
    one pending start per slot, the last (two records of one voice in one launch would race for its state on the device)"""
    oalgpu = _need()
    data = [RAMP, -RAMP, RAMP * 0.5]

    def scene(starts):
        sc = _scene(oalgpu)
        assert [_register(sc, data=d) for d in data] == [0, 1, 2]
        for voice, buffer in starts:
            assert _init(sc, voice, buffer) == OK
        for voice in {v for v, _ in starts}:
            assert _set_params(sc, [voice], [_params(line=voice)]) == OK
        out = _update(sc)
        info = [sc.buffer_info(h) for h in range(3)]
        sc.close()
        return out, info

    all3, info = scene([(0, 0), (1, 1), (0, 2)])
    assert info == [(True, False, 0), (True, False, 1), (True, False, 1)]
    only = [scene([s])[0] for s in ((0, 0), (1, 1), (0, 2))]
    assert np.array_equal(all3[0], only[2][0]) and np.array_equal(all3[1], only[1][1])
    assert not np.array_equal(all3[0], only[0][0])
    assert np.array_equal(all3[0].view(np.float32), RAMP * 0.5) and np.array_equal(all3[1].view(np.float32), -RAMP)


def test_setter_order_around_a_deferred_start():
    """a start waits for the next update (or the next setter of the voice): a setter issued behind it lands behind it, and a
    start issued behind a setter clears what the setter left, as it clears the ambisonic scale (oalgpu.h)"""
    oalgpu = _need()
    want = {True: np.concatenate([np.zeros(8, np.float32), RAMP[:N - 8]]), False: RAMP}
    for delay_after_init in (True, False):
        sc = _scene(oalgpu)
        h = _register(sc)
        if delay_after_init:
            assert _init(sc, 0, h) == OK
            assert oalgpu.lib.oalgpu_voice_set_start_delay(sc.h, 0, 8) == OK
        else:
            assert oalgpu.lib.oalgpu_voice_set_start_delay(sc.h, 0, 8) == OK
            assert _init(sc, 0, h) == OK
        assert _set_params(sc, [0], [_params()]) == OK
        sc.mix(N)
        got = np.array(sc.dry()[0, :N], np.float32)
        print("delay after init" if delay_after_init else "init after delay", got[:12])
        assert np.array_equal(got.view(np.uint32), want[delay_after_init].view(np.uint32)), delay_after_init
        sc.close()
