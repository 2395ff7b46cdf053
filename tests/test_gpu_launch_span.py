"""One voice launch over several deferred updates (OALGPU_CTX_APPLY_IN_VOICE_KERNEL; the bounded run of csrc/voice_wave16.hip,
RunMixSpan in csrc/api.hip) against a launch per update.  Spanning changes scheduling, not arithmetic: every comparison
between two runs of the product is value-exact (np.array_equal).

Reading anything back submits what waits, so a run cannot look at an update in the middle of a span.  The per-update
comparison therefore runs every PREFIX of the nine updates with the span under test and reads at its end: the state after
update m of a launch per update (one run, read after every update) against the state at the end of a run of m updates in
forced spans -- whose last launch covers what was left, so spans of every length up to the forced one are exercised.

The scene (24, 1100 and 2050 voices: the 4-, 8- and 16-wavefront form on a 256-CU device, 2050 with a ragged last workgroup):
three pitches, every other voice filtered, every third voice moved by every update's block (its HRIR is replaced between
two updates of one span: old and new response blend), non-looping voices whose buffer ends in the first update of a span
(the second has to see Stopping), delayed starts that fall into the second update, one 16-bit voice, one queued voice (the
generic loader)."""
import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_wave16_grid import _cus, kernel_for
from test_tolerance_model import multi_voice_tolerance

pytestmark = pytest.mark.gpu

TODO = (1024, 1000, 64, 37, 1024, 1000, 64, 37, 1024)
SIZES = (24, 1100, 2050)
# voices on the short non-looping buffer (900 frames at 70000 / 65536 frames per output sample: gone within 1024 outputs): 1 and
# 10 end in update 0, 16 starts with update 4 -- the first of a launch at spans 2 and 4, the second at span 3 -- and ends in it
SHORT_END, I16_VOICE, QUEUE_VOICE = (1, 10, 16), 5, 6
DELAYS = {3: 1024 + 300, 9: 1024 + 1000 + 64 + 37 + 200, 13: 5, 16: 1024 + 1000 + 64 + 37}     # voice -> samples ahead: into updates 1, 4, 0 and 4


def params_of(v, k):
    r = np.random.default_rng(7000 * v + k)
    return ol.make_voice_params([60211, 70000, 48000][v % 3], ol.RS_BSINC24,
                                hrtf=(np.arcsin(r.uniform(-1, 1)), r.uniform(-np.pi, np.pi), 2.0, 0.0, 10 ** (r.uniform(-30, -12) / 20)),
                                direct_filter=ol.default_filter(active=v % 2, gain_hf=0.5))


def moving(nvoices):
    return [v for v in range(nvoices) if v % 3 == 0]


def build(lib, mhr, nvoices):
    """the scene on `lib`: the product (oalgpu.Api) or the reference (oracle_lib) -- the scene interface is the same"""
    lib.hrtf_load(mhr)
    kw = dict(max_voices=nvoices) if hasattr(lib, "device") else {}
    sc = lib.make_scene(num_dry=4, num_real=2, num_sends=0, num_slots=0, wet_channels=4, hrtf=True, **kw)
    rng = np.random.default_rng(33)
    cc = np.zeros((4, 128, 2), np.float32)
    cc[:, :64] = rng.uniform(-0.2, 0.2, (4, 64, 2))
    sc.set_direct_hrtf(cc, [1.0, 0.8, 0.8, 0.8], 400.0 / 48000.0, 64)
    long_buf = sc.add_buffer(rng.uniform(-1, 1, 9000).astype(np.float32), ol.FMT_FLOAT, loop_start=100, loop_end=8900)
    short_buf = sc.add_buffer(rng.uniform(-1, 1, 900).astype(np.float32), ol.FMT_FLOAT)
    i16_buf = sc.add_buffer((rng.uniform(-1, 1, 7000) * 30000).astype(np.int16), ol.FMT_SHORT, loop_start=0, loop_end=7000)
    q1 = sc.add_buffer(rng.uniform(-1, 1, 1500).astype(np.float32), ol.FMT_FLOAT)
    q2 = sc.add_buffer(rng.uniform(-1, 1, 2500).astype(np.float32), ol.FMT_FLOAT)
    sc.link_buffers(q1, q2)
    for v in range(nvoices):
        if v == QUEUE_VOICE:
            sc.add_queue_voice(q1, looping=False)
        elif v in SHORT_END:
            sc.add_voice(short_buf, looping=False, position=0 if v == 1 else 100)
        elif v == I16_VOICE:
            sc.add_voice(i16_buf, looping=True, position=17)
        else:
            sc.add_voice(long_buf, looping=v % 5 != 4, position=(v * 977) % 8000, frac=(v * 131) % 65536)
        sc.set_params(v, params_of(v, 0))
        if v in DELAYS:
            sc.set_start_delay(v, DELAYS[v])
    return sc


def make_blocks(sc, nvoices):
    mv = moving(nvoices)
    blocks = [None]
    for k in range(1, len(TODO)):
        arr = (ol.VoiceParams * len(mv))(*[params_of(v, k) for v in mv])
        blocks.append(sc.param_block(mv, arr))
    return blocks


def read_all(sc, nvoices, n):
    states = []
    for v in range(nvoices):
        s = sc.voice_state(v)
        states.append((s.play_state, s.position, s.position_frac, s.has_buffer, s.fading, s.hrtf_old_gain, tuple(s.hrtf_old_delay),
                       bytes(s.prev_samples), bytes(s.hrtf_history), bytes(s.direct_lp), bytes(s.direct_hp)))
    return sc.dry()[:, :n].copy(), sc.hrtf_accum().copy(), states


def product(span, flags=None):
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    return oalgpu.Api(oalgpu.MATH_FAST, ctx_flags=oalgpu.CTX_APPLY_IN_VOICE_KERNEL if flags is None else flags)


_PER_UPDATE = {}


def launch_per_update(mhr, nvoices):
    """the state after every update of a run that never spans (computed once per size, never changed)"""
    if nvoices not in _PER_UPDATE:
        sc = build(product(1), mhr, nvoices)
        assert sc.voice_kernel_name() == kernel_for(nvoices, _cus()), sc.voice_kernel_name()
        sc.set_launch_span(1)
        blocks = make_blocks(sc, nvoices)
        out = []
        for k, n in enumerate(TODO):
            if k:
                sc.apply_block(blocks[k])
            sc.mix(n, post_process=True)
            out.append(read_all(sc, nvoices, n))
        spans, _ = sc.launch_stats()
        assert spans == [len(TODO), 0, 0, 0], spans
        sc.close()
        _PER_UPDATE[nvoices] = out
    return _PER_UPDATE[nvoices]


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "output lines", float(np.abs(got[0] - want[0]).max()))
    assert np.array_equal(got[1], want[1]), (what, "carried accumulator", float(np.abs(got[1] - want[1]).max()))
    assert got[2] == want[2], (what, "voice state", [v for v, (a, b) in enumerate(zip(got[2], want[2])) if a != b][:8])


def run_spanned(sc, blocks, upto, between=None):
    for k in range(upto):
        if k:
            sc.apply_block(blocks[k])
        sc.mix(TODO[k], post_process=True)
        if between is not None:
            between(k)


@pytest.mark.parametrize("span", [2, 3, 4])
@pytest.mark.parametrize("nvoices", SIZES)
def test_forced_spans_give_the_values_of_a_launch_per_update(synth_mhr, nvoices, span):
    want = launch_per_update(synth_mhr, nvoices)
    # the scene does what it is there for: the short buffers end in update 0 and are Stopped after update 1, the delayed voices start late
    assert all(want[0][2][v][0] == ol.VOICE_STOPPING and want[1][2][v][0] == ol.VOICE_STOPPED for v in (1, 10)), [want[0][2][v][:2] for v in (1, 10)]
    assert want[3][2][16][0] == ol.VOICE_PLAYING and want[4][2][16][0] == ol.VOICE_STOPPING and want[5][2][16][0] == ol.VOICE_STOPPED
    assert want[0][2][3][1] == (3 * 977) % 8000 and want[1][2][3][1] != (3 * 977) % 8000       # (the delayed start fell into update 1)
    assert float(np.abs(want[0][0]).max()) > 0.01, "the scene must sound"
    for m in range(1, len(TODO) + 1):
        sc = build(product(span), synth_mhr, nvoices)
        sc.set_launch_span(span)
        blocks = make_blocks(sc, nvoices)
        run_spanned(sc, blocks, m)
        got = read_all(sc, nvoices, TODO[m - 1])
        spans, _ = sc.launch_stats()
        sc.close()
        # m updates in launches of `span`, and one launch over what was left
        expect = [0, 0, 0, 0]
        expect[span - 1] += m // span
        if m % span:
            expect[m % span - 1] += 1
        assert spans == expect, (nvoices, span, m, spans, expect)
        same(got, want[m - 1], (nvoices, span, m))


@pytest.mark.parametrize("flush", ["sync", "setter", "readback"])
def test_a_flush_inside_a_forced_span_changes_nothing(synth_mhr, flush):
    nvoices = 1100
    want = launch_per_update(synth_mhr, nvoices)
    sc = build(product(4), synth_mhr, nvoices)
    sc.set_launch_span(4)
    blocks = make_blocks(sc, nvoices)

    def between(k):
        if k != 1 and k != 6:
            return
        if flush == "sync":
            sc.sync()
        elif flush == "setter":
            sc.set_start_delay(nvoices - 1, 0)           # (a value the voice already has: the call only has to flush)
        else:
            assert sc.dry().shape[1] == 1024
    run_spanned(sc, blocks, 8, between)
    got = read_all(sc, nvoices, TODO[7])
    spans, _ = sc.launch_stats()
    sc.close()
    assert spans == [2, 1, 0, 1], spans                 # updates 0-1 | 2-5 | 6 | 7
    same(got, want[7], flush)


def test_a_host_that_reads_every_update_back_never_spans(synth_mhr):
    nvoices = 1100
    want = launch_per_update(synth_mhr, nvoices)
    sc = build(product(0), synth_mhr, nvoices)           # (the automatic rule is the default)
    blocks = make_blocks(sc, nvoices)
    for k, n in enumerate(TODO):
        if k:
            sc.apply_block(blocks[k])
        sc.mix(n, post_process=True)
        assert np.array_equal(sc.dry()[:, :n], want[k][0]), k
    spans, _ = sc.launch_stats()
    sc.close()
    assert spans == [len(TODO), 0, 0, 0], spans


def test_the_automatic_rule_spans_for_a_host_that_runs_ahead(synth_mhr):
    """a host that only submits: the first launch covers one update (the GPU was idle), later ones what was handed over
    while it was busy -- how many is a matter of timing, the values are not"""
    nvoices = 2050
    want = launch_per_update(synth_mhr, nvoices)
    sc = build(product(0), synth_mhr, nvoices)
    blocks = make_blocks(sc, nvoices)
    run_spanned(sc, blocks, len(TODO))
    got = read_all(sc, nvoices, TODO[-1])
    spans, _ = sc.launch_stats()
    sc.close()
    print("automatic rule, 9 updates:", spans)
    assert sum((i + 1) * s for i, s in enumerate(spans)) == len(TODO) and spans[0] >= 1, spans
    same(got, want[-1], "automatic")


def test_span_one_flag_never_spans(synth_mhr):
    import oalgpu
    nvoices = 24
    want = launch_per_update(synth_mhr, nvoices)
    sc = build(product(0, oalgpu.CTX_APPLY_IN_VOICE_KERNEL | oalgpu.CTX_SPAN_ONE), synth_mhr, nvoices)
    blocks = make_blocks(sc, nvoices)
    run_spanned(sc, blocks, len(TODO))
    got = read_all(sc, nvoices, TODO[-1])
    spans, _ = sc.launch_stats()
    sc.close()
    assert spans == [len(TODO), 0, 0, 0], spans
    same(got, want[-1], "span-one flag")


def test_spans_of_three_match_the_reference(synth_mhr):
    """2050 voices, six updates in two launches of three, against the compiled reference: the suite's HRTF tolerance
    (tests/test_tolerance_model.py: voices x 64 serial adds per output sample), integer voice state exact"""
    if not ol.available("ref"):
        pytest.skip("needs the compiled reference (oracle/_ref)")
    L = ol.load("ref")
    L.L.oal_set_simd(1)
    nvoices, updates = 2050, 6
    osc = build(L, synth_mhr, nvoices)
    mv = moving(nvoices)
    for k in range(updates):
        if k:
            for v in mv:
                osc.set_params(v, params_of(v, k))
        osc.mix(TODO[k], post_process=True)
    want_dry, want_acc = osc.dry()[:, :TODO[updates - 1]].copy(), osc.hrtf_accum().copy()
    want_int = [(s.play_state, s.position, s.position_frac, s.has_buffer, s.fading) for s in (osc.voice_state(v) for v in range(nvoices))]
    osc.close()
    sc = build(product(3), synth_mhr, nvoices)
    assert sc.voice_kernel_name() == kernel_for(nvoices, _cus())
    sc.set_launch_span(3)
    blocks = make_blocks(sc, nvoices)
    run_spanned(sc, blocks, updates)
    got_dry, got_acc, got_states = read_all(sc, nvoices, TODO[updates - 1])
    spans, _ = sc.launch_stats()
    sc.close()
    assert spans == [0, 0, 2, 0], spans
    assert [s[:5] for s in got_states] == want_int
    for what, got, want in (("output lines", got_dry, want_dry), ("carried accumulator", got_acc, want_acc)):
        scale = float(np.abs(want).max())
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        bound = multi_voice_tolerance(nvoices, 64, scale)
        print(f"{what}: max err {err:.3e}, bound {bound:.3e}, max|ref| {scale:.3e}")
        assert err <= bound, (what, err, bound)
    assert float(np.abs(want_dry).max()) > 0.01
