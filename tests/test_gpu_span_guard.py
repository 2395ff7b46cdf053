"""ONE guard of the partial-bus sets in front of a voice launch over several deferred updates (GuardPartialSets, RunMixSpan in
csrc/api.hip): the reductions run in order on the post stream, so the event of the newest one that read a set the launch writes
stands for the others.  That changes what the main stream waits for, not arithmetic: every comparison between two runs of the
product is value-exact (np.array_equal) on the output lines, the carried accumulator and the voice states, against a run with
a launch per update (set_launch_span(1)).

The scene and the prefix method are tests/test_gpu_launch_span.py's: reading anything back submits what waits, so the state
after update m of the launch-per-update run is compared with the END of a run of m updates in forced spans, whose last launch
covers what was left.

Whether a query finds its event ready is a matter of timing, and so is the number of waits; how many launches ASK is not: a
launch asks once if any set it writes was read by a reduction the host does not know to be done (eight sets: from the ninth
update on, unless something synchronised), and the counts below are asserted exactly."""
import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_launch_span import build, moving, params_of, product, read_all, same
from test_gpu_wave16_grid import _cus, kernel_for
from test_tolerance_model import multi_voice_tolerance

pytestmark = pytest.mark.gpu

SIZES = (24, 1100)
FULL = (1024,) * 9
MIXED = ((1024, 1024, 1024, 37), (1024, 1024, 64, 1024), (37, 1024, 1024, 1024))


def make_blocks(sc, nvoices, count):
    mv = moving(nvoices)
    blocks = [None]
    for k in range(1, count):
        arr = (ol.VoiceParams * len(mv))(*[params_of(v, k) for v in mv])
        blocks.append(sc.param_block(mv, arr))
    return blocks


def run(sc, blocks, lens, between=None):
    for k, n in enumerate(lens):
        if k:
            sc.apply_block(blocks[k])
        sc.mix(n, post_process=True)
        if between is not None:
            between(k)


_PER_UPDATE = {}


def launch_per_update(mhr, nvoices, lens, every=True):
    """the state after every update (every=False: after the last only, nothing read in between) of a run that never spans:
    computed once per scene size and update lengths, never changed"""
    key = (nvoices, lens, every)
    if key not in _PER_UPDATE:
        sc = build(product(1), mhr, nvoices)
        assert sc.voice_kernel_name() == kernel_for(nvoices, _cus()), sc.voice_kernel_name()
        sc.set_launch_span(1)
        blocks = make_blocks(sc, nvoices, len(lens))
        out = []
        run(sc, blocks, lens, (lambda k: out.append(read_all(sc, nvoices, lens[k]))) if every else None)
        if not every:
            out.append(read_all(sc, nvoices, lens[-1]))
        spans, silent = sc.launch_stats()
        assert spans == [len(lens), 0, 0, 0] and silent == len(lens), (spans, silent)
        guards, queries = sc.guard_stats()
        # a launch per update asks once per update whose set was used before -- unless every update was read back, which tells the host
        assert queries == (0 if every else max(0, len(lens) - 8)) and guards <= queries, (guards, queries)
        sc.close()
        _PER_UPDATE[key] = out
    return _PER_UPDATE[key]


def spanned(mhr, nvoices, span, lens, flags=None, between=None):
    """-> (state at the end, launches by updates covered, silent posts, (main-stream guards, launches that queried))"""
    sc = build(product(span, flags), mhr, nvoices)
    sc.set_launch_span(span)
    blocks = make_blocks(sc, nvoices, len(lens))
    run(sc, blocks, lens, (lambda k: between(sc, k)) if between else None)
    got = read_all(sc, nvoices, lens[-1])
    spans, silent = sc.launch_stats()
    guards = sc.guard_stats()
    sc.close()
    return got, spans, silent, guards


@pytest.mark.parametrize("span", [2, 3, 4])
@pytest.mark.parametrize("nvoices", SIZES)
def test_full_line_spans_keep_the_values(synth_mhr, nvoices, span):
    want = launch_per_update(synth_mhr, nvoices, FULL)
    assert float(np.abs(want[0][0]).max()) > 0.01, "the scene must sound"
    assert float(np.abs(want[-1][1][:128]).max()) > 1e-4, "something must be carried"
    for m in range(1, len(FULL) + 1):
        got, spans, silent, guards = spanned(synth_mhr, nvoices, span, FULL[:m])
        expect = [0, 0, 0, 0]
        expect[span - 1] += m // span
        if m % span:
            expect[m % span - 1] += 1
        assert spans == expect and silent == m, (nvoices, span, m, spans, expect, silent)
        assert guards[1] == (1 if m > 8 else 0) and guards[0] <= guards[1], (m, guards)      # (the ninth update rewrites set 0)
        same(got, want[m - 1], (nvoices, span, m))


@pytest.mark.parametrize("lens", MIXED)
@pytest.mark.parametrize("nvoices", SIZES)
def test_mixed_lengths_keep_the_values(synth_mhr, nvoices, lens):
    want = launch_per_update(synth_mhr, nvoices, lens)
    for m in range(1, len(lens) + 1):
        got, spans, silent, guards = spanned(synth_mhr, nvoices, 4, lens[:m])
        expect = [0, 0, 0, 0]
        expect[m - 1] = 1
        assert spans == expect and silent == m and guards == (0, 0), (lens, m, spans, silent, guards)
        same(got, want[m - 1], (nvoices, lens, m))


@pytest.mark.parametrize("nvoices", SIZES)
def test_sets_rewritten_without_a_read_back_take_one_guard_per_launch(synth_mhr, nvoices):
    lens = (1024,) * 20                         # eight sets, spans of 4: every set is rewritten, sets 0-3 twice
    want = launch_per_update(synth_mhr, nvoices, lens, every=False)
    got, spans, silent, guards = spanned(synth_mhr, nvoices, 4, lens)
    assert spans == [0, 0, 0, 5] and silent == 20, (spans, silent)
    print("(main-stream guards, queries) in front of 5 voice launches:", guards)
    # launches 3, 4 and 5 rewrite four sets each and ask ONCE each (a guard per update asked twelve times)
    assert guards[1] == 3 and guards[0] <= 3, guards
    same(got, want[-1], (nvoices, "20 updates"))


def test_after_a_synchronisation_no_launch_asks(synth_mhr):
    nvoices = 1100
    lens = (1024,) * 16
    want = launch_per_update(synth_mhr, nvoices, lens, every=False)
    got, spans, silent, guards = spanned(synth_mhr, nvoices, 4, lens, between=lambda sc, k: sc.sync() if k == 7 else None)
    # updates 8-15 rewrite all eight sets, whose reductions (updates 0-7) the host knows to be done
    assert spans == [0, 0, 0, 4] and guards == (0, 0), (spans, guards)
    same(got, want[-1], "synchronised after eight updates")


def test_the_whole_post_chain_takes_one_guard_per_launch_too(synth_mhr):
    import oalgpu
    nvoices = 1100
    lens = (1024,) * 21                         # spans of 3: seven launches, sets 0-4 rewritten twice
    want = launch_per_update(synth_mhr, nvoices, lens, every=False)
    got, spans, silent, guards = spanned(synth_mhr, nvoices, 3, lens, oalgpu.CTX_APPLY_IN_VOICE_KERNEL | oalgpu.CTX_FULL_POST)
    # launches 3-7 (sets 6 7 0 | 1 2 3 | ...) each rewrite a set and ask once: the reduction's event, with the post-process behind it
    assert spans == [0, 0, 7, 0] and silent == 0 and guards[1] == 5 and guards[0] <= 5, (spans, silent, guards)
    same(got, want[-1], "whole post chain")


def test_a_dry_writer_in_the_middle_of_a_run_changes_nothing(synth_mhr):
    nvoices = 1100
    def between(sc, k):
        if k == 3:
            sc.bus_device_ptr()                       # (the caller may write the dry lines from here on: sticky; submits updates 0-3)
            assert sc.launch_stats() == ([0, 0, 0, 1], 4)
    lens = (1024,) * 12
    want = launch_per_update(synth_mhr, nvoices, lens, every=False)
    got, spans, silent, guards = spanned(synth_mhr, nvoices, 4, lens, between=between)
    # the third launch rewrites sets 0-3, read by the one-launch posts of updates 0-3, in front of a whole post chain: one query
    assert spans == [0, 0, 0, 3] and silent == 4 and guards[1] == 1 and guards[0] <= 1, (spans, silent, guards)
    same(got, want[-1], "dry writer")


def test_guarded_spans_match_the_reference(synth_mhr):
    """1100 voices, twelve full updates in four launches of three -- the last two rewrite sets whose reductions the guard asks
    about -- against the compiled reference: the suite's HRTF tolerance (tests/test_tolerance_model.py: voices x 64 serial adds
    per output sample), integer voice state exact"""
    if not ol.available("ref"):
        pytest.skip("needs the compiled reference (oracle/_ref)")
    L = ol.load("ref")
    L.L.oal_set_simd(1)
    nvoices, updates = 1100, 12
    osc = build(L, synth_mhr, nvoices)
    mv = moving(nvoices)
    for k in range(updates):
        if k:
            for v in mv:
                osc.set_params(v, params_of(v, k))
        osc.mix(1024, post_process=True)
    want_dry, want_acc = osc.dry()[:, :1024].copy(), osc.hrtf_accum().copy()
    want_int = [(s.play_state, s.position, s.position_frac, s.has_buffer, s.fading) for s in (osc.voice_state(v) for v in range(nvoices))]
    osc.close()
    (got_dry, got_acc, got_states), spans, silent, guards = spanned(synth_mhr, nvoices, 3, (1024,) * updates)
    assert spans == [0, 0, 4, 0] and silent == updates and guards[1] == 2 and guards[0] <= 2, (spans, silent, guards)
    assert [s[:5] for s in got_states] == want_int
    for what, got, want in (("output lines", got_dry, want_dry), ("carried accumulator", got_acc, want_acc)):
        scale = float(np.abs(want).max())
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        bound = multi_voice_tolerance(nvoices, 64, scale)
        print(f"{what}: max err {err:.3e}, bound {bound:.3e}, max|ref| {scale:.3e}")
        assert err <= bound, (what, err, bound)
    assert float(np.abs(want_dry).max()) > 0.01
