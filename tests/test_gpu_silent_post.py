"""The one-launch reduce-and-shift of an HRTF update whose dry lines have no writer (BusReduceShiftKernel, csrc/voice_kernel.hip;
ReduceShiftSilent, csrc/api.hip) against the chain it replaces -- the reduction, then the whole post-process (band split,
decoder FIR, shift), which OALGPU_CTX_FULL_POST keeps.  The post-process of silent dry lines adds exactly nothing, and the
additions that are left are made per element as before: every comparison is value-exact (np.array_equal).

oalgpu_context_launch_stats says which path an update took, so a case cannot pass because the shortcut never ran."""
import numpy as np
import pytest

import attach_cases as ac
from test_gpu_launch_span import build, moving, params_of, product
import oracle_lib as ol

pytestmark = pytest.mark.gpu

TODO = (1024, 1000, 64, 37, 1024, 300, 1, 1024)
NVOICES = 1100


def flags(full_post):
    """the shortcut belongs to the contexts that defer their updates (OALGPU_CTX_APPLY_IN_VOICE_KERNEL); every read-back of
    these cases submits what waits, so the updates are launched one by one unless a case says otherwise"""
    import oalgpu
    return oalgpu.CTX_APPLY_IN_VOICE_KERNEL | (oalgpu.CTX_FULL_POST if full_post else 0)


def scene(synth_mhr, full_post):
    return build(product(0, flags(full_post)), synth_mhr, NVOICES)


def step(sc, k, split=False):
    """update k: the moved voices' parameters, then the update -- as one call or as voices + post-process"""
    if k:
        mv = moving(NVOICES)
        sc.set_params_batch(mv, (ol.VoiceParams * len(mv))(*[params_of(v, k) for v in mv]))
    if split:
        sc.mix_voices(TODO[k])
        sc.post_process(TODO[k])
    else:
        sc.mix(TODO[k], post_process=True)
    return sc.dry()[:, :TODO[k]].copy(), sc.hrtf_accum().copy()


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "output lines", float(np.abs(got[0] - want[0]).max()))
    assert np.array_equal(got[1], want[1]), (what, "carried accumulator", float(np.abs(got[1] - want[1]).max()))


_FULL = {}


def full_chain(synth_mhr):
    """dry + real lines and carried accumulator after every update of the whole chain (computed once, never changed)"""
    if "run" not in _FULL:
        sc = scene(synth_mhr, True)
        _FULL["run"] = [step(sc, k) for k in range(len(TODO))]
        assert sc.launch_stats()[1] == 0
        sc.close()
        assert float(np.abs(_FULL["run"][0][0][4:]).max()) > 0.01, "the scene must sound"
        assert not np.any(_FULL["run"][-1][0][:4]), "nothing writes the dry lines of this context"
    return _FULL["run"]


def test_reduce_and_shift_gives_the_values_of_the_whole_chain(synth_mhr):
    want = full_chain(synth_mhr)
    sc = scene(synth_mhr, False)
    for k in range(len(TODO)):
        assert_same(step(sc, k), want[k], k)
    assert sc.launch_stats()[1] == len(TODO)
    sc.close()


@pytest.mark.parametrize("first", ["update", "split"])
def test_switching_between_the_update_and_its_two_halves(synth_mhr, first):
    """oalgpu_mix_update on the shortcut and oalgpu_mix_voices + oalgpu_post_process (which reduce into the bus block and
    post-process in full) find each other's carried accumulator, whichever buffer it is in"""
    want = full_chain(synth_mhr)
    sc = scene(synth_mhr, False)
    for k in range(len(TODO)):
        split = (k >= 3) == (first == "update")          # three updates one way, then the other -- and back for the last two
        if k >= 6:
            split = not split
        assert_same(step(sc, k, split), want[k], (first, k))
    assert 0 < sc.launch_stats()[1] < len(TODO)
    sc.close()


def test_contexts_that_do_not_defer_keep_the_whole_chain(synth_mhr):
    want = full_chain(synth_mhr)
    sc = build(product(0, 0), synth_mhr, NVOICES)
    for k in range(3):
        assert_same(step(sc, k), want[k], k)
    assert sc.launch_stats()[1] == 0
    sc.close()


def test_spanned_updates_take_the_shortcut_too(synth_mhr):
    want = full_chain(synth_mhr)
    sc = scene(synth_mhr, False)
    sc.set_launch_span(3)
    mv = moving(NVOICES)
    blocks = [None] + [sc.param_block(mv, (ol.VoiceParams * len(mv))(*[params_of(v, k) for v in mv])) for k in range(1, len(TODO))]
    for k in range(len(TODO)):
        if k:
            sc.apply_block(blocks[k])
        sc.mix(TODO[k], post_process=True)
    got = sc.dry()[:, :TODO[-1]].copy(), sc.hrtf_accum().copy()
    spans, silent = sc.launch_stats()
    sc.close()
    assert spans == [0, 1, 2, 0] and silent == len(TODO), (spans, silent)
    assert_same(got, want[-1], "spans of three")


def test_an_attached_context_ends_the_shortcut_for_good(synth_mhr):
    """three updates on the shortcut, then a context is attached (its lines merge into the dry lines: the splitters see
    signal), two updates later detached: the run equals the one that kept the whole chain throughout, and after the
    detach the context stays on the whole chain (the splitters hold state)"""
    import oalgpu

    def run(full_post):
        api = product(0, flags(full_post))
        sc = build(api, synth_mhr, NVOICES)
        child, _, _ = ac.build_child(api, max_voices=6)
        out = []
        for k in range(len(TODO)):
            if k == 3:
                sc.attach(child, ac.CHILD_MAP)
            if k == 5:
                child.detach()
            out.append(step(sc, k))
        stats = sc.launch_stats()[1]
        sc.close()
        child.close()
        return out, stats
    want, none = run(True)
    got, silent = run(False)
    assert none == 0 and silent == 3, (none, silent)
    assert np.any(want[3][0][:4]), "the attached context must reach the dry lines"
    for k in range(len(TODO)):
        assert_same(got[k], want[k], k)
