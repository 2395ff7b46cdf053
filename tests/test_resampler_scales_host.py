"""CPU side of the resampler-scale cases (tests/resampler_scale_cases.py): the steps reach every scale index and tap
count of every bsinc table, the numpy restatement of one resampled sample is the oracle's bit for bit, and -- on that
restatement -- one wrong argument of the resampler (the rows of a neighbouring scale, sf = 0, the window one sample off,
the neighbouring phase) moves a tested voice by more than 100x the tolerance the GPU tests grant its scene.  So a kernel
that picked a wrong row set, tap count or window for one scale cannot pass tests/test_gpu_resampler_scales.py."""
from functools import lru_cache

import numpy as np
import pytest

import loop_edge_cases as lc
import resampler_scale_cases as rc
from test_tolerance_model import multi_voice_tolerance

BSINC = tuple(rc.FAMILY)
IDS = [rc.NAMES[r] for r in rc.RESAMPLERS]
TAPS = {12: {12, 16, 20, 24}, 24: {24, 28, 32, 36, 40, 44, 48}, 48: {48}}


@pytest.mark.parametrize("resampler", BSINC, ids=[rc.NAMES[r] for r in BSINC])
def test_steps_reach_every_scale_and_tap_count(resampler):
    L = rc.oracle()
    steps = rc.steps_for(resampler)
    assert {rc.scale_of(resampler, s.step)[0] for s in steps} == set(range(16))
    assert {rc.scale_of(resampler, s)[0] for s in rc.middle_steps(resampler)} == set(range(16))
    assert {L.prepare_resampler(resampler, s.step).m for s in steps} == TAPS[rc.FAMILY[resampler]]
    by_role = {(s.si, s.role): s.step for s in steps}
    for si in range(15):
        low, mid, high = by_role[si, "low"], by_role[si, "middle"], by_role[si, "high"]
        assert rc.FRAC_ONE < low <= mid <= high <= rc.MAX_PITCH
        for s in (low, mid, high):
            st = L.prepare_resampler(resampler, s)
            assert rc.scale_of(resampler, s)[0] == si and st.m == rc.tables(rc.FAMILY[resampler])["m"][si]
            assert st.l == st.m // 2 - 1 and st.kind == (4 if resampler in rc.FULL_BSINC else 3)
        assert rc.scale_of(resampler, low - 1)[0] == si + 1             # the ends really are ends
        if si > 0:
            assert rc.scale_of(resampler, high + 1)[0] == si - 1
        else:
            assert high == rc.MAX_PITCH
        f = rc.scale_of(resampler, mid)[1]
        assert 0.5 <= f <= 0.9, (si, mid, f)                            # the full bsinc's sf is far from 0
        if resampler in rc.FULL_BSINC:
            assert L.prepare_resampler(resampler, mid).sf > 0.1
    for s in rc.TOP_SCALE_STEPS:
        st = L.prepare_resampler(resampler, s)
        assert rc.scale_of(resampler, s)[0] == 15 and st.kind == 3 and st.sf == 0.0


@pytest.mark.parametrize("resampler", rc.PLAIN, ids=[rc.NAMES[r] for r in rc.PLAIN])
def test_plain_resampler_steps(resampler):
    assert rc.middle_steps(resampler) == (30000, 65536, 65537, 100000, 300000, 655360)


@pytest.mark.parametrize("family", [12, 24, 48])
def test_the_products_tap_counts_are_the_oracles(family):
    import oalgpu
    mine, ref = oalgpu.Api().bsinc_table(family), rc.tables(family)
    assert mine["m"] == ref["m"] and mine["filterOffset"] == ref["filterOffset"]
    assert set(ref["m"]) == TAPS[family]
    for resampler in (r for r in BSINC if rc.FAMILY[r] == family):
        for s in rc.steps_for(resampler):
            a, b = oalgpu.Api().prepare_resampler(resampler, s.step), rc.oracle().prepare_resampler(resampler, s.step)
            assert (a.kind, a.table, a.m, a.l, a.filter_offset) == (b.kind, b.table, b.m, b.l, b.filter_offset), s
            assert np.float32(a.sf).view(np.uint32) == np.float32(b.sf).view(np.uint32), s


def _source(n, seed=3):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


@pytest.mark.parametrize("resampler", rc.RESAMPLERS, ids=IDS)
def test_the_restatement_is_the_oracles_bit_for_bit(resampler):
    L = rc.oracle()
    n = 43                                          # not a multiple of 4: the SSE4.1 cubic's main loop and its tail
    for step in rc.middle_steps(resampler):
        for frac in (0, 40000):
            src = _source(((n * step + frac) >> 16) + 128, seed=step % 1000)
            want = L.resample(resampler, step, src, frac, n)
            got = rc.resample_call(resampler, step, src, frac, n)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (step, frac, np.abs(got - want).max())


def test_todo_fits_the_window_then_exceeds_it():
    for resampler in rc.RESAMPLERS:
        for s in rc.steps_for(resampler):
            n_fit, whole, short = rc.todo_for(s.step)
            assert 64 <= n_fit <= 1024 and whole == 1024 and short == 37
            for frac in (0, 12345, rc.FRAC_MASK):
                assert lc.calc_buffer_size(frac, s.step, n_fit) == (n_fit, lc.calc_buffer_size(frac, s.step, n_fit)[1])
                assert lc.calc_buffer_size(frac, s.step, n_fit)[1] <= lc.WINDOW
            assert n_fit == 1024 or lc.calc_buffer_size(rc.FRAC_MASK, s.step, n_fit + 1)[1] > lc.WINDOW
            if s.step > 1.1 * rc.FRAC_ONE:
                assert all(lc.calc_buffer_size(f, s.step, 1024)[1] > lc.WINDOW for f in (0, rc.FRAC_MASK)), s
        steps = rc.middle_steps(resampler)
        assert rc.moving_todo(steps)[0] == min(rc.todo_for(s)[0] for s in steps) >= 64
    # no voice starts without a fraction: step 1.0 resamples, it is not the 1:1 copy
    assert all(rc.voice_start(i)[2] != 0 for i in range(4096))
    assert {rc.voice_start(i)[0] for i in range(8)} == {0, 1, 2, 3}


# ---- sensitivity ------------------------------------------------------------------------------------------------------
KINDS = ("hrtf", "hrtf_sends", "dry", "dry_sends")


@lru_cache(maxsize=None)
def _granted(layout, resampler, steps, mhr):
    """the largest tolerance tests/test_gpu_resampler_scales.py grants a scene of these steps, over the scene forms and
    the scene's updates: multi_voice_tolerance(voices, 64, max|reference bus|)"""
    worst = 0.0
    for kind in KINDS:
        buses, ints, _ = rc.run(rc.oracle(), layout, resampler, steps, kind, mhr=mhr)
        worst = max(worst, max(multi_voice_tolerance(len(ints[0]), 64, float(np.abs(b).max())) for b in buses))
    return worst


def _perturbations(resampler, step):
    s = rc.state_of(resampler, step)
    out = {"l-1": dict(l=s["l"] - 1), "l+1": dict(l=s["l"] + 1)}
    if s["kind"] >= 2:
        out.update({"phase-1": dict(dphase=-1), "phase+1": dict(dphase=1)})
    if s["kind"] >= 3:
        for d in (-1, 1):
            if 0 <= s["si"] + d <= 15:
                out[f"si{d:+d}"] = dict(si=s["si"] + d)
    if s["kind"] == 4:
        out["sf=0"] = dict(sf=0.0)
    return s, out


@pytest.mark.parametrize("resampler", rc.RESAMPLERS, ids=IDS)
def test_one_wrong_argument_exceeds_the_tolerance_100_fold(resampler, synth_mhr):
    """Per middle step, on tested voice 0 as the scenes start it (a float buffer, gain 0.5): each wrong argument moves
    the voice's resampled signal by more than 100x what the step's one_key scene is granted.  The moving scene carries
    all steps at once, so its buses -- and with them its tolerance -- are several times larger than a heavily
    low-passed voice of its lowest scales: there the margin asserted is 10x."""
    steps = rc.middle_steps(resampler)
    moving = _granted("moving", resampler, steps, synth_mhr)
    for step in steps:
        granted = _granted("one_key", resampler, (step,), synth_mhr)
        assert granted < moving < 1e-3
        b, pos, frac = rc.voice_start(0)
        assert b == 0
        n = min(rc.todo_for(step)[0], 256)
        noise = rc.buffer_noise(700 + b).astype(np.float32)
        need = ((n * step + frac) >> 16) + 128
        src = np.take(noise, np.arange(pos - rc.MAX_EDGE, pos - rc.MAX_EDGE + need), mode="wrap")
        base = rc.resample_call(resampler, step, src, frac, n)
        state, perturbed = _perturbations(resampler, step)
        if resampler in rc.FAMILY:
            assert {"l-1", "l+1", "phase-1", "phase+1"} <= set(perturbed) and ("si-1" in perturbed or "si+1" in perturbed)
            assert ("sf=0" in perturbed) == (resampler in rc.FULL_BSINC and step > rc.FRAC_ONE)
        for name, kw in perturbed.items():
            other = rc.resample_call(resampler, step, src, frac, n, **kw)
            moved = rc.TESTED_GAIN * float(np.abs(other.astype(np.float64) - base).max())
            assert moved > 100 * granted, (rc.NAMES[resampler], step, state, name, moved, granted)
            assert moved > 10 * moving, (rc.NAMES[resampler], step, state, name, moved, moving)
