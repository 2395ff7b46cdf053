"""Every resampler at every scale index of its bsinc table (tests/resampler_scale_cases.py) on every voice kernel form,
against the compiled reference (or, where oracle/_ref is absent, the restatement pinned to it bit for bit).

The per-call resampler runs every step of steps_for, the ends of each scale's step range included.  The scenes play the
middle steps: `one_key` scenes put one resampler at one step on every voice, so the workgroup's key voice carries it and
the voices take the staged coefficient rows wherever the form stages that tap count; the `moving` scene carries all of
a resampler's middle steps at once and moves every voice to the next step between updates, next to fillers on another
key.  After every update every voice's integer state must equal the reference's and every bus must meet the multi-voice
tolerance of tests/test_tolerance_model.py; tests/test_resampler_scales_host.py shows that rows of a neighbouring scale,
sf = 0, a window one sample off or a neighbouring phase move a tested voice by more than 100x that tolerance."""
from functools import lru_cache

import numpy as np
import pytest

import oracle_lib as ol
import resampler_scale_cases as rc
from test_gpu_loop_edges import FORMS, _api, _oracle, compare

pytestmark = pytest.mark.gpu

IDS = [rc.NAMES[r] for r in rc.RESAMPLERS]
FAST_RTOL, FAST_ATOL = 2e-5, 1e-7               # tests/test_gpu_parity.py: MULTI_RTOL, MULTI_ATOL


@pytest.mark.parametrize("resampler", rc.RESAMPLERS, ids=IDS)
def test_per_call_resample_every_scale(resampler):
    exact, fast, L = _api("exact", 0), _api("fast", 0), _oracle()
    rng = np.random.default_rng(300 + resampler)
    for s in rc.steps_for(resampler):
        for frac in (0, 40000):
            need = ((1021 * s.step + frac) >> 16) + 128
            n = 1021 if need <= 65536 else 301
            src = rng.uniform(-1, 1, ((n * s.step + frac) >> 16) + 128).astype(np.float32)
            want = L.resample(resampler, s.step, src, frac, n)
            got = exact.resample(resampler, s.step, src, frac, n)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
                (s, frac, "exact", float(np.abs(got - want).max()))
            got = fast.resample(resampler, s.step, src, frac, n)
            err = float(np.abs(got.astype(np.float64) - want).max())
            bound = FAST_RTOL * float(np.abs(want).max()) + FAST_ATOL
            assert err <= bound, (s, frac, "fast", err, bound)


@lru_cache(maxsize=None)
def _want(layout, resampler, steps, kind, mhr, nvoices=None):
    """the reference's run of a scene, shared by the forms that mix the same kind of scene"""
    return rc.run(_oracle(), layout, resampler, steps, kind, mhr=mhr, nvoices=nvoices)


def _check(form, layout, resampler, steps, synth_mhr):
    mode, flags, kind, kernel = FORMS[form]
    hrtf = kind.startswith("hrtf")
    mhr = synth_mhr if hrtf else None
    names = []
    got = rc.run(_api(mode, flags), layout, resampler, steps, kind, mhr=mhr, scene_kw=dict(max_voices=128),
                 kernel_names=names)
    assert names == [kernel], names
    want = _want(layout, resampler, steps, kind, mhr)
    compare(got, want, f"{form} {layout} {rc.NAMES[resampler]} steps {steps}", (len(want[1][0]), 64 if hrtf else 1))


@pytest.mark.parametrize("resampler", rc.RESAMPLERS, ids=IDS)
@pytest.mark.parametrize("form", list(FORMS))
def test_one_key(form, resampler, synth_mhr):
    for step in rc.middle_steps(resampler):
        _check(form, "one_key", resampler, (step,), synth_mhr)


@pytest.mark.parametrize("resampler", rc.RESAMPLERS, ids=IDS)
@pytest.mark.parametrize("form", list(FORMS))
def test_moving_scales(form, resampler, synth_mhr):
    _check(form, "moving", resampler, rc.middle_steps(resampler), synth_mhr)


@pytest.mark.parametrize("resampler", rc.RESAMPLERS, ids=IDS)
def test_exact_one_voice_bit_for_bit(resampler):
    """EXACT contexts with one voice per scene: bit for bit, buses and state."""
    api = _api("exact", 0)
    for step in rc.middle_steps(resampler):
        names = []
        gb, gi, _ = rc.run(api, "one_key", resampler, (step,), "dry", nvoices=1, kernel_names=names)
        wb, wi, _ = _want("one_key", resampler, (step,), "dry", None, 1)
        assert names == ["VoiceMixKernel<true, LINES>"], names
        assert gi == wi, (step, gi, wi)
        a, b = np.concatenate(gb), np.concatenate(wb)
        assert float(np.abs(b).max()) > 0.1
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (step, float(np.abs(a - b).max()))


# ---- the resident context: staged rows kept from one update to the next -----------------------------------------------
RESIDENT_VOICES = 4096
# tested voices: whole heads of four workgroups of VoiceWave16Kernel<16> (16 g is the key voice of workgroup g; its rows are
# the ones staged, and kept while the key stays), and two voices whose key voice is a filler
RESIDENT_TESTED = [16 * g + d for g in (0, 37, 101, 255) for d in (0, 1, 2, 7)] + [16 * 3 + 5, 16 * 200 + 9]


def _by_taps(resampler, wanted):
    """middle steps of a resampler whose tap counts are `wanted`, in order, each at a scale index not used before"""
    steps, used = [], set()
    for m in wanted:
        for step in rc.middle_steps(resampler):
            si, _, st = rc.scale_of(resampler, step)
            if st.m == m and si not in used:
                used.add(si)
                steps.append(step)
                break
        else:
            raise AssertionError((resampler, m))
    return steps


def _resident_run(L, resampler, steps, mhr, scene_kw=None, kernel_names=None, stats=None):
    """Five 1024-sample updates of 4096 HRTF voices through parameter blocks; block k re-tunes the tested voices to
    steps[k] (the last update keeps the step before it)."""
    L.hrtf_load(mhr)
    sc = L.make_scene(num_dry=4, num_real=2, num_sends=0, num_slots=0, wet_channels=4, hrtf=True, **(scene_kw or {}))
    if kernel_names is not None:
        kernel_names.append(sc.voice_kernel_name())
    rng = np.random.default_rng(5)
    cc = np.zeros((4, 128, 2), np.float32)
    cc[:, :64] = rng.uniform(-0.2, 0.2, (4, 64, 2))
    sc.set_direct_hrtf(cc, [1.0, 0.8, 0.8, 0.8], 400.0 / 48000.0, 64)
    bufs = []
    for b in range(4):
        fmt = ol.FMT_FLOAT if b % 2 == 0 else ol.FMT_SHORT
        bufs.append(sc.add_buffer(rc.lc.encode(rc.buffer_noise(700 + b), fmt), fmt))
    tested = set(RESIDENT_TESTED)

    def params(i, step):
        r = np.random.default_rng(1000 + i)
        hrtf = (r.uniform(-0.5, 0.5), r.uniform(-np.pi, np.pi), 2.0, 0.0)
        if i in tested:
            return ol.make_voice_params(step, resampler, hrtf=hrtf + (rc.TESTED_GAIN,))
        return ol.make_voice_params(rc.FILLER_STEP, rc.FILLER_RESAMPLER, hrtf=hrtf + (rc.FILLER_GAIN,))

    for i in range(RESIDENT_VOICES):
        b, pos, frac = rc.voice_start(i)
        sc.add_voice(bufs[b], looping=True, position=pos, frac=frac)
    via_blocks = hasattr(sc, "param_block")
    blocks = []
    for k, step in enumerate(steps):
        ids = list(range(RESIDENT_VOICES)) if k == 0 else sorted(tested)
        ps = [params(i, step) for i in ids]
        blocks.append((ids, ps, sc.param_block(np.array(ids), (ol.VoiceParams * len(ps))(*ps)) if via_blocks else None))
    if via_blocks:
        sc.resident_set_short_run(0)
    buses, ints = [], []
    for k in range(5):
        if via_blocks:
            sc.mix_run([blocks[k][2] if k < len(blocks) else None], 1024, post_process=True)
        else:
            if k < len(blocks):
                for i, p in zip(blocks[k][0], blocks[k][1]):
                    sc.set_params(i, p)
            sc.mix(1024, post_process=True)
        buses.append(np.concatenate([sc.dry().ravel(), sc.hrtf_accum().ravel()]))
        sts = []
        for i in sorted(tested) + [4, 16 * 37 + 3, 4095]:
            st = sc.voice_state(i)
            sts.append((st.play_state, st.position, st.position_frac, st.has_buffer, st.fading))
        ints.append(sts)
    if stats is not None:
        stats.append(sc.resident_stats())
    sc.close()
    return buses, ints, sorted(tested)


@pytest.mark.parametrize("resampler,taps", [(ol.RS_FAST_BSINC12, (24, 20, 24, 12)), (ol.RS_FAST_BSINC24, (48, 44, 48, 24))],
                         ids=["fast_bsinc12", "fast_bsinc24"])
def test_resident_rows_follow_the_key_voice(resampler, taps, synth_mhr):
    """An OALGPU_CTX_RESIDENT context keeps the staged coefficient rows from one update to the next while the key
    voice's row set stays: parameter blocks move the tested voices, key voices among them, through scales of other tap
    counts, back to the first tap count at another scale index, and to the top scale; the fifth update keeps the fourth's."""
    steps = _by_taps(resampler, taps)
    assert len({rc.scale_of(resampler, s)[0] for s in steps}) == 4
    names, stats = [], []
    got = _resident_run(_api("fast", "CTX_RESIDENT"), resampler, steps, synth_mhr,
                        scene_kw=dict(max_voices=RESIDENT_VOICES), kernel_names=names, stats=stats)
    assert names == ["VoiceWave16Kernel<16>"], names
    assert stats[0]["enabled"] == 1 and stats[0]["failed"] == 0 and stats[0]["updates"] == 5, stats
    want = _resident_run(_oracle(), resampler, steps, synth_mhr)
    compare(got, want, f"resident, {rc.NAMES[resampler]} steps {steps}", (RESIDENT_VOICES, 64))
