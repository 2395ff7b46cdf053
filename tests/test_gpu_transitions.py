"""Playing voices whose filters, gains, directions and play state change (tests/transition_cases.py) on every voice kernel
form, against the compiled reference (or, where oracle/_ref is absent, the restatement pinned to it bit for bit).

Every role of a schedule plays on one scene.  After every update every voice's integer state -- play state, position,
fraction, has-buffer, fading, the HRIR delays and the counters of the direct pair and of send 0's pair -- must equal the
reference's, the buses must meet the multi-voice tolerance of tests/test_tolerance_model.py, every filter's targets must be
the reference's bits (both sides design them with the host's libm), its current coefficients must be within
COEFF_TOLERANCE (eight times the rounding noise of the reference's own lerpf chain) and the current gains within 16 float32
ulps (2e-6 relative, floor 1e-6: a lerpf is two operations; derived, not measured -- the largest disagreement seen is
printed, so that the figure can be tightened; on the MI355X it was 0 for coefficients and gains on every form and path:
the kernels' lerpf is not contracted, and a gain ramp of min(samplesToMix, 64) samples ends at its target inside the
update).  tests/test_transitions_host.py shows on the reference that every role
reaches its branch and that missing its transition moves the output by more than 100x the tolerance.

The delivery tests hand the parameters over as blocks: applied by a parameter kernel, installed by the update's own voice
kernel (contexts that defer the update: params(k + 1) go in right behind update k, and the state is read with them
installed -- between the install and the next update is also the only place where a retargeted filter's own counter
shows), and installed by the resident launch."""
from functools import lru_cache

import numpy as np
import pytest

import transition_cases as tc
from test_gpu_loop_edges import FORMS, _api, _oracle, compare

pytestmark = pytest.mark.gpu

COEFFS, TARGETS = slice(2, 7), slice(7, 12)         # of Biquad.as_tuple()
SEEN = {"coeff": 0.0, "gain": 0.0}


@lru_cache(maxsize=None)
def _want(schedule, kind, mhr, roles=None, mixed=True, total=None, early=False):
    """the reference's run of a scene, shared by the forms and delivery paths that mix the same scene"""
    return tc.run(_oracle(), schedule, kind, mhr=mhr, roles=roles, mixed=mixed, total=total, early=early)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def compare_floats(got, want, what):
    """targets bit for bit, current coefficients within COEFF_TOLERANCE of max(|x|, 1), current gains within GAIN_RTOL of
    max(|x|, GAIN_FLOOR)"""
    gf, wf = got[2]["floats"], want[2]["floats"]
    assert got[2]["roles"] == want[2]["roles"] and len(gf) == len(wf)
    for k in range(len(wf)):
        assert gf[k].keys() == wf[k].keys(), (what, k)
        for name, w in wf[k].items():
            g = gf[k][name]
            for key in w:
                if key in ("hrtf_old_gain", "dry_current"):
                    a, b = np.atleast_1d(np.float64(g[key])), np.atleast_1d(np.float64(w[key]))
                    rel = float((np.abs(a - b) / np.maximum(np.abs(b), tc.GAIN_FLOOR)).max())
                    SEEN["gain"] = max(SEEN["gain"], rel)
                    assert rel <= tc.GAIN_RTOL, f"{what}: update {k}, {name}.{key}: {g[key]} vs the reference's {w[key]}"
                    continue
                assert _bits(g[key][TARGETS]) == _bits(w[key][TARGETS]), \
                    f"{what}: update {k}, {name}.{key}: targets {g[key][TARGETS]} vs the reference's {w[key][TARGETS]}"
                a, b = np.float64(g[key][COEFFS]), np.float64(w[key][COEFFS])
                rel = float((np.abs(a - b) / np.maximum(np.abs(b), 1.0)).max())
                SEEN["coeff"] = max(SEEN["coeff"], rel)
                assert rel <= tc.COEFF_TOLERANCE, \
                    f"{what}: update {k}, {name}.{key}: coefficients {g[key][COEFFS]} vs the reference's {w[key][COEFFS]}"
    print(f"{what}: largest disagreement so far: coefficients {SEEN['coeff']:.3e} (bound {tc.COEFF_TOLERANCE:.1e}), "
          f"gains {SEEN['gain']:.3e} (bound {tc.GAIN_RTOL:.1e})")


@pytest.mark.parametrize("schedule", list(tc.SCHEDULES))
@pytest.mark.parametrize("form", list(FORMS))
def test_transitions_match_the_reference(form, schedule, synth_mhr):
    mode, flags, kind, kernel = FORMS[form]
    hrtf = kind.startswith("hrtf")
    mhr = synth_mhr if hrtf else None
    names = []
    got = tc.run(_api(mode, flags), schedule, kind, mhr=mhr, scene_kw=dict(max_voices=128), kernel_names=names)
    assert names == [kernel], names
    want = _want(schedule, kind, mhr)
    what = f"{form} {schedule}"
    compare(got, want, what, (len(want[1][0]), 64 if hrtf else 1))
    compare_floats(got, want, what)


@pytest.mark.parametrize("schedule", list(tc.SCHEDULES))
@pytest.mark.parametrize("role", list(tc.ROLES))
def test_exact_one_voice_bit_for_bit(role, schedule, synth_mhr):
    """EXACT contexts with one role voice per scene, on dry lines and through the HRTF mix: buses, integer state, the whole
    float state of the direct pair (delay elements, current and target coefficients) and the current gains, bit for bit.
    `hrir` included: tests/test_gpu_parity.py's single-voice EXACT HRTF scenes, whose voice moves, are bit-exact today."""
    api, L = _api("exact", 0), _oracle()
    for kind in ("dry", "hrtf"):
        if role not in tc.role_names(kind):
            continue
        mhr = synth_mhr if kind == "hrtf" else None
        names = []
        gb, gi, gx = tc.run(api, schedule, kind, mhr=mhr, roles=(role,), mixed=False, kernel_names=names)
        wb, wi, wx = _want(schedule, kind, mhr, roles=(role,), mixed=False)
        assert names == ["VoiceMixKernel<true, LINES>"], names
        assert gi == wi, (kind, role, schedule, gi, wi)
        a, b = np.concatenate(gb), np.concatenate(wb)
        assert float(np.abs(b).max()) > 0.01
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (kind, role, schedule, float(np.abs(a - b).max()))
        for k, w in enumerate(wx["floats"]):
            assert gx["floats"][k].keys() == w.keys()
            for key, val in w.get(role, {}).items():
                assert _bits(gx["floats"][k][role][key]) == _bits(val), (kind, role, schedule, k, key, gx["floats"][k][role][key], val)


def _resident_voices():
    """the smallest scene the resident launch of the voice-per-wavefront kernel takes: more than 8 voices per compute unit
    (its 16-wavefront form, tests/test_gpu_wave16_grid.py waves_for)"""
    from test_gpu_wave16_grid import _cus, waves_for
    n = 8 * _cus() + 1
    assert waves_for(n, _cus()) == 16 and waves_for(n - 1, _cus()) == 8
    return n


# name: (context flags, delivery, params(k + 1) in behind update k, the kernel that must mix the scene)
PATHS = {
    "block": (0, "block", False, "VoiceWave16Kernel<4>"),
    "block_early": (0, "block", True, "VoiceWave16Kernel<4>"),
    "block_in_voice_kernel": ("CTX_APPLY_IN_VOICE_KERNEL", "block", True, "VoiceWave16Kernel<4>"),
    "block_in_voice_kernel_wave_pairs": ("CTX_APPLY_IN_VOICE_KERNEL|CTX_WAVE_PAIRS", "block", True,
                                         "VoiceWaveKernel<17, 64, 0, false, true>"),
    "block_fused_reduce": ("CTX_FUSED_REDUCE", "block", False, "VoiceWave16Kernel<4>"),
    "run_resident": ("CTX_RESIDENT", "run", False, "VoiceWave16Kernel<16>"),
    "run_resident_wave_pairs": ("CTX_RESIDENT|CTX_WAVE_PAIRS", "run", False, "VoiceWaveKernel<17, 64, 0, false, true>"),
}


def _flags(text):
    import oalgpu
    out = 0
    for name in (text.split("|") if text else []):
        out |= getattr(oalgpu, name)
    return out


def _delivery(kind, schedule, flags, delivery, early, kernel, mhr, total=None, resident=False):
    names, stats = [], []
    got = tc.run(_api("fast", _flags(flags)), schedule, kind, mhr=mhr, delivery=delivery, roles=tc.DELIVERY_ROLES, total=total,
                 early=early, scene_kw=dict(max_voices=total or 128), kernel_names=names, stats=stats if resident else None)
    assert names == [kernel], names
    if resident:
        st = stats[0]
        assert st["enabled"] == 1 and st["failed"] == 0 and st["updates"] == len(tc.SCHEDULES[schedule]), st
    want = _want(schedule, kind, mhr, roles=tc.DELIVERY_ROLES, total=total, early=early)
    what = f"{kind} {schedule} {delivery} on {flags or 'a plain context'}{' (early)' if early else ''}"
    compare(got, want, what, (total or len(want[1][0]), 64 if kind.startswith("hrtf") else 1))
    compare_floats(got, want, what)


@pytest.mark.parametrize("schedule", ["even", "short"])
@pytest.mark.parametrize("path", list(PATHS))
def test_delivery_paths(path, schedule, synth_mhr):
    """The HRTF scene with its parameters as blocks: applied by the parameter kernel (in front of the update, and right
    behind the update before), installed by the voice kernel of the update before (contexts that defer their update, both
    HRTF kernels), in front of a fused reduction, and through oalgpu_mix_update_run on resident contexts of both kernels
    (updates of differing lengths included: every update goes through the doorbell)."""
    flags, delivery, early, kernel = PATHS[path]
    resident = "CTX_RESIDENT" in (flags or "")
    total = _resident_voices() if path == "run_resident" else None
    _delivery("hrtf", schedule, flags or "", delivery, early, kernel, synth_mhr, total=total, resident=resident)


@pytest.mark.parametrize("schedule", ["even", "short"])
@pytest.mark.parametrize("form", ["register_lines", "rows"])
def test_delivery_paths_on_line_kernels(form, schedule):
    """Dry-line contexts that defer their update: the voice kernel of the update before installs the block -- direct and send
    filters retargeted in flight by the line kernels' record installs."""
    _, _, kind, kernel = FORMS[form]
    _delivery(kind, schedule, "CTX_APPLY_IN_VOICE_KERNEL", "block", True, kernel, None)
