"""Static voices at the edges of their loops (tests/loop_edge_cases.py) on every voice kernel form that mixes static voices,
against the compiled reference (or, where oracle/_ref is absent, the restatement pinned to it bit for bit).

Every case of a pitch plays on one scene; after every update every voice's integer state (play state, position, fraction,
has-buffer, fading) must match exactly, and the buses must meet the multi-voice tolerance of tests/test_tolerance_model.py.
The edge voices play at gain 0.5 and the fillers at 1e-3, so one wrong sample of one edge voice exceeds that bound by far
more than 100x (tests/test_loop_edges_host.py checks on the oracle that each case reaches its edge).  Each scene runs with
all edge voices on one resampler key (the register gather of the wavefront kernels is eligible) and with every fourth voice
a filler on another key (the same voices take the generic loader).  EXACT contexts: one voice per scene, bit for bit."""
import numpy as np
import pytest

import loop_edge_cases as lc
import oracle_lib as ol
from test_tolerance_model import multi_voice_tolerance

pytestmark = pytest.mark.gpu

FORMS = {   # name: (math mode, context flags, scene form, the kernel that must mix it)
    "wave16": ("fast", 0, "hrtf", "VoiceWave16Kernel<4>"),
    "wave_pairs": ("fast", "CTX_WAVE_PAIRS", "hrtf", "VoiceWaveKernel<17, 64, 0, false, true>"),
    "fir_valu": ("fast", "CTX_FIR_VALU", "hrtf", "VoiceWaveKernel<17, 64, 0, false>"),
    "wave16_sends": ("fast", 0, "hrtf_sends", "VoiceWave16Kernel<4, sends>"),
    "register_lines": ("fast", 0, "dry", "VoiceWaveKernel<17, 64, 1, false, false, false, DeviceLayout, 6>"),
    "rows": ("fast", 0, "dry_sends", "VoiceRowsKernel"),
    "stream_rows": ("fast", "CTX_STREAM_ROWS", "dry_sends", "VoiceWaveKernel<17, 64, 1, true>"),
    "exact_hrtf": ("exact", 0, "hrtf", "VoiceMixKernel<true, LINES>"),
    "exact_dry_sends": ("exact", 0, "dry_sends", "VoiceMixKernel<true, LINES>"),
}


def _oracle():
    L = ol.load("ref" if ol.available("ref") else "port")
    L.L.oal_set_simd(1)
    return L


def _api(mode, flags):
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    if isinstance(flags, str):
        flags = getattr(oalgpu, flags)
    return oalgpu.Api(oalgpu.MATH_EXACT if mode == "exact" else oalgpu.MATH_FAST, ctx_flags=flags)


def compare(got, want, what, terms):
    gb, gi, _ = got
    wb, wi, _ = want
    assert len(gi) == len(wi)
    for k in range(len(wi)):
        for v in range(len(wi[k])):
            assert gi[k][v] == wi[k][v], f"{what}: update {k}, voice {v}: {gi[k][v]} vs the reference's {wi[k][v]}"
        scale = float(np.abs(wb[k]).max())
        err = float(np.abs(gb[k].astype(np.float64) - wb[k].astype(np.float64)).max())
        bound = multi_voice_tolerance(terms[0], terms[1], scale)
        assert err <= bound, f"{what}: update {k}: max err {err:.3e}, bound {bound:.3e} (max|ref| {scale:.3e})"
        assert bound * 100 < 0.1, "an edge voice's one-sample error must exceed the bound by 100x"
    assert max(float(np.abs(b).max()) for b in wb) > 0.1, "the scene must sound"


def _steps_and_fracs():
    out = [(s, False) for s in lc.STEPS]
    out.insert(4, (lc.FRAC_ONE, True))            # step 1.0 without a fraction: the 1:1 copy
    return out


STEPS = _steps_and_fracs()
STEP_IDS = [f"{s}{'_frac0' if z else ''}" for s, z in STEPS]


@pytest.mark.parametrize("mixed", [False, True], ids=["one_key", "mixed_keys"])
@pytest.mark.parametrize("step,frac_zero", STEPS, ids=STEP_IDS)
@pytest.mark.parametrize("form", list(FORMS))
def test_loop_edges_match_the_reference(form, step, frac_zero, mixed, synth_mhr):
    mode, flags, kind, kernel = FORMS[form]
    hrtf = kind.startswith("hrtf")
    mhr = synth_mhr if hrtf else None
    names = []
    kw = dict(mhr=mhr, mixed=mixed, frac_zero=frac_zero)
    got = lc.run(_api(mode, flags), step, kind, scene_kw=dict(max_voices=128), kernel_names=names, **kw)
    assert names == [kernel], names
    want = lc.run(_oracle(), step, kind, **kw)
    compare(got, want, f"{form} step {step}", (len(want[1][0]), 64 if hrtf else 1))


def _exact_subset(step, frac_zero):
    """one case per branch, plus the cases around the wrap"""
    voices = lc.scene(step, frac_zero)
    pick, seen = [], set()
    for i, v in enumerate(voices):
        if v.branch not in seen or v.name.startswith(("boundary_equal", "loop1_", "tiny1_", "past_loop_end")):
            seen.add(v.branch)
            pick.append(i)
    return pick


@pytest.mark.parametrize("step,frac_zero", [(1, False), (60211, False), (lc.FRAC_ONE, True), (65537, False),
                                            (131072, False), (lc.MAX_PITCH, False)],
                         ids=["1", "60211", "65536_frac0", "65537", "131072", "655360"])
def test_exact_mode_one_voice_bit_for_bit(step, frac_zero):
    """EXACT contexts (the workgroup-per-voice-group kernel) with one edge voice per scene: bit for bit, buses and state."""
    api = _api("exact", 0)
    L = _oracle()
    picks = _exact_subset(step, frac_zero)
    assert len(picks) >= 5
    for i in picks:
        names = []
        gb, gi, _ = lc.run(api, step, "dry", only=[i], frac_zero=frac_zero, kernel_names=names)
        wb, wi, _ = lc.run(L, step, "dry", only=[i], frac_zero=frac_zero)
        assert names == ["VoiceMixKernel<true, LINES>"], names
        name = lc.scene(step, frac_zero)[i].name
        assert gi == wi, (step, name, gi, wi)
        a, b = np.concatenate(gb), np.concatenate(wb)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (step, name, float(np.abs(a - b).max()))


from test_gpu_wave16_grid import _cus, waves_for  # noqa: E402


@pytest.mark.parametrize("step", [60211, 65537])
def test_4096_hrtf_voices_edges_spread_over_the_machine(step, synth_mhr):
    """The machine-filling HRTF scene: 4096 voices on VoiceWave16Kernel<16>, the edge voices spread across its workgroups
    and the rest quiet fillers on another resampler key."""
    assert waves_for(4096, _cus()) == 16
    names = []
    kw = dict(mhr=synth_mhr, total=4096)
    got = lc.run(_api("fast", 0), step, "hrtf", scene_kw=dict(max_voices=4096), kernel_names=names, **kw)
    assert names == ["VoiceWave16Kernel<16>"], names
    want = lc.run(_oracle(), step, "hrtf", **kw)
    compare(got, want, f"4096 voices, step {step}", (4096, 64))


def test_block_driven_resident_context(synth_mhr):
    """bench.py's timed path: the parameters as a block resident in HBM, the updates through oalgpu_mix_update_run on an
    OALGPU_CTX_RESIDENT context of 4096 HRTF voices."""
    names, stats = [], []
    kw = dict(mhr=synth_mhr, total=4096, todo=(1024,) * 5)
    got = lc.run(_api("fast", "CTX_RESIDENT"), 60211, "hrtf", scene_kw=dict(max_voices=4096),
                 kernel_names=names, via_blocks=True, stats=stats, **kw)
    assert names == ["VoiceWave16Kernel<16>"], names
    assert stats[0]["enabled"] == 1 and stats[0]["failed"] == 0 and stats[0]["updates"] == 5, stats
    want = lc.run(_oracle(), 60211, "hrtf", **kw)
    compare(got, want, "resident, block-driven", (4096, 64))
