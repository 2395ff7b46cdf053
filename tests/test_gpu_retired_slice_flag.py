"""OALGPU_CTX_SLICE_LINES is retired (include/oalgpu.h): oalgpu_context_create accepts the bit and ignores it.
A context created with it runs the kernel of the same context without it and computes the same bits -- on the scenes the flag
once steered: dry lines with sends (a kernel of its own) and HRTF with sends (kept off the voice-per-wavefront kernel)."""
import pytest

import test_delayed_start as delayed
from test_gpu_baseline_configs import run_config

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("vpg", [0, 24], ids=["default_grid", "three_rounds_per_workgroup"])
def test_dry_lines_and_sends_run_the_rows_kernel_with_and_without_the_flag(synth_mhr, vpg):
    """BASELINE configs[3] in small: 5 dry lines, four reverb slots, 67 voices -- nine workgroups of one round, the last ragged, on the
    default grid; three workgroups of three rounds with 24 voices per workgroup (23 = 8 + 8 + 7, 21 = 8 + 8 + 5) -- and updates
    of 1024, 300 and 40 frames (inside the 64-frame gain ramp).  Both contexts meet the reference (run_config) and equal each
    other bit for bit, buses and voice state."""
    import oalgpu
    runs = {flags: [] for flags in (oalgpu.CTX_SLICE_LINES, 0)}
    for flags, got in runs.items():
        run_config(4, 67, synth_mhr, todo=(1024, 300, 40), ctx_flags=flags, expect_kernel="VoiceRowsKernel", vpg=vpg, capture=got)
    assert len(runs[0]) == 3 and runs[oalgpu.CTX_SLICE_LINES] == runs[0]


def test_hrtf_with_sends_keeps_its_kernel_with_the_flag(synth_mhr):
    """HRTF + two sends, synthetic data set, 67 voices, one 1024-frame update: the same kernel and the same bits"""
    import oalgpu
    names, runs = {}, {}
    for flags in (oalgpu.CTX_SLICE_LINES, 0):
        out, ints = delayed.run(oalgpu.Api(oalgpu.MATH_FAST, ctx_flags=flags), synth_mhr, True, 2, nvoices=67, todo=(1024,),
                                on_scene=lambda sc, f=flags: names.__setitem__(f, sc.voice_kernel_name()))
        runs[flags] = ([o.tobytes() for o in out], ints)
    assert names[oalgpu.CTX_SLICE_LINES] == names[0] and "sends" in names[0], names
    assert runs[oalgpu.CTX_SLICE_LINES] == runs[0]


@pytest.mark.parametrize("hrtf", [False, True], ids=["dry_sends", "hrtf_sends"])
@pytest.mark.parametrize("other", ["CTX_PROFILE", "CTX_STREAM_ROWS"])
def test_the_flag_beside_another_form_flag_changes_nothing(synth_mhr, other, hrtf):
    import oalgpu
    names = []
    for flags in (getattr(oalgpu, other) | oalgpu.CTX_SLICE_LINES, getattr(oalgpu, other)):
        api = oalgpu.Api(oalgpu.MATH_FAST, ctx_flags=flags)
        api.hrtf_load(synth_mhr)
        sc = api.make_scene(num_dry=4 if hrtf else 5, num_real=2 if hrtf else 0, num_sends=2, num_slots=2, hrtf=hrtf, max_voices=67)
        names.append(sc.voice_kernel_name())
        sc.close()
    assert names[0] == names[1], names
