"""Register and LDS budgets of what the spanning voice launch and the reduce-and-shift launch add, from the compiler's own
metadata (tests/test_kernel_resources.py's method; no GPU needed).

* The bounded-run forms of the voice-per-wavefront HRTF kernel (csrc/voice_wave16.hip, SPAN) keep the launched forms' budget:
  no scratch -- not even a reserved private segment: its set-up is paid per dispatch --, the 16-wavefront form at most 112
  registers (four voice wavefronts and one of the post stream's on a SIMD) and 123 LDS granules, the 8-wavefront form twice
  per compute unit, the 4-wavefront form two wavefronts per SIMD.
* BusReduceShiftKernel (csrc/voice_kernel.hip) runs on the post stream beside the next voice launch, where BusReduceKernel<4>
  ran: it must fit where that one fits."""
from test_kernel_resources import full_metadata, granule, kernel_metadata, makefile_flags
from test_kernel_resources import pytestmark  # noqa: F401  (no hipcc: nothing to ask)


def test_bounded_run_forms_keep_the_launched_forms_budget(tmp_path):
    _, per_file = makefile_flags()
    assert "-disable-machine-licm" in per_file["voice_wave16"]
    meta, _ = full_metadata(tmp_path, "voice_wave16.hip")
    # VoiceWave16Kernel<PROF = false, WAVES, SENDS = false, RES = false, SPAN = true>
    span = {w: next(m for n, m in meta.items() if f"VoiceWave16KernelILb0ELi{w}ELb0ELb0ELb1E" in n) for w in (4, 8, 16)}
    launched = {w: next(m for n, m in meta.items() if f"VoiceWave16KernelILb0ELi{w}ELb0ELb0ELb0E" in n) for w in (4, 8, 16)}
    for w, m in span.items():
        assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (w, m)
        assert m["group_segment_fixed_size"] == launched[w]["group_segment_fixed_size"], (w, m)
    regs = {w: m["vgpr_count"] + m.get("agpr_count", 0) for w, m in span.items()}
    assert regs[16] <= 112, span[16]
    assert granule(span[16]["group_segment_fixed_size"], 1280) == 123 * 1280, span[16]
    assert 4 * granule(regs[8]) <= 512 and 2 * granule(span[8]["group_segment_fixed_size"], 1280) <= 160 * 1024, span[8]
    assert regs[4] <= 256, span[4]


def test_reduce_and_shift_fits_where_the_reduction_fits(tmp_path):
    vk = kernel_metadata(tmp_path, "voice_kernel.hip")
    reduce4 = next(m for n, m in vk.items() if "BusReduceKernelILi4E" in n)
    shift = next(m for n, m in vk.items() if "BusReduceShiftKernel" in n)
    assert shift["vgpr_spill_count"] == 0 and shift["private_segment_fixed_size"] == 0, shift
    assert granule(shift["vgpr_count"]) <= granule(reduce4["vgpr_count"]), (shift, reduce4)
    assert shift["group_segment_fixed_size"] <= reduce4["group_segment_fixed_size"], (shift, reduce4)
    meta, _ = full_metadata(tmp_path, "voice_wave16.hip")
    for tag in ("ELb0ELb0ELb0E", "ELb0ELb0ELb1E"):        # the launched and the bounded-run 16-wavefront form
        k16 = next(m for n, m in meta.items() if "VoiceWave16KernelILb0ELi16" + tag in n)
        assert 4 * granule(k16["vgpr_count"] + k16.get("agpr_count", 0)) + granule(shift["vgpr_count"]) <= 512, (k16, shift)
        assert granule(k16["group_segment_fixed_size"], 1280) + granule(shift["group_segment_fixed_size"], 1280) <= 160 * 1024, (k16, shift)
