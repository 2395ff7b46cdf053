"""The voice-per-wavefront HRTF kernel (VoiceWave16Kernel, csrc/voice_wave16.hip) at every width, on ragged grids and above
4096 voices -- up to the goal's 10 240 -- against the compiled reference.

The kernel puts 4, 8 or 16 voices (one per wavefront) in a workgroup: the narrowest whose grid fits the machine in one
round (Wave16WavesFor), 16 beyond that.  Its grid can be larger than the two-voices-per-wavefront grid the context's partial
buses were once sized for -- above 8192 voices, or with voices_per_group --, so these cases cover:

  (a) every width with and without sends, and the first ragged grid of each (1021, 1025, 2049, 4099 voices: a last
      workgroup with idle wavefronts), on the irregular scene of tests/test_delayed_start.py (delays, a stop before the
      start, non-looping voices, three pitches, every other voice filtered, random directions -- period 6, against the
      kernel's slot rotation of period 4), up to 10 240 voices;
  (b) BASELINE's scenes above 4096 voices (configs 3 and 5 at 10 240, config 3 at 4099 with odd update lengths);
  (c) the block-driven update pipelines at 10 240 voices -- the resident launch has to give up there (640 workgroups of
      sixteen wavefronts: more than 256 compute units hold at once) and the context launches per update instead;
  (d) voices_per_group on HRTF contexts: the narrowest width whose grid fits the partial buses.

Every case asserts the kernel it ran on (the width is computed here the way the library computes it, from the device's
compute units).  Tolerances: tests/test_tolerance_model.py's multi_voice_tolerance -- (voices, 64) for the HRTF
accumulator and the lines fed from it, (voices, 1) for the wet buses; integer voice state exact."""
import numpy as np
import pytest

import oracle_lib as ol
from test_delayed_start import TODO, run
from test_gpu_baseline_configs import REAL_MHR, SCHEDULE, run_config
from test_tolerance_model import multi_voice_tolerance

pytestmark = pytest.mark.gpu


def _cus():
    """device 0's compute units, asked of the HIP runtime the library runs on (hipDeviceGetAttribute,
    hipDeviceAttributeMultiprocessorCount = 63 in hip_runtime_api.h)"""
    import ctypes
    import oalgpu  # noqa: F401  (loads liboalgpu.so, and with it the HIP runtime)
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64.so" in line)
    hip = ctypes.CDLL(path)
    n = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(n), 63, 0) == 0 and n.value > 0, n.value
    return n.value


def waves_for(voices, cus):
    """Wave16WavesFor (csrc/voice_wave16.hip): the narrowest of 4 / 8 whose grid fits the machine in one round, else 16"""
    for w in (4, 8):
        if -(-voices // w) <= cus:
            return w
    return 16


def kernel_for(voices, cus, sends=False, vpg=0):
    """the voice kernel of a FAST HRTF context (csrc/api_hrtf.hip, ChooseWave16): by default the device's width; with
    voices_per_group the narrowest of 4 / 8 / 16 whose grid fits the partial buses, which oalgpu_context_create sizes for
    the larger of the two-voices-per-wavefront grid at that many voices per workgroup and the default width's grid"""
    if vpg == 0:
        w = waves_for(voices, cus)
    else:
        pairs = -(-voices // (4 * max(1, -(-vpg // 4))))
        allocated = max(pairs, -(-voices // waves_for(voices, cus)))
        w = next((w for w in (4, 8, 16) if -(-voices // w) <= allocated), None)
        if w is None:
            return "VoiceWaveKernel<"
    return f"VoiceWave16Kernel<{w}, sends>" if sends else f"VoiceWave16Kernel<{w}>"


def _reference():
    if not ol.available("ref"):
        pytest.skip("needs the compiled reference (oracle/_ref)")
    L = ol.load("ref")
    L.L.oal_set_simd(1)
    return L


# 1021 / 1024: <4> ragged and full; 1025 / 2048: <8>; 2049, 4099: <16> ragged; 8192 / 8193: the last size the two-voices-per-
# wavefront grid covered and the first it did not; 10 240: the goal
VOICES = [1021, 1024, 1025, 2048, 2049, 4099, 8192, 8193, 10240]


@pytest.mark.parametrize("sends", [0, 2])
@pytest.mark.parametrize("nvoices", VOICES)
def test_every_width_on_an_irregular_scene_matches_the_reference(synth_mhr, nvoices, sends):
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    L = _reference()
    want_kernel = kernel_for(nvoices, _cus(), sends=bool(sends))
    names = []
    got, gi = run(oalgpu.Api(oalgpu.MATH_FAST), synth_mhr, True, sends, nvoices=nvoices, split=True,
                  on_scene=lambda sc: names.append(sc.voice_kernel_name()))
    print(f"{nvoices} voices, {sends} sends: {names[0]}")
    assert names == [want_kernel], (names, want_kernel)
    want, wi = run(L, synth_mhr, True, sends, nvoices=nvoices, split=True)
    for k in range(len(TODO)):
        assert gi[k] == wi[k], (nvoices, sends, k, [(v, a, b) for v, (a, b) in enumerate(zip(gi[k], wi[k])) if a != b][:4])
        assert set(got[k]) == set(want[k]) == {"dry", "accum"} | {f"wet{s}" for s in range(sends)}
        for part in want[k]:
            scale = float(np.abs(want[k][part]).max())
            bound = multi_voice_tolerance(nvoices, 1 if part.startswith("wet") else 64, scale)
            err = float(np.abs(got[k][part] - want[k][part]).max())
            assert err <= bound, (nvoices, sends, k, part, err, bound, scale)
        assert float(np.abs(want[k]["dry"]).max()) > 0.01, "the scene must sound"
    assert wi[-1][7][0] == ol.VOICE_STOPPED         # (stopped before its start)


def test_config3_10240_voices_after_updates_1_2_8_50():
    run_config(3, 10240, REAL_MHR, todo=(1024,) * 50, check_at=SCHEDULE, expect_kernel=kernel_for(10240, _cus()))


def test_config3_4099_voices_odd_update_lengths(synth_mhr):
    run_config(3, 4099, synth_mhr, todo=(1024, 1000, 300, 40, 257, 1024), expect_kernel=kernel_for(4099, _cus()))


def test_config5_10240_voices(synth_mhr):
    run_config(5, 10240, synth_mhr, expect_kernel=kernel_for(10240, _cus(), sends=True))


@pytest.mark.parametrize("mode", ["plain", "apply_in_voice_kernel", "fused_reduce", "resident"])
def test_config3_block_driven_contexts_at_10240_voices(mode):
    """bench.py's timed loop at 10 240 voices, fifty updates.  OALGPU_CTX_RESIDENT: 640 workgroups of sixteen wavefronts are
    more than the device holds at once (at most two per compute unit), so the resident launch gives up and the context
    launches per update -- with the same results."""
    import oalgpu
    flags = {"plain": 0, "apply_in_voice_kernel": oalgpu.CTX_APPLY_IN_VOICE_KERNEL, "fused_reduce": oalgpu.CTX_FUSED_REDUCE,
             "resident": oalgpu.CTX_RESIDENT}[mode]
    assert -(-10240 // 16) > 2 * _cus()
    run_config(3, 10240, REAL_MHR, todo=(1024,) * 50, check_at=SCHEDULE, ctx_flags=flags, via_blocks=True,
               expect_kernel=kernel_for(10240, _cus()), resident_fits=False)


@pytest.mark.parametrize("nvoices,vpg", [(512, 8), (1000, 12), (4096, 16), (4096, 32)])
def test_voices_per_group_on_hrtf_contexts(synth_mhr, nvoices, vpg):
    """bench.build_scene (bench.py --vpg) with voices_per_group: the data set loads, the kernel is the one the rule gives"""
    run_config(3, nvoices, synth_mhr, vpg=vpg, expect_kernel=kernel_for(nvoices, _cus(), vpg=vpg))
