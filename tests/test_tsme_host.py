"""The stereo TSME encoder's host side (no GPU): the delays oalgpu_tsme_encoder_delay reports against the reference's getDelay,
and the two restatements the GPU kernels follow (tests/tsme_cases.py) against the compiled reference's own encoders over ragged
updates with non-zero direct lines: the serial float32 IIR bit for bit, the float64 direct FIR to the rounding of the
reference's own float32 FFT path.

That last figure is what the GPU tests' FIR bound is made of (tsme_cases.FIR_GPU_BOUND = ten times it): the worst
|restated - reference| / line max, measured here as 1.453e-7 for FIR-256 and 1.330e-7 for FIR-512.  The test prints it and
asserts that it has not grown past the recorded figure by more than a quarter, so that the bound stays tied to what it was
derived from."""
import numpy as np
import pytest

import tsme_cases as tc

SIZES = (1024, 17, 47, 128, 129, 1000, 700, 1, 1024, 1024, 909)


def _need_ref():
    if not tc.available():
        pytest.skip("needs the compiled reference")


def _inputs(seed, n):
    rng = np.random.default_rng(seed)
    w, y, z, x, left, right = rng.uniform(-1.0, 1.0, (6, n)).astype(np.float32)
    return w, y, z, x, np.float32(0.3) * left, np.float32(0.3) * right


def test_delays():
    import oalgpu
    assert (oalgpu.TSME_IIR, oalgpu.TSME_FIR256, oalgpu.TSME_FIR512) == (0, 1, 2)
    assert [oalgpu.tsme_encoder_delay(q) for q in (oalgpu.TSME_IIR, oalgpu.TSME_FIR256, oalgpu.TSME_FIR512)] == [1, 256, 384]
    assert oalgpu.tsme_encoder_delay(-1) == 0 and oalgpu.tsme_encoder_delay(3) == 0
    _need_ref()
    for q in range(3):
        assert oalgpu.tsme_encoder_delay(q) == tc.ref_delay(q), q


def _compare(quality, exact):
    """-> the worst |restated - reference| / line max over the run"""
    _need_ref()
    ref, mine = tc.RefTsmeEncoder(quality), tc.restated(quality)
    worst, peak = 0.0, 0.0
    for k, n in enumerate(SIZES):
        args = _inputs(100 * quality + k, n)
        want = ref.encode(*args)
        got = mine.encode(*args)
        for g, w in zip(got, want):
            peak = max(peak, float(np.abs(w).max()))
            if exact:
                assert np.array_equal(np.asarray(g, np.float32).view(np.uint32), w.view(np.uint32)), (quality, k, n)
            else:
                worst = max(worst, float(np.abs(np.asarray(g, np.float64) - w).max()))
    assert peak > 0.5
    return worst / peak


def test_iir_restatement_is_the_reference_bit_for_bit():
    _compare(0, True)


@pytest.mark.parametrize("quality", [1, 2])
def test_fir_restatement_matches_the_reference(quality):
    ratio = _compare(quality, False)
    print(f"TSME FIR quality {quality}: worst |restated - reference| / line max {ratio:.3e}")
    assert ratio <= 1.25 * tc.FIR_RESTATEMENT_RATIO, ratio


def test_the_encoding_is_stereo_compatible():
    """a source straight ahead encodes to equal left and right (D carries only j(WX), which the sum cancels), a source to the
    left mostly to the left line: the restated IIR form over a steady tone"""
    t = np.arange(4096)
    tone = np.sin(2.0 * np.pi * 440.0 / 48000.0 * t).astype(np.float32)
    zero = np.zeros_like(tone)
    rt3 = np.float32(np.sqrt(3.0))
    front = tc.IirRestated().encode(tone, zero, zero, rt3 * tone, zero, zero)            # N3D: X = sqrt(3) cos(az)
    left = tc.IirRestated().encode(tone, rt3 * tone, zero, zero, zero, zero)             # Y = sqrt(3) sin(az)
    e = [float(np.sum(np.asarray(a[1024:], np.float64) ** 2)) for a in (*front, *left)]
    assert abs(e[0] / e[1] - 1.0) < 1e-3, e
    assert e[2] > 2.5 * e[3], e                     # (|S + D|^2 : |S - D|^2 = 0.945 : 0.281 for a hard-left source)
