"""The stereo UHJ encoder's host side (no GPU): the delays oalgpu_uhj_encoder_delay reports against the reference's getDelay,
and the two restatements the GPU kernels follow (tests/uhj_cases.py) against the compiled reference's own encoders over
ragged updates with non-zero direct lines: the serial float32 IIR bit for bit, the float64 direct FIR to 1e-6."""
import numpy as np
import pytest

import uhj_cases as uc

SIZES = (1024, 17, 47, 128, 129, 1000, 700, 1, 1024, 1024, 909)


def _need_ref():
    if not uc.available():
        pytest.skip("needs the compiled reference")


def _inputs(seed, n):
    rng = np.random.default_rng(seed)
    w, x, y, left, right = rng.uniform(-1.0, 1.0, (5, n)).astype(np.float32)
    return w, x, y, np.float32(0.3) * left, np.float32(0.3) * right


def test_delays():
    import oalgpu
    assert [oalgpu.uhj_encoder_delay(q) for q in (oalgpu.UHJ_IIR, oalgpu.UHJ_FIR256, oalgpu.UHJ_FIR512)] == [1, 256, 384]
    assert oalgpu.uhj_encoder_delay(-1) == 0 and oalgpu.uhj_encoder_delay(3) == 0
    if uc.available():
        for q in range(3):
            assert oalgpu.uhj_encoder_delay(q) == uc.ref_delay(q), q


def _compare(quality, bound):
    _need_ref()
    ref, mine = uc.RefUhjEncoder(quality), uc.restated(quality)
    worst, peak = 0.0, 0.0
    for k, n in enumerate(SIZES):
        args = _inputs(100 * quality + k, n)
        want = ref.encode(*args)
        got = mine.encode(*args)
        for g, w in zip(got, want):
            peak = max(peak, float(np.abs(w).max()))
            if bound == 0.0:
                assert np.array_equal(np.asarray(g, np.float32).view(np.uint32), w.view(np.uint32)), (quality, k, n)
            else:
                err = float(np.abs(np.asarray(g, np.float64) - w).max())
                worst = max(worst, err)
                assert err <= bound, (quality, k, n, err)
    assert peak > 0.5
    return worst


def test_iir_restatement_is_the_reference_bit_for_bit():
    _compare(0, 0.0)


@pytest.mark.parametrize("quality", [1, 2])
def test_fir_restatement_matches_the_reference(quality):
    worst = _compare(quality, 1e-6)
    print(f"FIR quality {quality}: worst |err| {worst:.2e}")

