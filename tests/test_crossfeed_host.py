"""The bs2b crossfeed's host side (no GPU): oalgpu_crossfeed_constants against the compiled reference's
bs2b_processor::set_params bit for bit (all six levels at six sample rates, the five floats read out of the object), the
levels it refuses, and the float32 restatement of cross_feed the GPU kernel follows (tests/crossfeed_cases.py) against the
reference's own cross_feed bit for bit over block sizes that straddle its 128-sample staging."""
import numpy as np
import pytest

import crossfeed_cases as cc

RATES = (8000, 22050, 44100, 48000, 96000, 192000)
SIZES = (1024, 127, 128, 129, 1, 255, 256, 257, 17, 1000, 640)


def _need_ref():
    if not cc.available():
        pytest.skip("needs the compiled reference")


def test_level_constants_are_the_reference_enum():
    import oalgpu
    assert (oalgpu.BS2B_LOW, oalgpu.BS2B_MIDDLE, oalgpu.BS2B_HIGH, oalgpu.BS2B_LOW_EASY, oalgpu.BS2B_MIDDLE_EASY,
            oalgpu.BS2B_HIGH_EASY) == cc.LEVELS


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("level", cc.LEVELS)
def test_constants_are_the_reference_bits(level, rate):
    import oalgpu
    k = oalgpu.crossfeed_constants(level, rate)
    assert k.dtype == np.float32 and k.shape == (5,)
    # a0_lo, b1_lo, a0_hi, a1_hi, b1_hi: a low-pass and a high-boost with poles inside the unit circle
    assert 0.0 < k[0] < 1.0 and 0.0 < k[1] < 1.0 and 0.0 < k[2] and k[3] < 0.0 and 0.0 < k[4] < 1.0
    _need_ref()
    want = cc.RefBs2b(level, rate).constants
    assert np.array_equal(k.view(np.uint32), want.view(np.uint32)), (level, rate, k, want)


def test_constants_refuse_levels_outside_one_to_six():
    import oalgpu
    for bad in (0, -1, 7, 100):
        with pytest.raises(oalgpu.OalgpuError):
            oalgpu.crossfeed_constants(bad, 48000)
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.crossfeed_constants(oalgpu.BS2B_LOW, 0)


@pytest.mark.parametrize("level,rate", [(1, 44100), (3, 48000), (6, 48000), (5, 8000)])
def test_restatement_is_cross_feed_bit_for_bit(level, rate):
    _need_ref()
    ref = cc.RefBs2b(level, rate)
    mine = cc.Restated(ref.constants)
    rng = np.random.default_rng(10 * level + rate)
    peak = 0.0
    for k, n in enumerate(SIZES):
        left, right = rng.uniform(-1.0, 1.0, (2, n)).astype(np.float32)
        if k == 5:
            left[:] = 0.0                               # a silent line between busy ones: the histories decay
        want = ref.cross_feed(left, right)
        got = mine.cross_feed(left, right)
        for g, w in zip(got, want):
            peak = max(peak, float(np.abs(w).max()))
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (level, rate, k, n, float(np.abs(g - w).max()))
    assert peak > 0.5


def test_cross_feed_keeps_a_mono_signal_at_unity_at_dc():
    """the filter's design: hi(0) + lo(0) = 1 at DC (a0_hi + a1_hi) / (1 - b1_hi) + a0_lo / (1 - b1_lo), so a constant equal
    input on both lines comes out as it went in"""
    _need_ref()
    ref = cc.RefBs2b(6, 48000)
    x = np.full(1024, 0.5, np.float32)
    for _ in range(8):
        left, right = ref.cross_feed(x, x)
    assert np.array_equal(left.view(np.uint32), right.view(np.uint32))
    assert abs(float(left[-1]) - 0.5) < 1e-4, left[-1]
