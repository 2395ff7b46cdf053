"""The front stabilizer's and the distance compensation's host side (no GPU): oalgpu_distance_comp_from_distances against the
float32 restatement of InitDistanceComp (tests/stabilizer_cases.py), the stabilizer's host constants against libm's cosf / sinf
and the compiled reference's BandSplitter::init, the setters' refusals that need no device, and a sanity check of the reference
composition the GPU tests compare with."""
import numpy as np
import pytest

import oracle_lib as ol
import stabilizer_cases as sc

RATES = (44100, 48000, 96000)
DISTANCES = {
    "with a zero": [2.0, 2.5, 0.0, 3.0, 1.2, 2.999, 3.0, 0.5],
    "all equal": [2.5] * 8,
    "all zero": [0.0] * 8,
    "negative and zero": [-1.0, 0.0, -0.5],
    "one far enough to clamp": [1.0, 30.0, 29.0, 0.0, 27.5, 22.7, 30.0, 26.0],
    "a single channel": [4.0],
}


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("case", list(DISTANCES))
def test_distance_comp_from_distances_is_init_distance_comp(rate, case):
    import oalgpu
    d = DISTANCES[case]
    delays, gains, any_delay = oalgpu.distance_comp_from_distances(rate, d)
    want_delays, want_gains, want_any = sc.init_distance_comp(rate, d)
    assert np.array_equal(delays, want_delays), (delays, want_delays)
    assert np.array_equal(gains.view(np.uint32), want_gains.view(np.uint32)), (gains, want_gains)
    assert any_delay == want_any
    assert delays.max(initial=0) <= sc.MAX_DELAY
    if case == "one far enough to clamp":
        assert delays[0] == sc.MAX_DELAY and delays[3] == 0 and gains[3] == 1.0 and any_delay
    if case in ("all equal", "all zero", "negative and zero", "a single channel"):
        assert not any_delay and not delays.any()
    if case == "with a zero":
        assert delays[2] == 0 and gains[2] == 1.0 and delays[3] == 0 and delays[0] > 0


def test_distance_comp_from_distances_refuses_bad_arguments():
    import oalgpu
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.distance_comp_from_distances(0, [1.0, 2.0])
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.distance_comp_from_distances(48000, [])
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.distance_comp_from_distances(48000, [1.0] * 33)


@pytest.mark.parametrize("rate", RATES)
def test_stabilizer_constants_are_the_reference_bits(rate):
    import oalgpu
    f0 = np.float32(5000.0) / np.float32(rate)                  # CreateStablizer: 5000.0f / float(srate)
    k = oalgpu.front_stabilizer_constants(f0)
    want = np.array(sc.pan_constants(), np.float32)
    assert np.array_equal(k[1:].view(np.uint32), want.view(np.uint32)), (k[1:], want)
    assert abs(float(k[1]) - np.cos(np.pi / 6)) < 1e-6 and abs(float(k[4]) - np.sin(np.pi / 8)) < 1e-6
    if not sc.available():
        pytest.skip("the coefficient needs the compiled reference")
    ref = sc.RefBandSplitter(f0)
    assert np.array_equal(k[:1].view(np.uint32), ref.mem[:1].view(np.uint32)), (k[0], ref.coeff)
    assert -1.0 < float(k[0]) < 0.0


def test_stabilizer_constants_refuse_a_bad_crossover():
    import oalgpu
    for bad in (0.0, -0.1, 0.5, 0.7, float("nan")):
        with pytest.raises(oalgpu.OalgpuError):
            oalgpu.front_stabilizer_constants(bad)


def test_reference_composition_pans_a_centred_source_onto_the_centre_line():
    """silence in the direct lines and equal L and R feeds: the side stays zero (L == R afterwards), the centre line gains
    energy, and L + R and C hold the shares of the input energy that the two pan angles give"""
    if not sc.available():
        pytest.skip("needs the compiled reference")
    rng = np.random.default_rng(11)
    st = sc.RefStabilizer(8, 0, 1, 2, 5000.0 / 48000.0)
    energy_c, energy_lr, energy_in = 0.0, 0.0, 0.0
    for n in (1024, 17, 1000, 1, 1024):
        feed = rng.uniform(-0.5, 0.5, n).astype(np.float32)

        def decode(out, feed=feed, n=n):
            out[0, :n] += feed
            out[1, :n] += feed
            out[4, :n] += np.float32(0.25) * feed

        got = st.process(np.zeros((8, 1024), np.float32), n, decode)
        assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))          # side == 0
        assert not got[[3, 5, 6, 7]].any()
        energy_c += float(np.sum(got[2].astype(np.float64) ** 2))
        energy_lr += float(np.sum(got[:2].astype(np.float64) ** 2))
        energy_in += 2.0 * float(np.sum(feed.astype(np.float64) ** 2))
    # mid = 2 feed; per band L = R = feed cos(a) and C = feed sin(a) with a = pi/6 (low) or pi/8 (high): of the input energy
    # 2 feed^2, L + R keep cos^2(a) = 0.75 .. 0.854 and C gets sin^2(a) / 2 = 0.073 .. 0.125 (the bands' cross terms aside)
    assert 0.70 * energy_in < energy_lr < 0.90 * energy_in, (energy_lr, energy_in)
    assert 0.06 * energy_in < energy_c < 0.14 * energy_in, (energy_c, energy_in)


def test_expected_distance_comp_is_a_delay_and_a_gain_over_the_run():
    rng = np.random.default_rng(3)
    delays, gains = [0, 1, 300, 1023], np.array([0.5, 1.0, 0.93, 0.25], np.float32)
    exp = sc.DistanceCompExpected(delays, gains)
    x = rng.uniform(-1, 1, (4, 6000)).astype(np.float32)
    pos, outs = 0, []
    for n in (1024, 17, 1, 1000, 129, 1024, 1024, 700):
        outs.append(exp.process(x[:, pos:pos + n], n))
        pos += n
    y = np.concatenate(outs, axis=1)
    assert np.array_equal(y[0], x[0, :pos])                                            # delay 0: the gain is not applied
    for i, d in enumerate(delays[1:], 1):
        assert not y[i, :d].any()
        assert np.array_equal(y[i, d:], x[i, :pos - d] * gains[i])
