"""What oalgpu_effect_* refuses and what it accepts (include/oalgpu.h, csrc/effects_api.hip): argument checks of create, the
order update / set_upsampler / process must be called in, what update needs per kind, the limits of the echo's and the
chorus' delay lines -- each with the message oalgpu_last_error() gives -- and the two shifters' hop counters across
differently sized blocks.  The outputs themselves are compared with the reference in test_effects.py / test_effects2.py.

Shapes: 1 or 4 wet channels (the pitch shifter 9), 4 output lines, blocks of 64 samples; the hop tests feed 1024.

oalgpu_effect_set_upsampler's "at most 32 output lines" cannot be reached through the C-ABI: create refuses more than
OALGPU_MAX_OUTPUT_CHANNELS = 32 lines.  That refusal and the accepted 32 lines are what is checked here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

(EQUALIZER, MODULATOR, ECHO, DEDICATED, COMPRESSOR, CHORUS, DISTORTION, AUTOWAH, VMORPHER, FSHIFTER, PSHIFTER) = range(11)
NAMES = ["equalizer", "modulator", "echo", "dedicated", "compressor", "chorus", "distortion", "autowah", "vmorpher", "fshifter",
         "pshifter"]
# the property struct's fields in declaration order (include/oalgpu.h)
PROPS = {
    EQUALIZER: [200.0, 2.0, 500.0, 0.5, 1.0, 3000.0, 3.0, 0.7, 6000.0, 0.3],
    MODULATOR: [440.0, 800.0, 1],
    ECHO: [0.1, 0.1, 0.5, 0.5, -1.0],
    DEDICATED: None,
    COMPRESSOR: [1],
    CHORUS: [1, 90, 1.1, 0.1, 0.25, 0.016],
    DISTORTION: [0.2, 0.05, 8000.0, 3600.0, 3600.0],
    AUTOWAH: [0.06, 0.06, 1000.0, 11.22],
    VMORPHER: [5.0, 1, 4, 7, -5, 1],
    FSHIFTER: [100.0, 0, 1],
    PSHIFTER: [12, 0],
}
NLINES = 4
BAD_ARGS = "oalgpu_effect_create: bad arguments"
NO_UPDATE = "oalgpu_effect_process: no update() yet"
NO_UPSAMPLER = "oalgpu_effect_set_upsampler: only the chorus, the distortion and the frequency / pitch shifters up-sample"
# update without props or without targets: the first five kinds are named, the others are "this effect"
NEEDS = {k: "oalgpu_effect_update: this effect needs props and targets" for k in range(CHORUS, PSHIFTER + 1)}
NEEDS.update({k: f"oalgpu_effect_update: {NAMES[k]} needs props and targets" for k in (EQUALIZER, MODULATOR, COMPRESSOR)})
ALL_KINDS = pytest.mark.parametrize("kind", range(11), ids=NAMES)


def wet_channels(kind):
    return 9 if kind == PSHIFTER else 4


def make(kind, num_in=None, nlines=NLINES, rate=48000):
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    return oalgpu.Effect(kind, nlines, wet_channels(kind) if num_in is None else num_in, rate, oalgpu.MATH_EXACT)


def refused(message, call, *args):
    """`call` fails and oalgpu_last_error() is exactly `message`"""
    import oalgpu
    with pytest.raises(oalgpu.OalgpuError) as info:
        call(*args)
    assert str(info.value).endswith("): " + message), str(info.value)


def targets(fx):
    """wet channel c onto line c; the wet channels beyond the output lines onto none (OALGPU_INVALID_CHANNEL)"""
    t = np.arange(fx.num_in, dtype=np.uint32)
    t[fx.nlines:] = 0xffffffff
    return t


def gains(fx):
    """enough for every kind: [num_in], the dedicated effect's [nlines], the echo's [2][nlines], an up-sampler's [9][nlines]"""
    return np.full(9 * fx.nlines, 0.5, np.float32)


def block(fx, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((fx.num_in, 1024)) * 0.25).astype(np.float32)


def process(fx, x, n):
    """`n` samples of x through fx, onto silence: out_lines[nlines][n]"""
    wet = np.zeros((fx.num_in, 1024), np.float32)
    wet[:, :n] = x
    out = np.zeros((fx.nlines, 1024), np.float32)
    fx.process(wet, out, n)
    assert not out[:, n:].any(), "samples past n must stay untouched"
    return out[:, :n].copy()


@pytest.mark.parametrize("kind,rate,num_in,nlines", [(-1, 48000, 4, 4), (11, 48000, 4, 4), (ECHO, 7999, 4, 4), (EQUALIZER, 48000, 0, 4),
                                                     (EQUALIZER, 48000, 17, 4), (CHORUS, 48000, 17, 4), (EQUALIZER, 48000, 4, 0),
                                                     (CHORUS, 48000, 4, 33)],
                         ids=["kind_below", "kind_above", "rate_7999", "no_wet_channel", "17_wet_channels", "17_wet_channels_chorus",
                              "no_line", "33_lines"])
def test_create_refuses_bad_arguments(kind, rate, num_in, nlines):
    refused(BAD_ARGS, make, kind, num_in, nlines, rate)


def test_create_refuses_a_pitch_shifter_with_ten_channels():
    refused("oalgpu_effect_create: the pitch shifter works on up to 9 channels (second order)", make, PSHIFTER, 10)
    make(PSHIFTER, 9).close()
    make(FSHIFTER, 16).close()           # the A-Format kinds take the first four of however many there are


def test_create_accepts_the_limits():
    make(EQUALIZER, 1, 1, 8000).close()
    make(EQUALIZER, 16, 32, 8000).close()


@ALL_KINDS
def test_process_before_update_is_refused(kind):
    fx = make(kind)
    x = block(fx)
    refused(NO_UPDATE, process, fx, x[:, :64], 64)
    fx.update(PROPS[kind], None if kind in (ECHO, DEDICATED) else targets(fx), gains(fx))
    assert process(fx, x[:, :64], 64).shape == (NLINES, 64)
    fx.close()


def test_process_after_set_upsampler_needs_another_update():
    fx = make(CHORUS)
    x = block(fx)
    fx.update(PROPS[CHORUS], targets(fx), gains(fx))
    process(fx, x[:, :64], 64)
    fx.set_upsampler(np.array([1.0, 0.8], np.float32), 400.0 / 48000.0)
    refused(NO_UPDATE, process, fx, x[:, :64], 64)
    refused(NO_UPDATE, process, fx, x[:, :64], 64)
    fx.update(PROPS[CHORUS], targets(fx), gains(fx))        # gains: [4][nlines] now
    process(fx, x[:, :64], 64)
    fx.set_upsampler(None, 0.0)                             # first order again: the same rule
    refused(NO_UPDATE, process, fx, x[:, :64], 64)
    fx.update(PROPS[CHORUS], targets(fx), gains(fx))
    process(fx, x[:, :64], 64)
    fx.close()


@pytest.mark.parametrize("kind", sorted(NEEDS), ids=[NAMES[k] for k in sorted(NEEDS)])
def test_update_needs_props_and_targets(kind):
    fx = make(kind, 1 if kind < CHORUS else None)
    refused(NEEDS[kind], fx.update, None, targets(fx), gains(fx))
    refused(NEEDS[kind], fx.update, PROPS[kind], None, gains(fx))
    refused(NEEDS[kind], fx.update, None, None, gains(fx))
    refused(NO_UPDATE, process, fx, block(fx)[:, :64], 64)  # a refused update is no update
    fx.update(PROPS[kind], targets(fx), gains(fx))
    fx.close()


def test_update_of_the_echo_needs_props_only():
    fx = make(ECHO, 1)
    refused("oalgpu_effect_update: echo needs props", fx.update, None, None, gains(fx))
    refused("oalgpu_effect_update: echo needs props", fx.update, None, targets(fx), gains(fx))
    fx.update(PROPS[ECHO], None, gains(fx))
    process(fx, block(fx)[:, :64], 64)
    fx.close()


def test_update_of_the_dedicated_effect_needs_neither():
    fx = make(DEDICATED, 1)
    fx.update(None, None, gains(fx))
    out = process(fx, block(fx)[:, :64], 64)
    assert np.abs(out).max() > 0.0
    fx.close()


def test_update_refuses_null_gains():
    import oalgpu
    fx = make(DEDICATED, 1)
    assert oalgpu.lib.oalgpu_effect_update(fx.h, None, None, None) < 0
    assert oalgpu.lib.oalgpu_last_error().decode() == "oalgpu_effect_update: null argument"
    fx.close()


@ALL_KINDS
def test_set_upsampler_only_for_the_kinds_that_up_sample(kind):
    fx = make(kind)
    scales = np.array([1.0, 0.8], np.float32)
    if kind in (CHORUS, DISTORTION, FSHIFTER, PSHIFTER):
        fx.set_upsampler(scales, 400.0 / 48000.0)
        fx.set_upsampler(None, 0.0)
    else:
        refused(NO_UPSAMPLER, fx.set_upsampler, scales, 400.0 / 48000.0)
        refused(NO_UPSAMPLER, fx.set_upsampler, None, 0.0)
    fx.close()


@pytest.mark.parametrize("kind", [CHORUS, DISTORTION, FSHIFTER, PSHIFTER], ids=["chorus", "distortion", "fshifter", "pshifter"])
def test_set_upsampler_takes_32_lines(kind):
    """(more than 32 cannot exist: test_create_refuses_bad_arguments[33_lines])"""
    fx = make(kind, nlines=32)
    fx.set_upsampler(np.array([1.0, 0.8], np.float32), 400.0 / 48000.0)
    fx.update(PROPS[kind], targets(fx), gains(fx))
    assert process(fx, block(fx)[:, :64], 64).shape == (32, 64)
    fx.close()


def test_echo_delay_line_limits():
    """48 kHz: the line is NextPowerOf2(9936 + 19392) = 32768 samples.  0.207 s + 0.404 s: taps 9936 and 29328, inside;
    0.3 s + 0.404 s: the second tap, 14400 + 19392 = 33792, is past the mask."""
    fx = make(ECHO, 1)
    refused("oalgpu_effect_update: echo delays beyond AL_ECHO_MAX_DELAY + AL_ECHO_MAX_LRDELAY", fx.update,
            [0.3, 0.404, 0.5, 0.5, -1.0], None, gains(fx))
    refused(NO_UPDATE, process, fx, block(fx)[:, :64], 64)
    fx.update([0.207, 0.404, 0.5, 0.5, -1.0], None, gains(fx))
    process(fx, block(fx)[:, :64], 64)
    fx.close()


def test_chorus_delay_line_limit():
    """48 kHz: four lines of NextPowerOf2(1536 + 1) = 2048 samples; 0.05 s are 2400"""
    fx = make(CHORUS)
    refused("oalgpu_effect_update: chorus delay beyond the delay line", fx.update, [1, 90, 1.1, 0.1, 0.25, 0.05], targets(fx), gains(fx))
    fx.update(PROPS[CHORUS], targets(fx), gains(fx))
    process(fx, block(fx)[:, :64], 64)
    fx.close()


@pytest.mark.parametrize("kind,hop", [(PSHIFTER, 128), (FSHIFTER, 256)], ids=["pshifter_8x128", "fshifter_4x256"])
def test_shifter_hops_do_not_depend_on_the_block_size(kind, hop):
    """1024 samples in blocks of one hop and as one block: the same output lines, bit for bit.  A block of 64 comes first, so
    that the gains have reached their targets and every block after it ends in the middle of a hop."""
    outs = []
    for size in (hop, 1024):
        fx = make(kind)
        x, lead = block(fx, 5), block(fx, 6)[:, :64]
        fx.update(PROPS[kind], targets(fx), gains(fx))
        process(fx, lead, 64)
        process(fx, x, 1024)                                # fills the STFT's FIFO: what follows is no longer silence
        outs.append(np.concatenate([process(fx, x[:, at:at + size], size) for at in range(0, 1024, size)], axis=1))
        fx.close()
    assert np.abs(outs[1]).max() > 0.01
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
