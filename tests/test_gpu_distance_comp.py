"""Speaker distance compensation (oalgpu_set_distance_comp) against out[t] = gain * x[t - delay] over the run
(tests/stabilizer_cases.DistanceCompExpected: ApplyDistanceComp is file-local in the reference and its bridge renders without
ChannelDelays, so this statement is the yardstick), bit for bit.

Two contexts run the same 7.1 scene, one without compensation and one with it; the expected lines are made from the first
one's.  Updates are ragged, so both branches of ApplyDistanceComp (SamplesToDo >= delay and < delay) and n = 1 occur; one line
has delay 0 and a gain that is not 1, and must come through unscaled.  Behind the compensation the reference's own dither and
Write<T> (its bridge) give the expected PCM."""
import numpy as np
import pytest

import bridge_lib as bl
import limiter_cases as lc
import stabilizer_cases as sc

from test_gpu_stabilizer import XOVER, _api, _check_kernel, _install, _need, _reference, _sizes

pytestmark = pytest.mark.gpu
LAYOUT = "7.1"
ND = sc.LAYOUTS[LAYOUT]["num_dry"]
DELAYS = (0, 1, 5, 300, 1023, 64, 17, 0)
GAINS = (0.5, 1.0, 0.93, 0.8, 0.71, 0.66, 1.25, 1.0)


def _run(mode, sizes, comp=None, events=None, no_real=False, decoder=True):
    """every update's bus lines of a fresh 7.1 scene (decoder and dedicated slot on, so that every real line carries signal);
    comp: (delays, gains) set before the first update; events: {update: f(scene)}"""
    scene, fx, update = sc.build_scene(_api(mode), LAYOUT, dedicated=not no_real, no_real=no_real)
    if decoder and not no_real:
        scene.set_bformat_decoder(*sc.decoder_matrices(LAYOUT))
    if comp is not None:
        scene.set_distance_comp(*comp)
    out = []
    for k, n in enumerate(sizes):
        if events and k in events:
            events[k](scene)
        update(k)
        scene.mix(n, post_process=True)
        out.append(np.array(scene.dry()[:, :n], np.float32))
    _check_kernel(scene, mode)
    scene.close()
    if fx is not None:
        fx.close()
    return out


def _expect(plain, delays, gains, first_line, start=0):
    exp = sc.DistanceCompExpected(delays, gains)
    want = []
    for k, p in enumerate(plain):
        if k < start:
            want.append(p.copy())
            continue
        w = p.copy()
        w[first_line:] = exp.process(p[first_line:], p.shape[1])
        want.append(w)
    return want


def _equal(got, want, tag):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (tag, k, np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_compensated_lines_are_delayed_and_scaled(mode):
    _need()
    sizes = _sizes(24)
    plain = _run(mode, sizes)
    assert min(float(np.abs(np.concatenate([p[ND + i] for p in plain])).max()) for i in range(8)) > 1e-3   # every line carries signal
    got = _run(mode, sizes, comp=(DELAYS, GAINS))
    _equal(got, _expect(plain, DELAYS, GAINS, ND), f"{mode} 7.1")
    # the line with delay 0 and gain 0.5 came through unscaled, the one with delay 1023 starts 1023 samples late
    assert all(np.array_equal(g[ND], p[ND]) for g, p in zip(got, plain))
    assert not got[0][ND + 4, :1023].any() and got[0][ND + 4, 1023] == np.float32(GAINS[4]) * plain[0][ND + 4, 0]


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_fewer_channels_than_lines_and_a_context_without_real_lines(mode):
    _need()
    sizes = _sizes(16)
    plain = _run(mode, sizes)
    got = _run(mode, sizes, comp=(DELAYS[1:4], GAINS[1:4]))          # lines 0-2 only
    _equal(got, _expect(plain, DELAYS[1:4], GAINS[1:4], ND), f"{mode} three channels")
    # no real lines: the dry lines are the output
    plain = _run(mode, sizes, no_real=True)
    assert plain[0].shape[0] == ND and float(np.abs(plain[0]).max()) > 1e-3
    got = _run(mode, sizes, comp=(DELAYS[2:7], GAINS[2:7]), no_real=True)
    _equal(got, _expect(plain, DELAYS[2:7], GAINS[2:7], 0), f"{mode} dry lines")


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_removal_and_reinstall(mode):
    """removed: the uncompensated lines from that update on; re-installed: fresh (zero) history"""
    _need()
    sizes = _sizes(20)
    plain = _run(mode, sizes)
    removed = _run(mode, sizes, comp=(DELAYS, GAINS), events={7: lambda s: s.set_distance_comp(None)})
    for k in range(7, len(sizes)):
        assert np.array_equal(removed[k].view(np.uint32), plain[k].view(np.uint32)), k
    assert not np.array_equal(removed[3], plain[3])
    again = _run(mode, sizes, comp=(DELAYS, GAINS),
                 events={5: lambda s: s.set_distance_comp(None), 9: lambda s: s.set_distance_comp(DELAYS[::-1], GAINS[::-1])})
    _equal(again[9:], _expect(plain, DELAYS[::-1], GAINS[::-1], ND, start=9)[9:], f"{mode} re-installed")
    _equal(again[:5], _expect(plain, DELAYS, GAINS, ND)[:5], f"{mode} before removal")


def test_refused_arguments(synth_mhr):
    import oalgpu
    _need()
    api = _api("fast")
    api.hrtf_load(synth_mhr)
    h = api.make_scene(num_dry=4, num_real=2, wet_channels=4, hrtf=True, max_voices=4)
    with pytest.raises(oalgpu.OalgpuError):
        h.set_distance_comp([1, 2], [1.0, 1.0])
    h.set_distance_comp(None)                           # (removing what is not there is no error)
    h.close()
    sizes = _sizes(12)
    plain = _run("fast", sizes)

    def refusals(s):
        with pytest.raises(oalgpu.OalgpuError):
            s.set_distance_comp([1] * 9, [1.0] * 9)     # more channels than real lines
        with pytest.raises(oalgpu.OalgpuError):
            s.set_distance_comp([0, 1024], [1.0, 1.0])  # DistanceComp::MaxDelay - 1 = 1023

    got = _run("fast", sizes, comp=(DELAYS, GAINS), events={4: refusals})
    _equal(got, _expect(plain, DELAYS, GAINS, ND), "after refusals")


PCM_DELAYS = (300, 17, 5, 0, 1023, 64, 1, 0)
PCM_GAINS = (0.93, 1.25, 0.8, 0.5, 0.71, 0.66, 1.0, 1.0)


@pytest.mark.parametrize("depth", [0.0, 32768.0], ids=["no dither", "dither"])
def test_compensated_pcm_matches_the_reference_output_stage(depth):
    """oalgpu_read_output in s16: the reference's ApplyDither + Write<short> (its bridge renders a stereo device's RealOut)
    on the expected FrontLeft / FrontRight lines"""
    import oalgpu
    _need()
    if not bl.available():
        pytest.skip("needs the reference bridge")
    sizes = _sizes(16)
    plain = _run("fast", sizes)
    want = _expect(plain, PCM_DELAYS, PCM_GAINS, ND)
    bridge = bl.Bridge(bl.MODE_CPU)
    bl.build_config1(bridge, nsources=1)
    scene, fx, update = sc.build_scene(_api("fast"), LAYOUT, dedicated=True)
    scene.set_bformat_decoder(*sc.decoder_matrices(LAYOUT))
    scene.set_distance_comp(PCM_DELAYS, PCM_GAINS)
    for k, n in enumerate(sizes):
        update(k)
        scene.mix(n, post_process=True)
        lines = np.zeros((2, 1024), np.float32)
        lines[:, :n] = want[k][ND:ND + 2]
        ref, _ = bridge.render_lines(lines, oalgpu.OUT_I16, depth, 22222 + k, n, 2)
        scene.set_output(oalgpu.OUT_I16, depth, 22222 + k)
        got = scene.read_output(n, 2)
        assert np.array_equal(got, ref), (k, int(np.argmax(got != ref)))
    assert np.abs(ref.astype(np.int32)).max() > 100
    _check_kernel(scene, "fast")
    scene.close(); fx.close(); bridge.close()


def test_async_read_out_sees_the_compensated_lines():
    _need()
    sizes = _sizes(12)
    plain = _run("fast", sizes)
    want = _expect(plain, DELAYS, GAINS, ND)
    scene, fx, update = sc.build_scene(_api("fast"), LAYOUT, dedicated=True)
    scene.set_bformat_decoder(*sc.decoder_matrices(LAYOUT))
    scene.set_distance_comp(DELAYS, GAINS)
    for k, n in enumerate(sizes):
        update(k)
        scene.mix(n, post_process=True)
        got = scene.output_wait(scene.read_output_async())
        assert np.array_equal(got[:, :n].view(np.uint32), want[k][ND:].view(np.uint32)), k
    _check_kernel(scene, "fast")
    scene.close(); fx.close()


@pytest.mark.parametrize("depth", [0.0, 32768.0], ids=["no dither", "dither"])
def test_the_whole_output_stage(depth):
    """everything on, expected value built in the reference's order: stabilized decode -> Compressor -> distance compensation
    -> dither -> Write<short>.  An EXACT context, so that the limiter's input is the reference composition bit for bit; the
    limiter is bounded, not bit-exact (1e-5 of the line maximum = 0.33 LSB of s16 at full scale), so the float lines are held
    to that bound and the PCM to one LSB."""
    import oalgpu
    _need()
    if not (bl.available() and lc.available()):
        pytest.skip("needs the compiled reference and its bridge")
    nr = sc.LAYOUTS[LAYOUT]["num_real"]
    sizes = _sizes(16)
    params = lc.limiter_params(48000, "no automation")
    # the plain run: no decoder (the reference composition decodes)
    scene, fx, update = sc.build_scene(_api("exact"), LAYOUT, dedicated=True, level=6.0)
    plain = []
    for k, n in enumerate(sizes):
        update(k)
        scene.mix(n, post_process=True)
        plain.append(np.array(scene.dry()[:, :n], np.float32))
    scene.close(); fx.close()
    stabilized = _reference(LAYOUT, plain)
    assert float(max(np.abs(w).max() for w in stabilized)) > 0.5       # above the limiter's threshold
    comp = lc.RefCompressor(params, nr)
    limited = [comp.process(w, w.shape[1]) for w in stabilized]
    comp.close()
    exp = sc.DistanceCompExpected(PCM_DELAYS, PCM_GAINS)
    want = [exp.process(w, w.shape[1]) for w in limited]
    top = np.max([np.abs(w).max(axis=1) for w in want], axis=0)
    bridge = bl.Bridge(bl.MODE_CPU)
    bl.build_config1(bridge, nsources=1)
    scene, fx, update = sc.build_scene(_api("exact"), LAYOUT, dedicated=True, level=6.0)
    scene.set_bformat_decoder(*sc.decoder_matrices(LAYOUT))
    _install(scene, LAYOUT, XOVER)
    scene.set_output_limiter(params)
    scene.set_distance_comp(PCM_DELAYS, PCM_GAINS)
    worst = 0
    for k, n in enumerate(sizes):
        update(k)
        scene.mix(n, post_process=True)
        got = scene.dry()[ND:, :n]
        err = np.abs(got.astype(np.float64) - want[k]).max(axis=1)
        assert np.all(err <= 1e-5 * top + 1e-30), (k, err, top)
        lines = np.zeros((2, 1024), np.float32)
        lines[:, :n] = want[k][:2]
        ref, _ = bridge.render_lines(lines, oalgpu.OUT_I16, depth, 777 + k, n, 2)
        scene.set_output(oalgpu.OUT_I16, depth, 777 + k)
        pcm = scene.read_output(n, 2)
        worst = max(worst, int(np.abs(pcm.astype(np.int32) - ref.astype(np.int32)).max()))
    print(f"whole output stage, depth {depth}: worst PCM difference {worst} LSB")
    assert worst <= 1
    assert np.abs(ref.astype(np.int32)).max() > 1000
    _check_kernel(scene, "exact")
    scene.close(); fx.close(); bridge.close()
