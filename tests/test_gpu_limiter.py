"""The output limiter (oalgpu_set_output_limiter) against the compiled reference's own Compressor (core/mastering.cpp).

Two contexts run the same loud scene, one with the limiter and one without; every update's unlimited output lines go through
the reference Compressor, and the limited context's lines must match it.  The only difference under test is the limiter.
Scenes peak several times above full scale, with silent gaps and clicks shorter than the hold; updates are ragged (1024, 17,
47, 48, 49, 1000, 1024: across the n < lookAhead branch of the delay).  The kernel's logf / expf are correctly rounded where
glibc's are not everywhere, so the bound is 1e-5 x the run's maximum per line, not bit equality.

Contexts: FAST HRTF pipelined, read through oalgpu_read_output_async (the copy path that replaces the ring); HRTF on the
resident voice kernel; 7.1 speaker feeds from the B-Format decoder; a context without real output lines (its dry lines are
RealOut).  The PCM of oalgpu_read_output (s16, with and without dither) is compared with the reference's output stage on the
reference-limited lines."""
import os
import sys

import numpy as np
import pytest

import bridge_lib as bl
import limiter_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1024, 17, 47, 48, 49, 1000, 1024)
pytestmark = pytest.mark.gpu


def _need():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    if not lc.available():
        pytest.skip("needs the compiled reference")


def _sizes(updates):
    return [SIZES[k % len(SIZES)] for k in range(updates)]


KINDS = {
    # name: (bench config, voices, voices per workgroup, real lines, context flags, read path)
    "hrtf ring": (3, 8, 0, 2, 0, "async"),
    "hrtf resident": (3, 4096, 0, 2, "resident", "async"),      # (the machine-filling scene: the 16-wavefront kernel, resident)
    "7.1 decoder": (2, 8, 0, 8, 0, "dry"),
    "no real lines": (2, 8, 0, 0, 0, "dry"),
}


def _scene(kind, scale):
    import oalgpu
    import bench
    cfg, V, vpg, nreal, flags, _ = KINDS[kind]
    api = oalgpu.Api(oalgpu.MATH_FAST, ctx_flags=oalgpu.CTX_RESIDENT if flags == "resident" else 0)
    synth = lc.LoudSynth(scale)
    api._mhr = synth.synth_mhr_bytes()
    sc, script = bench.build_scene(oalgpu, synth, api, cfg, V, 0, api._mhr, vpg, num_real=nreal if cfg == 2 else None)
    if cfg == 2 and nreal == 8:
        hf, lf = synth.x71_decoder()
        sc.set_bformat_decoder(hf, lf)
    allv = list(range(V))
    sc.set_params_batch(allv, bench.param_array(oalgpu, script, allv, 0))
    if flags == "resident":
        sc.resident_set_short_run(0)
    return sc


def _run(kind, scale, sizes, params=None, clear_after=None):
    """Every update's output lines (list of nlines x n arrays) of a fresh scene, limited by `params` (None: no limiter)."""
    sc = _scene(kind, scale)
    if params is not None:
        sc.set_output_limiter(params)
    read = KINDS[kind][5]
    out, tickets = [], []
    for k, n in enumerate(sizes):
        if clear_after is not None and k == clear_after:
            sc.set_output_limiter(None)
        sc.mix(n, post_process=True)
        if read == "async":
            tickets.append((sc.read_output_async(), n))
            if len(tickets) == 3:
                t, m = tickets.pop(0)
                out.append(sc.output_wait(t).reshape(2, 1024)[:, :m].copy())
        else:
            d = sc.dry()
            nreal = KINDS[kind][3]
            lines = d[-nreal:] if nreal else d
            out.append(np.array(lines[:, :n], np.float32))
    for t, m in tickets:
        out.append(sc.output_wait(t).reshape(2, 1024)[:, :m].copy())
    info = sc.resident_stats() if KINDS[kind][4] == "resident" else None
    sc.close()
    return out, info


_SCALE = {}


def _scale(kind):
    """Buffer scale that puts the unlimited scene's peak near 6x full scale (mixing is linear in the buffers)."""
    if kind not in _SCALE:
        lines, _ = _run(kind, 1.0, [1024] * 6)
        peak = max(float(np.abs(x).max()) for x in lines)
        assert peak > 0.0
        _SCALE[kind] = 6.0 / peak
    return _SCALE[kind]


def _check(kind, rate, pset, updates):
    import oalgpu
    _need()
    scale = _scale(kind)
    sizes = _sizes(updates)
    params = lc.limiter_params(rate, pset)
    plain, _ = _run(kind, scale, sizes)
    got, info = _run(kind, scale, sizes, params)
    if info is not None:
        assert info["enabled"] == 1 and info["failed"] == 0 and info["updates"] == updates, info
    nlines = plain[0].shape[0]
    ref = lc.RefCompressor(params, nlines)
    want = [ref.process(x, x.shape[1]) for x in plain]
    ref.close()
    peak_in = max(float(np.abs(x).max()) for x in plain)
    assert 3.0 < peak_in < 12.0, peak_in                        # the scene drives the limiter hard
    top = np.max([np.abs(w).max(axis=1) for w in want], axis=0)    # per line
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want)):
        err = np.abs(g.astype(np.float64) - w).max(axis=1)
        rel = err / np.maximum(top, 1e-30)
        worst = max(worst, float(rel.max()))
        assert np.all(err <= 1e-5 * top + 1e-30), (kind, rate, pset, k, sizes[k], err, top)
    print(f"{kind} {rate} Hz {pset}: {updates} updates, peak in {peak_in:.2f}, out {float(top.max()):.3f}, "
          f"worst |err| / line max {worst:.2e}")
    return worst


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("rate", [44100, 48000, 96000])
def test_device_limiter_matches_the_reference(kind, rate):
    _check(kind, rate, "device default", 42)


@pytest.mark.parametrize("pset", [p for p in lc.PARAM_SETS if p != "device default"])
@pytest.mark.parametrize("kind", ["hrtf ring", "7.1 decoder"])
def test_limiter_parameter_sets_match_the_reference(kind, pset):
    _check(kind, 48000, pset, 42)


def test_long_run_covers_the_adaptation():
    """several hundred updates: the 2 s adaptation of the gain deviation (a_adp) settles"""
    _check("hrtf ring", 48000, "device default", 320)


def test_limited_pcm_matches_the_reference_output_stage():
    """oalgpu_read_output in s16, with and without dither: ApplyDither + Write<T> of the reference (its bridge renders a stereo
    device's RealOut) on the reference-limited lines."""
    import oalgpu
    _need()
    if not bl.available():
        pytest.skip("needs the reference bridge")
    kind = "hrtf ring"
    scale = _scale(kind)
    sizes = _sizes(42)
    plain, _ = _run(kind, scale, sizes)
    bridge = bl.Bridge(bl.MODE_CPU)
    bl.build_config1(bridge, nsources=1)
    total = off = 0
    for depth in (0.0, 32768.0):
        params = lc.limiter_params(48000, "device default", oalgpu.OUT_I16, depth)
        ref = lc.RefCompressor(params, 2)
        sc = _scene(kind, scale)
        sc.set_output_limiter(params)
        for k, n in enumerate(sizes):
            sc.mix(n, post_process=True)
            want_lines = np.zeros((2, 1024), np.float32)
            want_lines[:, :n] = ref.process(plain[k], n)
            seed = 22222 + k
            want, _ = bridge.render_lines(want_lines, oalgpu.OUT_I16, depth, seed, n, 2)
            sc.set_output(oalgpu.OUT_I16, depth, seed)
            got = sc.read_output(n, 2)
            d = np.abs(got.astype(np.int32) - want.astype(np.int32))
            assert d.max() <= 1, (depth, k, int(d.max()))
            total += d.size
            off += int(np.count_nonzero(d))
        ref.close()
        sc.close()
    bridge.close()
    print(f"PCM: {off} of {total} samples 1 LSB off")
    assert off <= 0.001 * total, (off, total)


def test_limiter_off_means_unchanged():
    """a limiter set and then removed leaves no trace: bit-identical output to a context that never had one (the HRTF context
    goes back to its output ring)"""
    _need()
    kind = "hrtf ring"
    scale = _scale(kind)
    sizes = _sizes(14)
    params = lc.limiter_params(48000, "device default")
    never, _ = _run(kind, scale, sizes)
    cleared_at_once, _ = _run(kind, scale, sizes, params, clear_after=0)
    cleared_later, _ = _run(kind, scale, sizes, params, clear_after=6)
    for k in range(len(sizes)):
        assert np.array_equal(cleared_at_once[k].view(np.uint32), never[k].view(np.uint32)), k
        if k >= 6:
            assert np.array_equal(cleared_later[k].view(np.uint32), never[k].view(np.uint32)), k
    for kind in ("7.1 decoder", "no real lines"):
        a, _ = _run(kind, _scale(kind), sizes[:6])
        b, _ = _run(kind, _scale(kind), sizes[:6], params, clear_after=0)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), kind


def test_bad_limiter_arguments_are_refused():
    import oalgpu
    _need()
    sc = _scene("7.1 decoder", 1.0)
    p = lc.limiter_params(48000, "device default")
    p.num_channels = 3                                   # the context has 8 output lines
    with pytest.raises(oalgpu.OalgpuError):
        sc.set_output_limiter(p)
    p.num_channels = 8
    sc.set_output_limiter(p)
    p.sample_rate = float("nan")
    with pytest.raises(oalgpu.OalgpuError):
        sc.set_output_limiter(p)
    sc.set_output_limiter(None)
    sc.close()
