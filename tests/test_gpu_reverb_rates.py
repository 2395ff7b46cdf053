"""The EAX reverb kernel at device rates other than 48 kHz (8000 .. 44100 Hz), through the C-ABI against the compiled
reference at the same rate.

Every delay, tap, window and sub-block length of the reverb is seconds x rate.  What a low rate changes in the kernel:
late sub-blocks of min(mLate.Offset[0], 256, left) samples become shorter than the early wave's 256 (density 0: 77 at
8000 Hz, 106 at 11025, 154 at 16000, 213 at 22050), so the two waves of a pipeline stop running in step and, during a
density cross-fade, the old and the new pipeline's late waves run different sub-block counts side by side; the LDS-window
all-passes advance in chunks of 3 (early) and 6 (late) samples at 8000 Hz; hf_reference / rate meets its 0.49 cap; every
line stride and mask is another power of two.  tests/reverb_cases.py holds the schedules and what each must prove from
the reference's parameter block."""
import numpy as np
import pytest

import oracle_lib as ol
from reverb_cases import (CASES, RATE_MATRIX, RATE_IDS, BUFFER_LINE, LATE_BLOCK, rate_seed, wet_input, out_init,
                          check_reach, check_longest_delays)
from test_reverb import UPMIX_CASES, as_oracle_params, bits, block_bytes

pytestmark = pytest.mark.gpu


def _gpu():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    return oalgpu


class _Oracle:
    """The compiled reference where it travelled with the tree, else the restatement fed the product's host blocks."""

    def __init__(self, oalgpu, nlines, rate):
        self.oalgpu, self.rate = oalgpu, rate
        self.is_ref = ol.available("ref")
        if self.is_ref:
            self.lib = ol.load("ref")
            self.orc, self.host = self.lib.make_reverb(nlines, rate), None
        else:
            self.orc, self.host = ol.load("port").make_reverb(nlines, rate), oalgpu.Reverb(nlines, rate, device=-1)
        self.k = 0

    def update(self, name, st):
        """-> the oracle's parameter block after this update(); with the reference, the case proves its reach"""
        if self.is_ref:
            before = self.orc.get_params().pipeline_state
            self.orc.update(ol.ReverbProps.make(**st["props"]), st["slot_gain"])
            blk = self.orc.get_params()
            check_reach(self.lib, ol.ReverbProps, name, self.rate, self.k, st, blk, before)
        else:
            self.host.update(self.oalgpu.ReverbProps.make(**st["props"]), st["slot_gain"])
            blk = as_oracle_params(block_bytes(self.host.get_params()))
            self.orc.set_params(blk)
        self.k += 1
        return blk

    def process_n(self, x, out, n):
        self.orc.process_n(x, out, n)
        if self.host is not None:
            self.host.skip(n)

    def close(self):
        self.orc.close()
        if self.host is not None:
            self.host.close()


def _run(name, schedule, rate, drive, fast=False):
    """drive 'update': the product's own update() (end to end); 'params': the oracle's block installed with set_params
    (the kernel alone).  -> [(gpu, oracle)] per update."""
    oalgpu = _gpu()
    g = oalgpu.Reverb(4, rate)
    if fast:
        g.set_math_mode(oalgpu.MATH_FAST)
    orc = _Oracle(oalgpu, 4, rate)
    x = wet_input(rate_seed(name, rate) + (1 if drive == "params" else 0), len(schedule))
    outs = []
    for u, st in enumerate(schedule):
        if st["props"] is not None:
            blk = orc.update(name, st)
            if drive == "params":
                g.set_params(blk)
            else:
                g.update(oalgpu.ReverbProps.make(**st["props"]), st["slot_gain"])
        a, b = out_init(4), out_init(4)
        g.process_n(x[u], a, st["n"])
        orc.process_n(x[u], b, st["n"])
        if not fast:
            assert np.array_equal(bits(a), bits(b)), (name, rate, drive, u, int(np.flatnonzero((bits(a) != bits(b)).any(0))[0]),
                                                      float(np.abs(a - b).max()))
        outs.append((a, b))
    assert sum(float(np.abs(b[:, 7:]).sum()) for _, b in outs) > 1.0, (name, rate)
    if orc.is_ref:
        check_longest_delays(name, rate, schedule, [b for _, b in outs], orc.orc.get_params())
    g.close(); orc.close()
    return outs


@pytest.mark.parametrize("name,schedule,rate", RATE_MATRIX, ids=RATE_IDS)
def test_gpu_exact_end_to_end_at_rate(name, schedule, rate):
    """EXACT mode, the product's own update() + the HIP process(): bit for bit with ReverbState::process, every update."""
    _run(name, schedule, rate, "update")


@pytest.mark.parametrize("name,schedule,rate", RATE_MATRIX, ids=RATE_IDS)
def test_gpu_exact_kernel_alone_at_rate(name, schedule, rate):
    """EXACT mode, the HIP process() fed the reference's parameter block: bit for bit, every update."""
    _run(name, schedule, rate, "params")


_fast_worst = {}


@pytest.mark.parametrize("name,schedule,rate", RATE_MATRIX, ids=RATE_IDS)
def test_gpu_fast_mode_at_rate(name, schedule, rate):
    """OALGPU_MATH_FAST (master band-pass and T60 filters as block scans) over the same matrix: every update within
    2e-5 of the run's maximum + 1e-7, the bound of test_gpu_fast_mode_matches_oracle, unchanged.  The worst ratio seen so
    far at each rate is printed (measured on an MI355X: 3.3e-6 at 8000 Hz, 2.6e-6 at 11025, 4.6e-6 at 16000, 5.5e-6 at
    22050, 4.5e-6 at 32000, 6.6e-6 at 44100)."""
    outs = _run(name, schedule, rate, "params", fast=True)
    scale = max(float(np.abs(b).max()) for _, b in outs)
    worst = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in outs)
    _fast_worst[rate] = max(_fast_worst.get(rate, 0.0), worst / scale)
    print(f"FAST reverb {name} at {rate} Hz: worst {worst:.3e} = {worst / scale:.2e} of the run's maximum {scale:.3e}; "
          f"worst ratio at this rate so far {_fast_worst[rate]:.2e}")
    assert scale > 1e-4, (name, rate, scale)
    assert worst <= 2e-5 * scale + 1e-7, (name, rate, worst, scale)


@pytest.mark.parametrize("rate", (44100, 22050))
def test_gpu_long_run_at_rate(rate):
    """The 60-update schedule of test_gpu_wide_target_and_long_run (16 target lines, modulated, panned, two parameter
    changes) at 44100 Hz, and at 22050 Hz with density 0 (213-sample late sub-blocks): bit for bit, every update."""
    oalgpu = _gpu()
    if not ol.available("ref"):
        pytest.skip("needs the compiled reference for a 16-line target")
    nlines = 16
    orc = ol.load("ref").make_reverb(nlines, rate)
    g = oalgpu.Reverb(nlines, rate)
    rng = np.random.default_rng(99)
    changes = {0: dict(modulation_depth=1.0, modulation_time=0.3, decay_time=4.0, late_reverb_pan=(0.2, 0.3, -0.5)),
               20: dict(modulation_depth=0.4, modulation_time=1.3, decay_time=2.0, density=0.3),
               41: dict(modulation_depth=0.4, modulation_time=1.3, decay_time=2.0, density=0.3, gain=0.1)}
    if rate == 22050:
        changes = {u: dict(kw, density=0.0) for u, kw in changes.items()}
    for u in range(60):
        if u in changes:
            orc.update(ol.ReverbProps.make(**changes[u]), 0.9)
            g.update(oalgpu.ReverbProps.make(**changes[u]), 0.9)
            blk = orc.get_params()
            short = blk.pipe[blk.current_pipeline].late_offset[0] < LATE_BLOCK
            assert short == (rate == 22050), (rate, u, blk.pipe[blk.current_pipeline].late_offset[0])
        x = (rng.standard_normal((4, BUFFER_LINE)) * 0.1).astype(np.float32)
        a, b = out_init(nlines), out_init(nlines)
        g.process(x, a)
        orc.process(x, b)
        assert np.array_equal(bits(a), bits(b)), (rate, u, float(np.abs(a - b).max()))
        assert np.array_equal(a[4:], out_init(nlines)[4:])
    assert float(np.abs(b[:4, 7:]).max()) > 1e-3
    g.close(); orc.close()


@pytest.mark.parametrize("rate", (44100, 22050))
@pytest.mark.parametrize("name,order,horizontal", UPMIX_CASES, ids=[f"{c[0]}_order{c[1]}" for c in UPMIX_CASES])
def test_gpu_upmix_at_rate(name, order, horizontal, rate):
    """MixOutAmbiUp with the band splitter designed for the device's rate (400 Hz / rate): bit for bit, every update."""
    oalgpu = _gpu()
    if not ol.available("ref"):
        pytest.skip("needs the compiled reference")
    ref = ol.load("ref")
    nlines = (order + 1) ** 2
    schedule = dict(CASES)[name]
    orc = ref.make_reverb(nlines, rate, device_order=order)
    g = oalgpu.Reverb(nlines, rate)
    sc, up, xo = ref.ambi_upmix_info(order, horizontal, rate)
    assert abs(xo * rate - ref.ambi_upmix_info(order, horizontal, 48000)[2] * 48000) < 1e-2, "the splitter follows the rate"
    g.set_upmix(sc, up, xo)
    x = wet_input(rate_seed(name, rate) + 5, len(schedule))
    for u, st in enumerate(schedule):
        if st["props"] is not None:
            orc.update(ol.ReverbProps.make(**st["props"]), st["slot_gain"])
            g.update(oalgpu.ReverbProps.make(**st["props"]), st["slot_gain"])
        a, b = out_init(nlines), out_init(nlines)
        g.process_n(x[u], a, st["n"])
        orc.process_n(x[u], b, st["n"])
        assert np.array_equal(bits(a), bits(b)), (name, rate, u, float(np.abs(a - b).max()))
    if name == "panned":
        assert np.abs(b[4:, 7:]).max() > 0.0, "higher-order lines are fed"
    g.close(); orc.close()


def test_gpu_four_reverb_slots_at_22050(synth_mhr):
    """The scene of test_gpu_four_reverb_slots_in_scene with its four reverbs created at 22050 Hz and densities 0, 0.01,
    0.2 and 1.0: late sub-blocks of 213 and of 256 samples inside one batched launch, mixing out in ticket order.
    Expected = the oracle scene's wet buses through four reference ReverbStates at 22050 Hz; the bound is that test's
    (2e-5 x max + 1e-7: the reverb inputs already differ in the last bit)."""
    oalgpu = _gpu()
    if not ol.available("ref"):
        pytest.skip("needs the compiled reference")
    L = ol.load("ref")
    L.L.oal_set_simd(1)
    api = oalgpu.Api(oalgpu.MATH_FAST)
    nlines, rate = 5, 22050

    def build(lib):
        sc = lib.make_scene(num_dry=nlines, num_real=0, num_sends=4, num_slots=4, wet_channels=4, hrtf=False)
        r = np.random.default_rng(11)
        buf = sc.add_buffer(r.uniform(-1, 1, 9000).astype(np.float32), ol.FMT_FLOAT, loop_start=0, loop_end=9000)
        for v in range(24):
            sc.add_voice(buf, looping=True, position=(v * 977) % 8000, frac=0)
            snd = [(i, r.uniform(0.05, 0.3, 4), ol.default_filter(active=1 if (v + i) % 3 == 0 else 0, gain_hf=0.6))
                   for i in range(v % 5)]
            sc.set_params(v, ol.make_voice_params(60211, ol.RS_BSINC24, dry_gains=r.uniform(0, 0.1, nlines),
                                                  direct_filter=ol.default_filter(active=v % 2, gain_hf=0.5), sends=snd))
        return sc

    presets = [dict(density=0.0), dict(density=0.01, decay_time=3.0, modulation_depth=0.4),
               dict(density=0.2, diffusion=0.5), dict(density=1.0, late_reverb_pan=(0.3, 0.0, -0.6), decay_time=0.8)]
    gsc, osc = build(api), build(L)
    grev, orev = [], []
    for slot, kw in enumerate(presets):
        g = oalgpu.Reverb(nlines, rate)
        g.update(oalgpu.ReverbProps.make(**kw), 0.5 + 0.1 * slot)
        gsc.set_slot_reverb(slot, g)
        o = L.make_reverb(nlines, rate)
        o.update(ol.ReverbProps.make(**kw), 0.5 + 0.1 * slot)
        grev.append(g); orev.append(o)
    late0 = [o.get_params().pipe[o.get_params().current_pipeline].late_offset[0] for o in orev]
    assert late0[0] < LATE_BLOCK <= late0[1] < late0[2] < late0[3], late0
    for k in range(6):
        n = (1024, 1024, 700, 1024, 1024, 1024)[k]
        if k == 3:          # a parameter change that cross-fades two of the instances
            for slot in (1, 2):
                kw = dict(density=presets[slot]["density"], decay_time=1.2 + slot)
                grev[slot].update(oalgpu.ReverbProps.make(**kw), 0.6)
                orev[slot].update(ol.ReverbProps.make(**kw), 0.6)
        gsc.mix(n, post_process=True)
        got = gsc.dry()
        osc.mix(n, post_process=False)
        want = osc.dry().copy()
        for slot in range(4):
            orev[slot].process_n(np.ascontiguousarray(osc.wet(slot)[:4]), want, n)
        err = float(np.abs(got[:, :n].astype(np.float64) - want[:, :n]).max())
        assert err <= 2e-5 * float(np.abs(want[:, :n]).max()) + 1e-7, (k, err)
    for slot in range(4):
        gsc.set_slot_reverb(slot, None)
    for x in grev + orev:
        x.close()
    gsc.close(); osc.close()


def test_gpu_creation_limits():
    """On a device the kernel's LDS windows hold rates up to 48 kHz: above, oalgpu_reverb_create refuses with a message
    that says so, and leaves nothing behind -- an instance at 48000 made afterwards works and matches the oracle."""
    oalgpu = _gpu()
    for rate in (48001, 96000):
        with pytest.raises(RuntimeError, match="above 48 kHz"):
            oalgpu.Reverb(4, rate)
    with pytest.raises(RuntimeError):
        oalgpu.Reverb(4, 7999)
    name, schedule = CASES[0]
    _run(name, schedule, 48000, "update")
