"""Several contexts on one device (oalgpu_context_attach: ProcessContexts, alc/alu.cpp:2177-2273): the scenes of
tests/test_gpu_attach.py and the reference they are held to.

The reference mixes every context of a device into the device's ONE MixBuffer.  Buses are sums, and
oracle_lib.Scene.dry_view() is writable between the voice loop and the post-process, so the reference of a device context
with attached contexts is composed of one reference scene per context:

  1. the device scene mixes with post_process=False;
  2. every attached context's scene (non-HRTF, the same line counts as the product's) mixes, and its effect slots run;
  3. their lines are added into the device scene's dry_view() rows through the map, in attach order, in float32
     (compose): (own value) + attached 0 + attached 1 + ..., one add per contributor and sample, as BusMergeKernel adds;
  4. the device scene post-processes (HRTF), or the comparison runs on the decoded dry block (speaker devices).

Every builder takes `lib`: the reference (oracle_lib.OracleLib) or the product (oalgpu.Api) -- the scene interface is the same."""
import os

import numpy as np

import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_MHR = os.path.join(ROOT, "tests", "golden", "default_hrtf.mhr")
XOVER = 400.0 / 48000.0
HF_SCALES = (1.26, 0.91, 0.91, 0.91)        # a first-order source's HF scales per channel (the same on both sides is all that matters)
CHILD_MAP = [0, 1, 2, 3, 4, 5]              # the attached 6-line context: lines 0-3 -> Dry (B-Format), 4-5 -> RealOut L/R


def reference():
    """the compiled reference (one Voice with several ChannelData for B-Format and stereo sources), or None"""
    if not ol.available("ref"):
        return None
    L = ol.load("ref")
    L.L.oal_set_simd(1)
    return L


def int_state(st):
    return (st.play_state, st.position, st.position_frac, st.has_buffer, st.fading)


def compose(dev_lines, attached, n):
    """step 3: attached = [(lines [k, 1024], map)] in attach order; adds frames [0, n) into dev_lines (a dry_view()) in place"""
    for lines, line_map in attached:
        for i, d in enumerate(line_map):
            if d >= 0:
                dev_lines[d, :n] = dev_lines[d, :n] + np.asarray(lines[i, :n], np.float32)


# ---- the HRTF device: 4 dry + 2 real lines, an explicit direct-HRTF decoder, HRTF voices ---------------------------------
def hrtf_params(v, k):
    r = np.random.default_rng(1000 * v + k)
    return ol.make_voice_params(60211 if v % 3 else 52000, ol.RS_BSINC24,
                                hrtf=(np.arcsin(r.uniform(-1, 1)), r.uniform(-np.pi, np.pi), 2.0, 0.0, 10 ** (r.uniform(-30, -10) / 20)),
                                direct_filter=ol.default_filter(active=v % 4 == 1, gain_hf=0.5 if k < 1 else 0.3))


def build_hrtf_device(lib, nvoices, irsize, **kw):
    """`lib` has the data set loaded (hrtf_load)"""
    rng = np.random.default_rng(41)
    cc = np.zeros((4, 128, 2), np.float32)
    cc[:, :irsize] = rng.uniform(-0.2, 0.2, (4, irsize, 2))
    data = rng.uniform(-1, 1, 8000).astype(np.float32)
    sc = lib.make_scene(num_dry=4, num_real=2, hrtf=True, **kw)
    sc.set_direct_hrtf(cc, [1.0, 0.8, 0.8, 0.8], XOVER, irsize)
    b = sc.add_buffer(data, ol.FMT_FLOAT, loop_start=0, loop_end=8000)
    for v in range(nvoices):
        sc.add_voice(b, looping=True, position=(v * 911) % 7000, frac=(v * 977) % 65536)
        sc.set_params(v, hrtf_params(v, 0))
    return sc


# ---- the attached lines context of an HRTF device: a B-Format source into Dry, a direct-channel stereo source into RealOut ----
def child_params(src, c, k):
    """source 0: first-order B-Format, channel c on line c (an unrotated source on a first-order device); source 1: stereo,
    channel c on line 4 + c (AL_DIRECT_CHANNELS_SOFT: RealOut L/R).  ONE audible channel per line: the sum over the channel
    voices has one non-zero term per line, so an EXACT context's lines are the reference's bits
    (tests/test_ambi_voices.py::test_gpu_one_channel_exact_mode_is_bit_exact).  Everything voice-wide (step, resampler,
    filter) depends on the source and the update only."""
    r = np.random.default_rng(100 * src + 10 * c + k)
    g = np.zeros(6, np.float32)
    g[c if src == 0 else 4 + c] = r.uniform(0.2, 0.6) * (-1.0 if (c + k) % 3 == 0 else 1.0)
    filt = ol.default_filter(active=1 if src == 0 else k % 2, gain_hf=0.5 if k < 1 else 0.25, gain_lf=0.8 if k < 1 else 0.6)
    return ol.make_voice_params([60211, 48000][src], ol.RS_BSINC24, dry_gains=g, direct_filter=filt)


def build_child(lib, **kw):
    """-> (scene, B-Format voice, stereo voice): what add_ambi_voice returned (the product: the first of the channel voices)"""
    rng = np.random.default_rng(17)
    sc = lib.make_scene(num_dry=6, num_real=0, hrtf=False, **kw)
    bfmt = sc.add_buffer(rng.uniform(-1, 1, 4 * 7000).astype(np.float32), ol.FMT_FLOAT, frame_step=4, loop_start=50, loop_end=6900)
    stereo = sc.add_buffer(rng.uniform(-1, 1, 2 * 6000).astype(np.float32), ol.FMT_FLOAT, frame_step=2, loop_start=0, loop_end=6000)
    a = sc.add_ambi_voice(bfmt, 4, looping=True, position=977, frac=12345)
    s = sc.add_ambi_voice(stereo, 2, looping=True, position=301, frac=40000)
    for c in range(4):
        sc.set_channel_ambi_scale(a, c, XOVER, HF_SCALES[c], 1.0)
    child_update(sc, a, s, 0)
    return sc, a, s


def child_update(sc, a, s, k):
    for c in range(4):
        sc.set_channel_params(a, c, child_params(0, c, k))
    for c in range(2):
        sc.set_channel_params(s, c, child_params(1, c, k))


# ---- plain lines scenes: a speaker device (4 dry + 2 real) and the contexts attached to it (4 dry) ----------------------
DEDICATED_GAINS = (0.7, -0.45, 0.0, 0.0)     # the dedicated effect of attached context B: wet channel 0 into B's lines 0-1


def build_lines(lib, nvoices, seed, num_real=0, send=False, line3_scale=1.0, **kw):
    rng = np.random.default_rng(seed)
    sc = lib.make_scene(num_dry=4, num_real=num_real, num_sends=1 if send else 0, num_slots=1 if send else 0, wet_channels=4,
                        hrtf=False, **kw)
    buf = sc.add_buffer(rng.uniform(-1, 1, 9000).astype(np.float32), ol.FMT_FLOAT, loop_start=0, loop_end=9000)
    for v in range(nvoices):
        sc.add_voice(buf, looping=True, position=(v * 701 + seed * 131) % 8000, frac=(v * 4099) % 65536)
        g = rng.uniform(0.05, 0.3, 4)
        g[3] *= line3_scale
        snd = [(0, rng.uniform(0.1, 0.4, 4), None)] if send else []
        sc.set_params(v, ol.make_voice_params([60211, 48000, 71000][v % 3], ol.RS_BSINC24, dry_gains=g,
                                              direct_filter=ol.default_filter(active=v % 2, gain_hf=0.4), sends=snd))
    return sc


class ReferenceDedicated:
    """DedicatedState::process (alc/effects/dedicated.cpp): MixSamples of wet channel 0 with the target gains, the current
    gains ramping over the update -- the reference's own Mix through the per-call entry point"""

    def __init__(self, L, gains):
        self.L = L
        self.cur = np.zeros(len(gains), np.float32)
        self.tgt = np.asarray(gains, np.float32)

    def process(self, wet0, lines, n):
        out = np.ascontiguousarray(lines[:len(self.tgt)])
        self.L.mix(np.ascontiguousarray(wet0[:n]), out, self.cur, self.tgt, n, 0)
        lines[:len(self.tgt)] = out
