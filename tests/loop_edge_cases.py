"""Static voices at the edges of their buffer's loop: short loops, loops that end inside the source window, positions at
and past the loop end, one-shot voices at and past the buffer end, tiny buffers -- LoadBufferStatic's branches
(core/voice.cpp:500-544), the past-the-loop-end rule (:1015-1019) and the position wrap after the update (:1139-1146),
which every voice kernel restates (csrc/wave_common.hpp GatherCovers / GatherStaticT / GatherIsLinear, dev_voice.hpp
FillFromStatic, and the position update of each kernel).

Driven through any object with the oracle_lib.Scene interface.  `scene(step)` builds the case list of one pitch;
`classify` names the branch the kernels' register gather takes for a voice's first chunk, and every case asserts that
it sits on the branch it was placed on.

Buffers carry sentinels: +0.9 in front of the loop start, -0.9 from the loop end on, loop contents in (-0.6, 0.6) (loops
of 1-3 samples: distinct fixed values).  A read past the loop end or a wrap to 0 instead of the loop start is then a
gross error, not rounding."""
from collections import namedtuple

import numpy as np

import oracle_lib as ol

WINDOW = 17 * 64                        # kPre * 64: the elements the register gather loads (csrc/wave_common.hpp)
RESAMPLE_DATA = 1024 + 256 + 48         # DeviceBase::mResampleData (BufferLineSize + 256 + MaxResamplerPadding)
MAX_EDGE = 24                           # MaxResamplerEdge
SRC_MAX = RESAMPLE_DATA - MAX_EDGE
FRAC_ONE = 1 << 16
MAX_PITCH = 10 * FRAC_ONE

SENTINEL_BEFORE, SENTINEL_AFTER = 0.9, -0.9        # (+-0.05 of noise, so that an offset read past the loop end shows)
SHORT_LOOPS = {1: [0.45], 2: [0.3, -0.5], 3: [0.55, -0.2, 0.35]}

BufSpec = namedtuple("BufSpec", "n ls le fmt fs")       # sample_len, loop start, loop end, format, frame step
Voice = namedtuple("Voice", "buf looping pos frac branch name")


def calc_buffer_size(frac, step, dst_remaining):
    """CalculateBufferSize, core/voice.cpp:600-640 (csrc/dev_voice.hpp CalcBufferSize): (dst, src)"""
    ext = 1 if step <= FRAC_ONE else 0
    src = (((dst_remaining - ext) * step + frac) >> 16) + ext + MAX_EDGE
    if src <= SRC_MAX:
        return dst_remaining, src
    dst = (((SRC_MAX - MAX_EDGE) << 16) - frac) // step
    if dst < dst_remaining:
        return dst & ~3, SRC_MAX
    return dst_remaining, SRC_MAX


def classify(buf, looping, pos, frac, step, todo):
    """The loader of a static voice's first chunk in the voice kernels' register gather (voice_wave16.hip:405-430):
    'past-loop-end' (a looping voice at or past a loop end inside the buffer: plays on unlooped), 'copy' (step 1.0 and
    no fraction: the 1:1 copy, never the register path), 'generic' (LoadBufferStatic's loop: a window over WINDOW, a
    format other than f32 / i16, or more than one wrap), 'linear' (GatherLinearT), 'one-wrap' (GatherStaticT looping)
    or 'end-clamp' (GatherStaticT of a one-shot voice: index clamped to the last sample)."""
    if looping and pos >= buf.le:
        if buf.le < buf.n:
            return "past-loop-end"
        looping = False
    if step == FRAC_ONE and frac == 0:
        return "copy"
    bsrc = calc_buffer_size(frac, step, todo)[1]
    if bsrc > WINDOW or buf.fmt not in (ol.FMT_FLOAT, ol.FMT_SHORT):
        return "generic"
    if looping and not (pos < buf.le and bsrc <= (buf.le - pos) + (buf.le - buf.ls)):
        return "generic"
    if buf.fs == 1 and pos + WINDOW <= buf.n and (not looping or pos + bsrc <= buf.le):
        return "linear"
    return "one-wrap" if looping else "end-clamp"


def buffer_data(spec, seed):
    """float32 samples of a buffer (interleaved frames for fs > 1: channel 0 is the one played), sentinels around the loop"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.6, 0.6, spec.n)
    x[np.abs(x) < 0.05] = 0.3
    length = spec.le - spec.ls
    if length in SHORT_LOOPS:
        x[spec.ls:spec.le] = SHORT_LOOPS[length]
    if spec.le < spec.n or spec.ls > 0:         # a one-shot buffer looped whole keeps plain contents
        x[:spec.ls] = SENTINEL_BEFORE + rng.uniform(-0.05, 0.05, spec.ls)
        x[spec.le:] = SENTINEL_AFTER + rng.uniform(-0.05, 0.05, spec.n - spec.le)
    if spec.le == spec.n and spec.ls == 0:
        x[-1] = 0.8                             # the held last sample of a one-shot voice
    if spec.fs > 1:
        frames = np.full((spec.n, spec.fs), 0.7)
        frames[:, 0] = x
        x = frames.ravel()
    return x


def encode(x, fmt):
    if fmt == ol.FMT_FLOAT:
        return x.astype(np.float32)
    if fmt == ol.FMT_SHORT:
        return np.round(x * 32767.0).astype(np.int16)
    assert fmt == ol.FMT_UBYTE
    return np.clip(np.round(x * 127.0 + 128.0), 0, 255).astype(np.uint8)


FMTS = (ol.FMT_FLOAT, ol.FMT_SHORT)


def _loop_lengths(step, todo0, out):
    # loop lengths around MaxResamplerEdge and MaxResamplerPadding, inside a buffer that extends past the loop end:
    # started below the loop start and one before the loop end; loop start 0 for some
    for i, length in enumerate((1, 2, 3, 23, 24, 25, 47, 48, 49, 64, 65)):
        fmt = (ol.FMT_FLOAT, ol.FMT_SHORT, ol.FMT_UBYTE)[i % 3]
        ls = 7
        b = BufSpec(ls + length + 9, ls, ls + length, fmt, 1)
        out.append((b, True, ls - 3, 1000 + 37 * i, f"loop{length}_below_start"))
        out.append((b, True, ls + length - 1, 40000 + i, f"loop{length}_at_end_minus_1"))
        if length in (1, 3, 24, 48, 65):
            b0 = BufSpec(length + 5, 0, length, FMTS[i % 2], 1)
            out.append((b0, True, 0, 5 + i, f"loop{length}_from_0"))


def _boundary(step, todo0, out):
    # bsrc == (le - pos) + (le - ls): the last window GatherCovers accepts; one either side by position and by length
    frac = 12345
    bsrc = calc_buffer_size(frac, step, todo0)[1]
    if bsrc > WINDOW:
        return
    length = (bsrc + 1) // 2 + 5
    d = 2 * length - bsrc                               # pos = ls + d puts the sum exactly at bsrc
    ls = 11
    for fmt in FMTS:
        b = BufSpec(ls + length + 30, ls, ls + length, fmt, 1)
        for dd, tag in ((d - 1, "inside"), (d, "equal"), (d + 1, "outside")):
            out.append((b, True, ls + dd, frac, f"boundary_{tag}_{'f32' if fmt == ol.FMT_FLOAT else 'i16'}"))
        for dl, tag in ((-1, "shorter"), (1, "longer")):
            bl = BufSpec(ls + length + dl + 30, ls, ls + length + dl, fmt, 1)
            out.append((bl, True, ls + d, frac, f"boundary_len_{tag}_{'f32' if fmt == ol.FMT_FLOAT else 'i16'}"))


def _linear_limit(step, todo0, out):
    # pos + WINDOW == sampleLen +-1 with loopEnd < sampleLen (the window's tail reads past the loop end: GatherIsLinear
    # must still hold pos + bsrc <= loopEnd); pos + bsrc == loopEnd +-1
    frac = 777
    bsrc = calc_buffer_size(frac, step, todo0)[1]
    if bsrc > WINDOW:
        return
    n = 3000
    le = n - (WINDOW - bsrc) // 2 - 1
    b = BufSpec(n, 500, le, ol.FMT_FLOAT, 1)
    b2 = BufSpec(2500 + WINDOW, 500, 2500, ol.FMT_FLOAT, 1)
    for dp in (-1, 0, 1):
        out.append((b, True, n - WINDOW + dp, frac, f"linear_limit_len{dp:+d}"))
        out.append((b2, True, b2.le - bsrc + dp, frac, f"linear_limit_loopend{dp:+d}"))
    bo = BufSpec(n, 0, n, ol.FMT_SHORT, 1)
    for dp in (-1, 0, 1):
        out.append((bo, False, n - WINDOW + dp, frac, f"oneshot_linear_limit{dp:+d}"))


def _positions(step, todo0, out):
    # at and past the loop end (plays on unlooped to sampleLen, then stops), the last sample, one-shot past the end
    b = BufSpec(1500, 100, 300, ol.FMT_FLOAT, 1)
    bi = BufSpec(1500, 100, 300, ol.FMT_SHORT, 1)
    for bb, t in ((b, "f32"), (bi, "i16")):
        out.append((bb, True, 300, 4321, f"at_loop_end_{t}"))
        out.append((bb, True, 307, 0 if t == "i16" else 99, f"past_loop_end_{t}"))
        out.append((bb, True, 299, 4321, f"loop_end_minus_1_{t}"))
        out.append((bb, True, 1499, 50000, f"last_sample_looping_{t}"))
        out.append((bb, False, 1499, 50000, f"last_sample_oneshot_{t}"))
        out.append((bb, False, 1500, 3, f"oneshot_at_len_{t}"))
        out.append((bb, False, 1507, 3, f"oneshot_past_len_{t}"))
        out.append((bb, False, 1500 - 700, 3, f"oneshot_ends_inside_{t}"))
    bw = BufSpec(600, 0, 600, ol.FMT_FLOAT, 1)          # loop end == sample length: at the end the loop still wraps
    out.append((bw, True, 599, 65535, "whole_loop_last_sample"))


def _tiny(step, todo0, out):
    for i, n in enumerate((1, 2, 23, 24, 25, 48, 49)):
        b = BufSpec(n, 0, n, FMTS[i % 2], 1)
        out.append((b, False, 0, 2000 * i, f"tiny{n}_oneshot"))
        out.append((b, True, n // 2, 2000 * i + 1, f"tiny{n}_looped"))


def _formats(step, todo0, out):
    # a frame_step 2 channel view of an interleaved buffer with a short loop; u8 (the generic loader) with loops
    bv = BufSpec(64, 3, 8, ol.FMT_FLOAT, 2)
    out.append((bv, True, 1, 3000, "view2_short_loop"))
    out.append((bv, True, 7, 3000, "view2_at_end_minus_1"))
    bvi = BufSpec(1400, 40, 1300, ol.FMT_SHORT, 2)
    out.append((bvi, True, 1290, 11, "view2_i16_long_loop"))
    out.append((BufSpec(2000, 50, 1500, ol.FMT_UBYTE, 1), True, 1480, 9, "u8_loop_end"))


GROUPS = (_loop_lengths, _boundary, _linear_limit, _positions, _tiny, _formats)
STEPS = (1, 30000, 60211, FRAC_ONE, 65537, 131072, 200000, MAX_PITCH)


def todo_of(step):
    # ragged update lengths: wraps land on an update's last sample and inside the 64-sample gain ramp; a first update
    # short enough that a double-speed window still fits the register gather
    first = 1024 if step <= FRAC_ONE else (500 if step <= 2 * FRAC_ONE else 300)
    return (first, 37, 1, 700, 1024)


def scene(step, frac_zero=False):
    """The cases of one pitch: [Voice].  frac_zero: every fraction 0 (step 1.0: the 1:1 copy)."""
    todo = todo_of(step)
    raw = []
    for g in GROUPS:
        g(step, todo[0], raw)
    out = []
    for b, looping, pos, frac, name in raw:
        frac = 0 if frac_zero else frac
        out.append(Voice(b, looping, pos, frac, classify(b, looping, pos, frac, step, todo[0]), name))
    return out


FILLER_STEP, FILLER_RESAMPLER = 47000, ol.RS_BSINC12
FILLER_BUF = BufSpec(6000, 100, 5900, ol.FMT_FLOAT, 1)


def layout(voices, mixed, total=None):
    """Voice slots: [(Voice, is_edge)].  mixed: every 4th slot (a workgroup's key voice of the 4-wide kernels) a quiet
    filler on another resampler, so the edge voices do not share their workgroup's resampler key and take the generic
    loader.  total: pad with quiet fillers to this many voices, edge voices spread over the whole range."""
    slots = []
    for v in voices:
        if mixed and len(slots) % 4 == 0:
            slots.append((None, False))
        slots.append((v, True))
    if total is not None:
        assert total >= len(slots)
        spread = [(None, False)] * total
        stride = total // len(slots)
        for i, s in enumerate(slots):
            spread[i * stride + (i * 7) % max(stride, 1)] = s
        slots = spread
    return slots


def run(L, step, form="hrtf", mhr=None, mixed=False, total=None, frac_zero=False, only=None, loop_end_to_len=False,
        move_in=False, scene_kw=None, kernel_names=None, via_blocks=False, todo=None, stats=None):
    """One pitch's cases on one scene.  form: 'hrtf', 'hrtf_sends', 'dry', 'dry_sends'.  only: the indices of scene()
    to play (one voice per scene for the bit-exact checks).  loop_end_to_len / move_in: the liveness variants (every
    buffer's loop end moved to its sample length; positions at or past the loop end moved into the loop).
    Returns (buses per update, [(play state, position, fraction, has buffer, fading) per voice] per update)."""
    voices = scene(step, frac_zero)
    if only is not None:
        voices = [voices[i] for i in only]
    slots = layout(voices, mixed, total)
    resampler = ol.RS_SPLINE
    todo = todo or todo_of(step)
    hrtf = form.startswith("hrtf")
    sends = {"hrtf": 0, "hrtf_sends": 1, "dry": 0, "dry_sends": 2}[form]
    if hrtf:
        L.hrtf_load(mhr)
    sc = L.make_scene(num_dry=4 if hrtf else 5, num_real=2 if hrtf else 0, num_sends=sends, num_slots=sends,
                      wet_channels=4, hrtf=hrtf, **(scene_kw or {}))
    if kernel_names is not None:
        kernel_names.append(sc.voice_kernel_name())
    if hrtf:
        rng = np.random.default_rng(5)
        cc = np.zeros((4, 128, 2), np.float32)
        cc[:, :64] = rng.uniform(-0.2, 0.2, (4, 64, 2))
        sc.set_direct_hrtf(cc, [1.0, 0.8, 0.8, 0.8], 400.0 / 48000.0, 64)
    handles = {}

    def handle(b):
        if b not in handles:
            data = encode(buffer_data(b, seed=17 * b.n + b.ls + 3 * b.le), b.fmt)
            handles[b] = sc.add_buffer(data, b.fmt, frame_step=b.fs, loop_start=b.ls,
                                       loop_end=b.n if loop_end_to_len else b.le)
        return handles[b]

    params = []
    for i, (v, edge) in enumerate(slots):
        gain = 0.5 if edge else 1e-3
        r = np.random.default_rng(1000 + i)
        if edge:
            pos = v.pos
            if move_in and v.looping and pos >= v.buf.le:
                pos = v.buf.le - 1
            sc.add_voice(handle(v.buf), looping=v.looping, position=pos, frac=v.frac)
        else:
            sc.add_voice(handle(FILLER_BUF), looping=True, position=(i * 7919) % 5000, frac=(i * 977) % 65536)
        snd = [(s, r.uniform(0.1, 0.4, 4) * gain, ol.default_filter()) for s in range(sends)]
        st, rs = (step, resampler) if edge else (FILLER_STEP, FILLER_RESAMPLER)
        if hrtf:
            p = ol.make_voice_params(st, rs, hrtf=(r.uniform(-0.5, 0.5), r.uniform(-np.pi, np.pi), 2.0, 0.0, gain),
                                     sends=snd)
        else:
            p = ol.make_voice_params(st, rs, dry_gains=r.uniform(0.3, 1.0, 5) * gain, sends=snd)
        params.append(p)
        if not via_blocks:
            sc.set_params(i, p)
    if via_blocks:             # the product's parameter blocks (oalgpu_mix_update_run): all voices' parameters in the first
        arr = (ol.VoiceParams * len(params))(*params)
        first = sc.param_block(np.arange(len(params)), arr)
        sc.resident_set_short_run(0)
    buses, ints = [], []
    for k in range(len(todo)):
        n = todo[k]
        if via_blocks:
            assert n == todo[0]
            sc.mix_run([first if k == 0 else None], n, post_process=hrtf)
        else:
            sc.mix(n, post_process=hrtf)
        out = [sc.dry()[:, :n].ravel()]
        if hrtf:
            out.append(sc.hrtf_accum().ravel())
        for s in range(sends):
            out.append(sc.wet(s)[:, :n].ravel())
        buses.append(np.concatenate(out))
        sts = []
        for i in range(len(slots)):
            st = sc.voice_state(i)
            sts.append((st.play_state, st.position, st.position_frac, st.has_buffer, st.fading))
        ints.append(sts)
    if stats is not None:
        stats.append(sc.resident_stats())
    sc.close()
    return buses, ints, [i for i, (v, e) in enumerate(slots) if e]
