"""Shared EAX-reverb scenarios: a list of (name, schedule) where a schedule is a list of
per-update steps {props: kwargs for ReverbProps.make, slot_gain, n} -- None props = no update()
before that process() call.  Input is seeded noise bursts on the 4-line wet bus."""
import zlib

import numpy as np

BUFFER_LINE = 1024


def out_init(nlines):
    """process() ADDS into the target lines: start them from a recognisable non-zero pattern."""
    o = np.zeros((nlines, BUFFER_LINE), np.float32)
    o[:, :7] = 0.125
    return o


def wet_input(seed, updates, burst_every=3):
    rng = np.random.default_rng(seed)
    x = np.zeros((updates, 4, BUFFER_LINE), np.float32)
    for u in range(updates):
        if u % burst_every == 0:
            x[u] = (rng.standard_normal((4, BUFFER_LINE)) * 0.25).astype(np.float32)
            x[u, 1:] *= 0.5
    return x


def _steps(first, count, later=None):
    s = [dict(props=first, slot_gain=1.0, n=BUFFER_LINE)]
    s += [dict(props=None, slot_gain=1.0, n=BUFFER_LINE) for _ in range(count - 1)]
    for k, v in (later or {}).items():
        s[k] = dict(props=v, slot_gain=s[k].get("slot_gain", 1.0), n=BUFFER_LINE)
    return s


CASES = [
    # AL_EAXREVERB_DEFAULT_*: first update from DeviceClear, then steady state
    ("default", _steps({}, 8)),
    # modulation active (Mod.Depth > 0 -> fractional cubic taps on the feedback lines)
    ("modulated", _steps(dict(modulation_depth=0.8, modulation_time=0.7, diffusion=0.6), 8)),
    # panned early/late reflections and non-unit shelf gains
    ("panned", _steps(dict(reflections_pan=(0.3, 0.1, -0.4), late_reverb_pan=(-0.2, 0.0, 0.9), gain_hf=0.4,
                          gain_lf=0.7, reflections_gain=0.6, late_reverb_gain=2.0), 6)),
    # small density -> short lines.  At 48 kHz this bounds nothing: mLate.Offset[0] is 465 there, above the 256-sample
    # sub-block; only the all-pass chunks (23 samples) are short.  RATE_CASES below reach the bounded sub-blocks.
    ("dense_small_room", _steps(dict(density=0.0, diffusion=0.3, decay_time=0.4, decay_hf_ratio=0.3,
                                     decay_lf_ratio=1.5, decay_hf_limit=0), 6)),
    # partial update (gain/pan/delays only: taps cross-fade, no pipeline swap)
    ("partial_update", _steps({}, 8, {3: dict(gain=0.6, reflections_delay=0.02, late_reverb_delay=0.03,
                                             reflections_pan=(0.5, 0.0, 0.0))})),
    # full update -> StartFade / Fading / Cleanup / Normal with both pipelines running
    ("pipeline_fade", _steps({}, 14, {2: dict(density=0.5, decay_time=2.5, diffusion=0.8)})),
    # two full updates in a row while the first fade is still running
    ("double_fade", _steps(dict(decay_time=0.3), 12, {2: dict(decay_time=3.0, modulation_depth=0.5),
                                                      4: dict(decay_time=1.0, density=0.2)})),
    # short / ragged process() sizes
    ("ragged", [dict(props={}, slot_gain=0.8, n=1024), dict(props=None, slot_gain=0.8, n=100),
                dict(props=None, slot_gain=0.8, n=1), dict(props=dict(decay_time=2.0), slot_gain=0.8, n=333),
                dict(props=None, slot_gain=0.8, n=1024), dict(props=None, slot_gain=0.8, n=257),
                dict(props=None, slot_gain=0.8, n=1024), dict(props=None, slot_gain=0.8, n=1024)]),
]

SEED = {name: zlib.crc32(name.encode()) % 1000 for name, _ in CASES}
FULL_CASES = ("default", "ragged")      # cases whose golden fixture holds the lines, not only CRCs


# ---- device rates other than 48 kHz -----------------------------------------------------------------------------------
# Every delay, tap, window and sub-block length is seconds x rate.  CASES run at each of RATES as well; RATE_CASES are
# built for what only a low rate reaches (see check_reach for what each must prove from the reference's block).
RATES = (8000, 11025, 16000, 22050, 32000, 44100)
LATE_BLOCK = 256            # MAX_UPDATE_SAMPLES: processLate takes min(mLate.Offset[0], 256, left) per sub-block
SHORT_LATE_RATES = (8000, 11025, 16000, 22050)      # density 0: mLate.Offset[0] = 77, 106, 154, 213


def _ragged_tail(gain=1.0):
    return [dict(props=None, slot_gain=gain, n=n) for n in (1, 100, 257, 333, 1023, 1024)]


_LONGEST = dict(reflections_delay=0.3, late_reverb_delay=0.1, density=1.0, decay_time=20.0)

RATE_CASES = [
    # density 0: at 8000-22050 Hz mLate.Offset[0] < 256 bounds the late sub-blocks, so the late wave runs more sub-blocks
    # than the early one; then ragged n so that `left` and Offset[0] take turns being the minimum
    ("short_late_blocks_lowdiff", _steps(dict(density=0.0, diffusion=0.1, decay_time=1.0), 5) + _ragged_tail()),
    ("short_late_blocks_highdiff", _steps(dict(density=0.0, diffusion=1.0, decay_time=0.6, modulation_depth=0.5), 5)
     + _ragged_tail()),
    # density 1 (256-sample late blocks) -> 0 (short ones) with noise running: both pipelines side by side with
    # different sub-block counts; back again while the first fade is still running
    ("density_across_the_threshold", _steps({}, 12, {2: dict(density=0.0), 4: dict(density=1.0, decay_time=1.0)})),
    # hf0norm = min(hf_reference / rate, 0.49): capped below 40.8 kHz
    ("hf_cap_lf20", _steps(dict(hf_reference=20000.0, lf_reference=20.0, decay_hf_ratio=0.1, decay_hf_limit=1), 8,
                           {4: dict(hf_reference=20000.0, lf_reference=20.0, decay_hf_ratio=2.0, decay_hf_limit=0)})),
    ("hf_cap_lf1000", _steps(dict(hf_reference=20000.0, lf_reference=1000.0, decay_hf_ratio=0.1, decay_hf_limit=0), 8,
                             {4: dict(hf_reference=20000.0, lf_reference=1000.0, decay_hf_ratio=2.0, decay_hf_limit=1)})),
    ("modulated_low_rate_fast", _steps(dict(modulation_depth=1.0, modulation_time=0.04, density=0.0), 8)),
    ("modulated_low_rate_slow", _steps(dict(modulation_depth=1.0, modulation_time=4.0), 8)),
    # the main-line taps at their furthest: 0.3 s is 14.06 updates at 48 kHz
    ("longest_delays", _steps(dict(_LONGEST), 18)),
    # partial update from the default delays to the longest: the two taps of the cross-fade are far apart
    ("longest_delays_partial", _steps({}, 18, {3: dict(reflections_delay=0.3, late_reverb_delay=0.1)})),
]
LONGEST_DELAY_CASES = ("longest_delays", "longest_delays_partial")       # these also run at 48000
ALL_CASES = CASES + RATE_CASES
RATE_MATRIX = [(name, sched, rate) for name, sched in ALL_CASES for rate in RATES] + \
    [(name, sched, 48000) for name, sched in RATE_CASES if name in LONGEST_DELAY_CASES]
RATE_IDS = [f"{name}-{rate}" for name, _, rate in RATE_MATRIX]


def rate_seed(name, rate):
    return zlib.crc32(f"{name}@{rate}".encode()) % 100000


def _bq_bytes(pipe):
    return bytes(memoryview(pipe.filter_lp)) + b"".join(bytes(memoryview(f)) for f in pipe.t60_hf)


def check_reach(ref_lib, props_cls, name, rate, k, step, blk, state_before):
    """What a case is for, proven from the REFERENCE's parameter block `blk` right after its k-th update() (`step` is the
    schedule step of that update, `state_before` the reference's pipeline_state before it)."""
    cur = blk.pipe[blk.current_pipeline]
    old = blk.pipe[1 - blk.current_pipeline]
    density = (step["props"] or {}).get("density", 1.0)
    if name.startswith("short_late_blocks") or (name == "density_across_the_threshold" and k == 1):
        if rate in SHORT_LATE_RATES:
            assert cur.late_offset[0] < LATE_BLOCK, (name, rate, cur.late_offset[0])
        else:
            assert cur.late_offset[0] >= LATE_BLOCK, (name, rate, cur.late_offset[0])
    if name == "density_across_the_threshold":
        if k == 1:      # the old pipeline keeps 256-sample late blocks while it fades out
            assert old.late_offset[0] >= LATE_BLOCK and blk.pipeline_state != 4, (rate, old.late_offset[0])
        if k == 2:      # ... and the first fade was still running when the next full update arrived
            assert state_before != 4 and cur.late_offset[0] >= LATE_BLOCK, (rate, state_before)
    if rate == 8000 and density == 0.0:
        assert cur.early_ap_offset[0] == 3 and cur.late_ap_offset[0] == 6, \
            (name, list(cur.early_ap_offset), list(cur.late_ap_offset))
    if name.startswith("hf_cap"):
        # the same update with hf_reference just above 0.49 x rate (0.49 x rate itself, rounded, may divide back to a
        # hair under the cap): identical filter designs <=> hf_reference 20000 is capped at this rate
        other = ref_lib.make_reverb(4, rate)
        kw = dict(step["props"]); kw["hf_reference"] = 0.49 * rate * (1.0 + 1e-5)
        other.update(props_cls.make(**kw), step["slot_gain"])
        capped = _bq_bytes(other.get_params().pipe[other.get_params().current_pipeline])
        other.close()
        if 20000.0 / rate > 0.49:
            assert _bq_bytes(cur) == capped, (name, rate, "hf0norm not capped")
        else:
            assert _bq_bytes(cur) != capped, (name, rate, "hf0norm unexpectedly capped")
    if name in LONGEST_DELAY_CASES and (step["props"] or {}).get("reflections_delay") == 0.3:
        assert min(cur.early_delay_tap[j][1] for j in range(4)) >= int(0.3 * rate), (name, rate)


def check_longest_delays(name, rate, schedule, outs, blk):
    """`outs`: the reference's output of every update (started from out_init).  With the burst of update 0 the only
    input so far, nothing can come out before the first early tap (0.3 s); after it the signal is back."""
    if name != "longest_delays":
        return
    tap = min(blk.pipe[blk.current_pipeline].early_delay_tap[j][1] for j in range(4))
    flat = np.concatenate([o[:, :st["n"]] - out_init(o.shape[0])[:, :st["n"]] for o, st in zip(outs, schedule)], axis=1)
    assert flat.shape[1] > tap + BUFFER_LINE, "the schedule must outlast the reflections delay"
    assert np.all(flat[:, :tap] == 0.0), (rate, tap, int(np.flatnonzero(np.abs(flat).sum(axis=0))[0]))
    assert np.abs(flat[:, tap:tap + BUFFER_LINE]).max() > 1e-6, (rate, tap)
