"""Several contexts on one device: attached contexts mix into the device context's lines (oalgpu_context_attach,
include/oalgpu.h; ProcessContexts, alc/alu.cpp:2177-2273) -- against the reference composed as tests/attach_cases.py says,
and the pipelined device context against its one-stream twin.

Bounds: none of its own.  EXACT with one contributor per line: the bits (what
tests/test_gpu_parity.py::test_scene_single_voice_bit_exact asserts of an EXACT single-voice HRTF scene with its
post-process).  FAST HRTF: tests/test_tolerance_model.py's multi_voice_tolerance(voices, 64, max|ref|) through
test_gpu_baseline_configs.close_to, the expression the config-3 tests use; sums of voices on lines: the same with one
term per voice."""
import numpy as np
import pytest

import attach_cases as ac
import oracle_lib as ol

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _need():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    L = ac.reference()
    if L is None:
        pytest.skip("needs the compiled reference (oracle/_ref)")
    return oalgpu, L


def _hrtf_pair(oalgpu, L, mode, nvoices, flags=0):
    """-> (api, irsize); both sides have the reference's own Default HRTF loaded"""
    info = L.hrtf_load(ac.REAL_MHR)
    api = oalgpu.Api(mode, ctx_flags=flags)
    api.hrtf_load(ac.REAL_MHR)
    return api, int(info.ir_size)


def _reference_hrtf_update(odev, ochild, n):
    """steps 1-4 of tests/attach_cases.py for the HRTF device with its one attached context; -> the six lines"""
    odev.mix(n, post_process=False)
    ochild.mix(n, post_process=False)
    ac.compose(odev.dry_view(), [(ochild.dry(), ac.CHILD_MAP)], n)
    odev.post_process(n)
    return odev.dry()


def test_exact_hrtf_device_with_bformat_and_direct_channel_voices():
    """An EXACT HRTF device context with ONE HRTF voice; attached: a 6-line context with a first-order B-Format source on the
    dry lines (decoded by MixDirectHrtf) and a stereo source on RealOut L/R (direct channels).  Four updates of 1024, 1024,
    1000 and 24 frames, gain and filter targets of every voice changing before the second.  Every destination line has one
    contributor besides the HRTF sum, so the comparison is what
    tests/test_gpu_parity.py::test_scene_single_voice_bit_exact uses for an EXACT single-voice HRTF scene and its
    post-process: bit equality -- of all six lines and of the 16-bit PCM oalgpu_read_output makes of them."""
    from test_output_stage import sample_conv
    oalgpu, L = _need()
    api, irsize = _hrtf_pair(oalgpu, L, oalgpu.MATH_EXACT, 1)
    gdev = ac.build_hrtf_device(api, 1, irsize, max_voices=1)
    gchild, ga, gs = ac.build_child(api, max_voices=6)
    odev = ac.build_hrtf_device(L, 1, irsize)
    ochild, oa, os_ = ac.build_child(L)
    gdev.attach(gchild, ac.CHILD_MAP)
    gdev.set_output(oalgpu.OUT_I16, 0.0, 22222)
    for k, n in enumerate((1024, 1024, 1000, 24)):
        if k == 1:      # ramps and filter transitions cross the merge
            for sc, a, s in ((gchild, ga, gs), (ochild, oa, os_)):
                ac.child_update(sc, a, s, 1)
            gdev.set_params(0, ac.hrtf_params(0, 1))
            odev.set_params(0, ac.hrtf_params(0, 1))
        gdev.mix(n, post_process=True)
        want = _reference_hrtf_update(odev, ochild, n)
        got = gdev.dry()
        for line in range(6):
            assert np.abs(want[line, :n]).max() > 1e-3, (k, line)              # every line sounds
            assert np.array_equal(_bits(got[line, :n]), _bits(want[line, :n])), \
                (k, line, float(np.abs(got[line, :n] - want[line, :n]).max()))
        pcm = gdev.read_output(n, 2)
        assert np.array_equal(pcm, sample_conv(want[4:], oalgpu.OUT_I16, n, 2)), k
        assert np.array_equal(_bits(gchild.dry()[:, :n]), _bits(ochild.dry()[:, :n])), k      # readable on its own
    # integer state of every voice of both contexts
    assert ac.int_state(gdev.voice_state(0)) == ac.int_state(odev.voice_state(0))
    for c in range(4):
        assert ac.int_state(gchild.voice_state(ga + c)) == ac.int_state(ochild.voice_state(oa)), c
    for c in range(2):
        assert ac.int_state(gchild.voice_state(gs + c)) == ac.int_state(ochild.voice_state(os_)), c
    gchild.close(); gdev.close(); ochild.close(); odev.close()


NV_FAST = 8
UPDATES_FAST = 6


def _run_fast_device(oalgpu, api, irsize, flags, through_ring):
    """Six updates of the FAST HRTF device (8 voices) with its attached context, whose voices move before every update.
    through_ring: nothing is read back between the updates but oalgpu_read_output_async tickets, collected one update late;
    None: nothing at all is read between the updates -- only the attached context's setters and oalgpu_mix_update are called --
    and the one entry of the result is the device context's six lines after the last update.
    -> (per update [2, 1024] output lines, the attached context's lines after the last update, kernel name)"""
    gdev = ac.build_hrtf_device(api, NV_FAST, irsize, max_voices=NV_FAST, flags=flags)
    name = gdev.voice_kernel_name()
    gchild, ga, gs = ac.build_child(api, max_voices=6)
    gdev.attach(gchild, ac.CHILD_MAP)
    assert gdev.voice_kernel_name() == name
    outs, tickets = [], []
    for k in range(UPDATES_FAST):
        if k:
            ac.child_update(gchild, ga, gs, k)
        gdev.mix(1024, post_process=True)
        if through_ring:
            tickets.append(gdev.read_output_async())
            if k:
                outs.append(gdev.output_wait(tickets[k - 1]).copy())
        elif through_ring is not None:
            outs.append(gdev.dry()[4:6].copy())
    if through_ring:
        outs.append(gdev.output_wait(tickets[-1]).copy())
    elif through_ring is None:
        outs.append(gdev.dry().copy())
    child_lines = gchild.dry()
    states = [ac.int_state(gchild.voice_state(v)) for v in range(6)] + [ac.int_state(gdev.voice_state(v)) for v in range(NV_FAST)]
    gchild.close(); gdev.close()
    return outs, child_lines, name, states


def test_fast_pipelined_hrtf_device_and_its_serial_twin():
    """The same scene with 8 HRTF voices on a FAST device context -- the two-stream pipeline, read only through
    oalgpu_read_output_async tickets (the ring the post-process kernel fills) -- against the composed reference within the
    FAST HRTF bound, and BIT FOR BIT against a twin whose device context is OALGPU_CTX_SERIAL: merge k reads reduction k of
    every attached context, not k + 1 and not k - 1."""
    from test_gpu_baseline_configs import close_to
    oalgpu, L = _need()
    api, irsize = _hrtf_pair(oalgpu, L, oalgpu.MATH_FAST, NV_FAST)
    plain = ac.build_hrtf_device(api, NV_FAST, irsize, max_voices=NV_FAST)
    usual = plain.voice_kernel_name()
    plain.close()
    piped, child_lines, name, states = _run_fast_device(oalgpu, api, irsize, 0, True)
    serial, child_serial, _, states_serial = _run_fast_device(oalgpu, api, irsize, oalgpu.CTX_SERIAL, False)
    assert name == usual and name.startswith("VoiceWave"), (name, usual)       # the device context's usual voice kernel
    # ---- the reference
    odev = ac.build_hrtf_device(L, NV_FAST, irsize)
    ochild, oa, os_ = ac.build_child(L)
    direct = 0.0
    for k in range(UPDATES_FAST):
        if k:
            ac.child_update(ochild, oa, os_, k)
        want = _reference_hrtf_update(odev, ochild, 1024)
        # the HRTF voices' 64-tap sums and the attached context's one term per line
        close_to(piped[k], want[4:6], f"update {k}: output lines through the ring", (NV_FAST + 6, 64))
        direct = max(direct, float(np.abs(ochild.dry()[4:6]).max()))
        assert np.array_equal(_bits(piped[k]), _bits(serial[k])), f"update {k}: pipelined and serial device contexts differ"
    assert direct > 0.05                                                       # the direct channels are a large part of the output
    close_to(child_lines[:4], ochild.dry()[:4], "the attached context's lines 0-3 (oalgpu_read_dry)", (6, 1))
    assert np.array_equal(_bits(child_lines), _bits(child_serial))
    want_states = [ac.int_state(ochild.voice_state(oa))] * 4 + [ac.int_state(ochild.voice_state(os_))] * 2 \
        + [ac.int_state(odev.voice_state(v)) for v in range(NV_FAST)]
    assert states == want_states and states_serial == want_states
    ochild.close(); odev.close()


@pytest.mark.parametrize("flag", ["OALGPU_CTX_APPLY_IN_VOICE_KERNEL", "OALGPU_CTX_FUSED_REDUCE"])
def test_deferred_and_fused_device_contexts_mix_what_the_plain_one_mixes(flag):
    """What a device context declines while something is attached, beside the resident launch.  With
    OALGPU_CTX_APPLY_IN_VOICE_KERNEL an update is submitted one library call late: here the next call is a setter of the
    ATTACHED context, which must submit the device context's update first -- the update mixes the attached voices as they
    were when it was called.  With OALGPU_CTX_FUSED_REDUCE reduction and post-process are one launch, which would reduce over
    the merged lines: the flag is declined while attached.  Either way: the bits of the context without the flag."""
    oalgpu, L = _need()
    api, irsize = _hrtf_pair(oalgpu, L, oalgpu.MATH_FAST, NV_FAST)
    bit = {"OALGPU_CTX_APPLY_IN_VOICE_KERNEL": oalgpu.CTX_APPLY_IN_VOICE_KERNEL, "OALGPU_CTX_FUSED_REDUCE": oalgpu.CTX_FUSED_REDUCE}[flag]
    for ring in (None, True):
        plain, child_plain, _, states_plain = _run_fast_device(oalgpu, api, irsize, 0, ring)
        got, child_got, _, states = _run_fast_device(oalgpu, api, irsize, bit, ring)
        assert len(got) == len(plain) == (1 if ring is None else UPDATES_FAST)
        for k, (a, b) in enumerate(zip(got, plain)):
            assert np.abs(b).max() > 1e-2
            assert np.array_equal(_bits(a), _bits(b)), (flag, ring, k, float(np.abs(a - b).max()))
        assert np.array_equal(_bits(child_got), _bits(child_plain)) and states == states_plain


def _run_speaker_device(oalgpu, api, order, line3_scale=1.0):
    """A speaker device (4 dry + 2 real lines, stereo B-Format decoder, 2 voices) with attached A (3 voices, identity map) and
    B (2 voices with a send into a slot whose dedicated effect writes B's lines 0-1; map [0, 1, 2, -1]); four updates.
    -> (per update the device's six lines, B's line 3 after the last update)"""
    from oalgpu import synth
    dev = ac.build_lines(api, 2, 1, num_real=2, max_voices=2)
    dev.set_bformat_decoder(synth.stereo_decoder()[0])
    a = ac.build_lines(api, 3, 2, max_voices=3)
    b = ac.build_lines(api, 2, 3, send=True, line3_scale=line3_scale, max_voices=2)
    fx = oalgpu.Effect(oalgpu.EFFECT_DEDICATED, 4, 4, 48000, api.mode)
    fx.update(None, None, np.asarray(ac.DEDICATED_GAINS, np.float32))
    b.set_slot_effect(0, fx)
    for which in order:
        dev.attach(a if which == "A" else b, [0, 1, 2, 3] if which == "A" else [0, 1, 2, -1])
    outs = []
    for n in SPEAKER_SIZES:
        dev.mix(n, post_process=True)
        outs.append(dev.dry()[:, :n].copy())
    b3 = b.dry()[3].copy()
    a.close(); b.close(); dev.close(); fx.close()
    return outs, b3


SPEAKER_SIZES = (1024, 1000, 24, 1024)


def _reference_speaker_device(L, order):
    from oalgpu import synth
    hf = synth.stereo_decoder()[0]
    dev = ac.build_lines(L, 2, 1, num_real=2)
    a = ac.build_lines(L, 3, 2)
    b = ac.build_lines(L, 2, 3, send=True)
    fx = ac.ReferenceDedicated(L, ac.DEDICATED_GAINS)
    dec = ol.BFormatDec(L, 4, hf)
    outs = []
    for n in SPEAKER_SIZES:
        dev.mix(n, post_process=False)
        a.mix(n, post_process=False)
        b.mix(n, post_process=False)
        fx.process(b.wet(0)[0], b.dry_view(), n)              # behind B's voices, in front of the merge
        maps = {"A": (a.dry(), [0, 1, 2, 3]), "B": (b.dry(), [0, 1, 2, -1])}
        lines = dev.dry_view()
        ac.compose(lines, [maps[w] for w in order], n)
        real = np.ascontiguousarray(lines[4:])
        dec.process(real, lines[:4], n)
        outs.append(np.concatenate([lines[:4, :n], real[:, :n]]))
    dec.close(); a.close(); b.close(); dev.close()
    return outs


def test_speaker_device_with_two_attached_contexts_on_the_same_lines():
    """Two attached contexts add into the same dry lines of a speaker device; B's dedicated effect writes into B's lines
    behind its voices, and the merge sits behind that.  Against the composed reference within the bound for sums of voices
    (7 voices, one term each); two runs give the same bits; the swapped attach order stays within the bound (another order
    of the adds: equality is not required); B's line 3 is mapped nowhere -- three times its level changes nothing."""
    from test_gpu_baseline_configs import close_to
    oalgpu, L = _need()
    api = oalgpu.Api(oalgpu.MATH_FAST)
    first, b3 = _run_speaker_device(oalgpu, api, "AB")
    again, _ = _run_speaker_device(oalgpu, api, "AB")
    swapped, _ = _run_speaker_device(oalgpu, api, "BA")
    louder, b3_louder = _run_speaker_device(oalgpu, api, "AB", line3_scale=3.0)
    want_ab = _reference_speaker_device(L, "AB")
    want_ba = _reference_speaker_device(L, "BA")
    plain = ac.build_lines(api, 2, 1, num_real=2, max_voices=2)             # the device context alone, for what the attachments add
    plain.mix(1024, post_process=False)
    alone = plain.dry()[:4]
    plain.close()
    assert np.abs(first[0][:4] - alone).max() > 0.1                         # the attached contexts are most of the lines
    for k in range(len(SPEAKER_SIZES)):
        close_to(first[k], want_ab[k], f"update {k}: A then B", (7, 1))
        close_to(swapped[k], want_ba[k], f"update {k}: B then A", (7, 1))
        close_to(swapped[k], want_ab[k], f"update {k}: B then A against the other order's reference", (7, 1))
        assert np.array_equal(_bits(first[k]), _bits(again[k])), k
        assert np.array_equal(_bits(first[k]), _bits(louder[k])), k
        assert np.abs(want_ab[k][4:]).max() > 1e-2                          # the decoder ran on the merged lines
    assert np.abs(b3).max() > 1e-2 and np.abs(b3_louder - b3).max() > 1e-2  # line 3 of B sounds, and reaches nothing


def test_resident_flag_is_declined_while_attached():
    """An OALGPU_CTX_RESIDENT device context launches per update while a context is attached (the resident launch has no
    merge): resident_stats().launches grows before the attach, stands still over 40 attached updates -- whose output is the
    launched twin's within the FAST HRTF bound -- and grows again after the detach."""
    import os
    import sys
    sys.path.insert(0, ac.ROOT)
    import bench
    from oalgpu import synth
    from test_gpu_baseline_configs import close_to
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    nv, updates = 512, 40
    mhr = synth.synth_mhr_bytes()
    outs = {}
    for mode in ("resident", "launched"):
        api = oalgpu.Api(oalgpu.MATH_FAST, ctx_flags=(oalgpu.CTX_RESIDENT if mode == "resident" else 0) | oalgpu.CTX_WAVE_PAIRS)
        api._mhr = mhr
        dev, script = bench.build_scene(oalgpu, synth, api, 3, nv, 0, mhr, 0)
        allv = list(range(nv))
        moving = [v for v in allv if script.is_moving(v)]
        dev.set_params_batch(allv, bench.param_array(oalgpu, script, allv, 0))
        blocks = [dev.param_block(moving, bench.param_array(oalgpu, script, moving, k + 1)) for k in range(updates + 8)]
        child, ga, gs = ac.build_child(oalgpu.Api(oalgpu.MATH_FAST), max_voices=6)
        step = iter(range(updates + 8))

        def run(count):
            for _ in range(count):
                k = next(step)
                dev.apply_block(blocks[k])
                dev.mix(1024, post_process=True)

        if mode == "resident":
            dev.resident_set_short_run(0)
            before = dev.resident_stats()["launches"]
            run(4)
            grown = dev.resident_stats()["launches"]
            assert grown > before, (before, grown)
        else:
            run(4)
        dev.attach(child, ac.CHILD_MAP)
        run(updates)
        outs[mode] = dev.dry().copy()
        if mode == "resident":
            info = dev.resident_stats()
            assert info["launches"] == grown and info["failed"] == 0, info
            child.detach()
            run(4)
            dev.sync()
            assert dev.resident_stats()["launches"] > grown
        child.close(); dev.close()
    assert np.abs(outs["launched"][4:6]).max() > 1e-2
    close_to(outs["resident"], outs["launched"], "attached updates of the resident-flag context against its launched twin", (nv + 6, 64))
