"""Effect slot targets on the GPU (oalgpu_slot_set_target, include/oalgpu.h): a slot's effects add into another slot's wet bus,
the slots run by descending depth -- against the compiled reference's effect states composed on the host in the documented
order over the voices-only buses of a copy of the scene without effects (tests/slot_target_cases.py).

Bounds: none of its own.  The equalizer, echo, compressor and square-carrier modulator are bit-identical to the reference
(tests/test_effects.py), the EXACT EAX reverb is (tests/test_reverb.py), and the inputs are the same bits: those chains are
compared bit for bit in both math modes.  FAST reverbs: tests/test_reverb.py::test_gpu_fast_mode_matches_oracle's bound,
2e-5 of the run's maximum + 1e-7.  Convolutions: tests/test_conv.py's close().  The HRTF case: the bound of
tests/test_effects.py::test_effect_on_a_context_slot behind the post-process, the bits ahead of it."""
import numpy as np
import pytest

import slot_target_cases as st
from slot_target_cases import SIZES, bits

pytestmark = pytest.mark.gpu
MODES = ["exact", "fast"]


def _need():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    L = st.reference()
    if L is None:
        pytest.skip("needs the compiled reference")
    return oalgpu, L


def _run_chain(mode, L, num_slots, targets, chain, sizes=SIZES, compare="bits"):
    """The chained copy against the composition over the copy without effects, update by update.
    -> per update (dry, [wet per slot]) of the chained copy, frames [0, n)."""
    api = st.api_for(mode)
    chained, plain = st.build_scene(api, num_slots), st.build_scene(api, num_slots)
    made = st.install(chained, mode, targets, chain)
    assert [chained.slot_target(s) for s in range(num_slots)] == list(targets)
    outs, run = [], []
    for k, n in enumerate(sizes):
        chained.mix(n, post_process=True)
        plain.mix(n, post_process=True)
        got_dry, got_wets = chained.dry(), [chained.wet(s) for s in range(num_slots)]
        want_dry, want_wets = st.compose(targets, chain, plain.dry(), [plain.wet(s) for s in range(num_slots)], n)
        assert np.abs(want_dry[:st.NUM_DRY, :n]).max() > 1e-3, k
        pairs = [("dry", got_dry, want_dry)] + [(f"wet({s})", got_wets[s], want_wets[s]) for s in range(num_slots)]
        for name, a, b in pairs:
            err = float(np.abs(a[:, :n].astype(np.float64) - b[:, :n]).max())
            print(f"{mode} update {k} n={n} {name}: max err {err:.3e}, max |want| {float(np.abs(b[:, :n]).max()):.3e}")
            if compare == "bits":
                assert np.array_equal(bits(a[:, :n]), bits(b[:, :n])), (mode, k, name, err)
            elif compare == "conv":
                from test_conv import close
                close(a[:, :n], b[:, :n], f"{mode} update {k} {name}")
            run.append((name, a[:, :n].astype(np.float64), b[:, :n].astype(np.float64)))
        outs.append((got_dry[:, :n].copy(), [w[:, :n].copy() for w in got_wets]))
    if compare == "run":        # tests/test_reverb.py::test_gpu_fast_mode_matches_oracle: over the run, per block of lines
        for name in sorted({r[0] for r in run}):
            scale = max(float(np.abs(b).max()) for nm, _, b in run if nm == name)
            worst = max(float(np.abs(a - b).max()) for nm, a, b in run if nm == name)
            print(f"{mode} {name}: worst {worst:.3e}, run maximum {scale:.3e}, bound {2e-5 * scale + 1e-7:.3e}")
            assert worst <= 2e-5 * scale + 1e-7, (mode, name, worst, scale)
    st.check_kernel(chained, mode)
    for s in range(num_slots):      # detach before the objects go
        chained.set_slot_effect(s, None); chained.set_slot_reverb(s, None); chained.set_slot_convolution(s, None)
    chained.close(); plain.close()
    st.close_all(made, [x for states in chain.values() for x in states])
    return outs


@pytest.mark.parametrize("mode", MODES)
def test_echo_into_equalizer(mode):
    """echo (slot 0) -> equalizer (slot 1) -> device, the voices sending into both slots and into slot 2, which has nothing"""
    oalgpu, L = _need()
    targets = [1, -1, -1]
    chain = {0: [st.RefEffect(L, st.KIND_ECHO, st.ECHO_A)], 1: [st.RefEffect(L, st.KIND_EQ, st.EQ_A)]}
    outs = _run_chain(mode, L, 3, targets, chain)
    # the same scene without the target: the echo goes to the device's lines, the equalizer hears the sends alone
    api = st.api_for(mode)
    flat = st.build_scene(api, 3)
    states = {0: [st.RefEffect(L, st.KIND_ECHO, st.ECHO_A)], 1: [st.RefEffect(L, st.KIND_EQ, st.EQ_A)]}
    made = st.install(flat, mode, [-1, -1, -1], states)
    differs = False
    for k, n in enumerate(SIZES):
        flat.mix(n, post_process=True)
        differs = differs or not np.array_equal(bits(flat.dry()[:, :n]), bits(outs[k][0]))
        if k == 0:
            assert not np.array_equal(bits(flat.wet(1)[:, :n]), bits(outs[k][1][1])), "wet(1) holds what the echo added"
    assert differs
    flat.set_slot_effect(0, None); flat.set_slot_effect(1, None)
    flat.close()
    st.close_all(made, [x for s in states.values() for x in s])


@pytest.mark.parametrize("mode", MODES)
def test_feeders_above_their_target_and_two_feeders_of_one_target(mode):
    """compressor (slot 2) and echo (slot 1) both feed the equalizer in slot 0: the feeders run first, in ascending slot order
    -- a loop in slot order would run the equalizer before anything has reached its wet bus"""
    oalgpu, L = _need()
    chain = {0: [st.RefEffect(L, st.KIND_EQ, st.EQ_B, 0.7)], 1: [st.RefEffect(L, st.KIND_ECHO, st.ECHO_B, 0.9)],
             2: [st.RefEffect(L, st.KIND_COMP, st.COMP_ON)]}
    _run_chain(mode, L, 3, [-1, 0, 0], chain)


@pytest.mark.parametrize("mode", MODES)
def test_three_deep(mode):
    """slot 0 -> slot 2 -> slot 1 -> device; slot 3 beside them goes to the device on its own"""
    oalgpu, L = _need()
    chain = {0: [st.RefEffect(L, st.KIND_MOD, st.MOD_SQUARE)], 2: [st.RefEffect(L, st.KIND_ECHO, st.ECHO_A, 0.8)],
             1: [st.RefEffect(L, st.KIND_EQ, st.EQ_A)], 3: [st.RefEffect(L, st.KIND_MOD, st.MOD_SAW, 0.8)]}
    _run_chain(mode, L, 4, [2, -1, 1, -1], chain)


@pytest.mark.parametrize("mode", MODES)
def test_reverbs_across_depths(mode):
    """reverb (slot 0) -> equalizer (slot 1), and equalizer (slot 2) -> reverb (slot 3); slot 1 has a reverb of its own too,
    which shares the depth-0 launch with slot 3's while slot 0's is the depth-1 launch"""
    oalgpu, L = _need()
    chain = {0: [st.RefReverb(L, dict(decay_time=2.0, modulation_depth=0.3), 0.7)],
             1: [st.RefEffect(L, st.KIND_EQ, st.EQ_A), st.RefReverb(L, dict(density=0.3, diffusion=0.5), 0.5)],
             2: [st.RefEffect(L, st.KIND_EQ, st.EQ_B, 0.7)],
             3: [st.RefReverb(L, dict(late_reverb_pan=(0.3, 0.0, -0.6), decay_time=0.8), 0.6)]}
    _run_chain(mode, L, 4, [1, -1, 3, -1], chain, compare="bits" if mode == "exact" else "run")


@pytest.mark.parametrize("mode", MODES)
def test_convolutions_across_depths(mode):
    """convolution (slot 0, 300 taps: the time-domain head and two frequency-domain segments) -> equalizer (slot 1), and
    equalizer (slot 2) -> convolution (slot 3)"""
    oalgpu, L = _need()
    rng = np.random.default_rng(77)
    ir = (rng.standard_normal(300) * np.exp(-np.arange(300) / 80.0) * 0.2).astype(np.float32)
    chain = {0: [st.RefConv(L, ir, 0.8)], 1: [st.RefEffect(L, st.KIND_EQ, st.EQ_A)],
             2: [st.RefEffect(L, st.KIND_EQ, st.EQ_B, 0.7)], 3: [st.RefConv(L, ir[::-1].copy(), 0.6)]}
    _run_chain(mode, L, 4, [1, -1, 3, -1], chain, compare="conv")


def test_chain_on_an_hrtf_context(synth_mhr):
    """echo (slot 0) -> equalizer (slot 1) -> the dry lines MixDirectHrtf decodes, FAST.  The effect leg from the voices-only
    wet buses of the copy without effects: the four dry lines ahead of the post-process, bit for bit (the post-process reads
    them and writes the two real lines).  The whole block behind the post-process as
    tests/test_effects.py::test_effect_on_a_context_slot compares it: the composed dry lines in the reference scene, its
    MixDirectHrtf, 2e-5 of the maximum + 1e-7."""
    oalgpu, L = _need()
    api = st.api_for("fast")
    api.hrtf_load(synth_mhr)
    L.hrtf_load(synth_mhr)
    targets = [1, -1, -1]
    chain = {0: [st.RefEffect(L, st.KIND_ECHO, st.ECHO_A)], 1: [st.RefEffect(L, st.KIND_EQ, st.EQ_A)]}
    chained, plain = st.build_scene(api, 3, hrtf=True), st.build_scene(api, 3, hrtf=True)
    osc = st.build_scene(L, 3, hrtf=True, product=False)
    made = st.install(chained, "fast", targets, chain)
    for k, n in enumerate(SIZES):
        chained.mix(n, post_process=True)
        plain.mix(n, post_process=False)
        osc.mix(n, post_process=False)
        dry0 = plain.dry()
        assert not dry0[:st.NUM_DRY].any(), "an HRTF context's voices leave the dry lines to the effects"
        want_dry, want_wets = st.compose(targets, chain, dry0, [plain.wet(s) for s in range(3)], n)
        got = chained.dry()
        assert np.array_equal(bits(got[:st.NUM_DRY, :n]), bits(want_dry[:st.NUM_DRY, :n])), k
        assert np.array_equal(bits(chained.wet(1)[:, :n]), bits(want_wets[1][:, :n])), k
        view = osc.dry_view()
        view[:st.NUM_DRY, :n] = want_dry[:st.NUM_DRY, :n]
        osc.post_process(n)
        b = osc.dry()
        err = float(np.abs(got[:, :n].astype(np.float64) - b[:, :n]).max())
        print(f"hrtf update {k} n={n}: max err {err:.3e}, max |want| {float(np.abs(b[:, :n]).max()):.3e}")
        assert np.abs(b[st.NUM_DRY:, :n]).max() > 1e-3
        assert err <= 2e-5 * float(np.abs(b[:, :n]).max()) + 1e-7, k
    st.check_kernel(chained, "fast")
    chained.set_slot_effect(0, None); chained.set_slot_effect(1, None)
    chained.close(); plain.close(); osc.close()
    st.close_all(made, [x for s in chain.values() for x in s])


def _path_run(L, path):
    """the chained FAST scene of test_three_deep through one update path; -> per update (dry, wets), frames [0, n)"""
    import oalgpu
    targets = [2, -1, 1, -1]
    chain = {0: [st.RefEffect(L, st.KIND_MOD, st.MOD_SQUARE)], 2: [st.RefEffect(L, st.KIND_ECHO, st.ECHO_A, 0.8)],
             1: [st.RefEffect(L, st.KIND_EQ, st.EQ_A)], 3: [st.RefEffect(L, st.KIND_COMP, st.COMP_ON)]}
    api = st.api_for("fast", oalgpu.CTX_APPLY_IN_VOICE_KERNEL if path == "deferred" else 0)
    scene = st.build_scene(api, 4)
    made = st.install(scene, "fast", targets, chain)
    device = None
    if path == "attached":      # a device context of the same lines with no voice playing, identity line map
        device = st.api_for("fast").make_scene(sample_rate=st.RATE, num_dry=st.NUM_DRY, num_real=st.NUM_REAL, max_voices=1)
        device.attach(scene, list(range(st.NUM_DRY + st.NUM_REAL)))
    outs = []
    for n in SIZES:
        if path in ("update", "deferred"):
            scene.mix(n, post_process=True)
        elif path == "serial":
            scene.mix_voices(n); scene.post_process(n)
        elif path == "overlapped":
            scene.mix_voices_overlapped(n); scene.post_process_overlapped(n, True)
        else:
            device.mix(n, post_process=True)
        own = scene.dry()[:, :n].copy()
        merged = device.dry()[:, :n].copy() if device is not None else own
        outs.append((own, merged, [scene.wet(s)[:, :n].copy() for s in range(4)]))
    st.check_kernel(scene, "fast")
    if device is not None:
        scene.detach()
        device.close()
    for s in range(4):
        scene.set_slot_effect(s, None)
    scene.close()
    st.close_all(made, [x for s in chain.values() for x in s])
    return outs


def test_every_update_path_gives_the_same_bits():
    """oalgpu_mix_update; oalgpu_mix_voices + oalgpu_post_process; the overlapped pair; the deferred submission; attached to a
    device context: the dry lines and every wet bus, bit for bit"""
    oalgpu, L = _need()
    base = _path_run(L, "update")
    assert any(np.abs(w).max() > 1e-3 for w in base[0][2])
    for path in ("serial", "overlapped", "deferred", "attached"):
        other = _path_run(L, path)
        for k, ((d0, m0, w0), (d1, m1, w1)) in enumerate(zip(base, other)):
            assert np.array_equal(bits(d0), bits(d1)), (path, k)
            assert np.array_equal(bits(m0), bits(m1)), (path, k, "through the merge")
            for s in range(4):
                assert np.array_equal(bits(w0[s]), bits(w1[s])), (path, k, s)


def test_an_update_without_post_process_leaves_the_wet_buses_to_the_voices():
    oalgpu, L = _need()
    api = st.api_for("fast")
    chain = {0: [st.RefEffect(L, st.KIND_ECHO, st.ECHO_A)], 1: [st.RefEffect(L, st.KIND_EQ, st.EQ_A)]}
    chained, plain = st.build_scene(api, 3), st.build_scene(api, 3)
    made = st.install(chained, "fast", [1, -1, -1], chain)
    for k, n in enumerate(SIZES[:6]):
        post = k in (0, 3)          # in between: the next reduction overwrites what the feeders added
        chained.mix(n, post_process=post)
        plain.mix(n, post_process=False)
        if post:
            assert not np.array_equal(bits(chained.wet(1)[:, :n]), bits(plain.wet(1)[:, :n])), k
            continue
        assert np.array_equal(bits(chained.dry()[:, :n]), bits(plain.dry()[:, :n])), k
        for s in range(3):
            assert np.array_equal(bits(chained.wet(s)[:, :n]), bits(plain.wet(s)[:, :n])), (k, s)
    chained.set_slot_effect(0, None); chained.set_slot_effect(1, None)
    chained.close(); plain.close()
    st.close_all(made, [x for s in chain.values() for x in s])


@pytest.mark.parametrize("mode", MODES)
def test_a_feeder_into_a_slot_with_nothing_attached(mode):
    """the reference's null effect there is silent: wet(target) takes the echo, the device's lines take nothing"""
    oalgpu, L = _need()
    chain = {0: [st.RefEffect(L, st.KIND_ECHO, st.ECHO_A)]}
    api = st.api_for(mode)
    plain = st.build_scene(api, 3)
    outs = _run_chain(mode, L, 3, [1, -1, -1], chain)         # (wet(1) against the composition)
    added = False
    for k, n in enumerate(SIZES):
        plain.mix(n, post_process=True)
        assert np.array_equal(bits(outs[k][0]), bits(plain.dry()[:, :n])), k
        added = added or not np.array_equal(bits(outs[k][1][1]), bits(plain.wet(1)[:, :n]))
    assert added
    plain.close()


def test_the_target_set_back_to_the_device():
    """three updates with echo -> equalizer, then the target back to -1 and fresh effects: the following updates are those of
    a copy that never had a target"""
    oalgpu, L = _need()
    mode = "fast"
    api = st.api_for(mode)

    def fresh():
        return {0: [st.RefEffect(L, st.KIND_ECHO, st.ECHO_A)], 1: [st.RefEffect(L, st.KIND_EQ, st.EQ_A)]}

    chained, never = st.build_scene(api, 3), st.build_scene(api, 3)
    states = [fresh(), fresh(), fresh(), fresh()]
    made = st.install(chained, mode, [1, -1, -1], states[0]) + st.install(never, mode, [-1, -1, -1], states[1])
    differed = False
    for k, n in enumerate(SIZES):
        if k == 3:
            chained.set_slot_target(0, None)
            assert chained.slot_target(0) == -1
            made += st.install(chained, mode, [-1, -1, -1], states[2]) + st.install(never, mode, [-1, -1, -1], states[3])
        chained.mix(n, post_process=True)
        never.mix(n, post_process=True)
        same = np.array_equal(bits(chained.dry()[:, :n]), bits(never.dry()[:, :n]))
        assert same or k < 3, k
        differed = differed or not same
        if k >= 3:
            for s in range(3):
                assert np.array_equal(bits(chained.wet(s)[:, :n]), bits(never.wet(s)[:, :n])), (k, s)
    assert differed, "with the target the first three updates are others"
    for sc in (chained, never):
        sc.set_slot_effect(0, None); sc.set_slot_effect(1, None)
        sc.close()
    st.close_all(made, [x for d in states for s in d.values() for x in s])
