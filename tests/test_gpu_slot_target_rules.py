"""What oalgpu_slot_set_target and the three oalgpu_slot_set_* calls refuse and accept (include/oalgpu.h): every refusal returns
OALGPU_ERR_INVALID, leaves oalgpu_slot_target as it was, and leaves the updates around it bit for bit those of a twin scene
that never made the refused calls.  No reference is needed: the scenes are compared with each other."""
import ctypes as C

import numpy as np
import pytest

import slot_target_cases as st
from slot_target_cases import SIZES, bits

pytestmark = pytest.mark.gpu
NUM_DRY = 6                 # more device lines (6 dry + 2 real) than a wet bus has (4): objects that fit one and not the other
SLOTS = 4
ERR_INVALID = -2


def _gpu():
    import oalgpu
    assert oalgpu.device_count() > 0, "GPU tests need a HIP device"
    return oalgpu


def _scene(api):
    return st.build_scene(api, SLOTS, num_dry=NUM_DRY)


def _equalizer(oalgpu, nlines, gain=1.0):
    fx = oalgpu.Effect(st.KIND_EQ, nlines, 4, st.RATE, oalgpu.MATH_FAST)
    fx.update(st.EQ_A, np.arange(4, dtype=np.uint32), np.full(4, gain, np.float32))
    return fx


def _echo(oalgpu, nlines):
    fx = oalgpu.Effect(st.KIND_ECHO, nlines, 4, st.RATE, oalgpu.MATH_FAST)
    g = np.zeros((2, nlines), np.float32)
    g[0, :4] = (0.5, 0.2, 0.0, 0.3)
    g[1, :4] = (0.5, -0.2, 0.0, 0.3)
    fx.update(st.ECHO_A, None, g)
    return fx


def _reverb(oalgpu, nlines):
    rev = oalgpu.Reverb(nlines)
    rev.update(oalgpu.ReverbProps.make(decay_time=0.8), 0.6)
    return rev


def _conv(oalgpu, nlines):
    ir = (np.random.default_rng(3).standard_normal(200) * 0.05).astype(np.float32)
    conv = oalgpu.Convolution(nlines, ir)
    conv.set_target_gains(np.linspace(0.5, 0.1, nlines).astype(np.float32))
    return conv


def _refused(oalgpu, call, *args):
    with pytest.raises(oalgpu.OalgpuError, match=rf"\({ERR_INVALID}\)"):
        call(*args)


def _targets(scene):
    return [scene.slot_target(s) for s in range(SLOTS)]


def _same(a, b, n, k):
    assert np.array_equal(bits(a.dry()[:, :n]), bits(b.dry()[:, :n])), k
    for s in range(SLOTS):
        assert np.array_equal(bits(a.wet(s)[:, :n]), bits(b.wet(s)[:, :n])), (k, s)


def test_refused_targets_change_nothing():
    """a null context, slots and targets out of range, a self-target, cycles of two, three and four slots: between the updates
    of a chained scene, against its twin"""
    oalgpu = _gpu()
    api = st.api_for("fast")
    scene, twin = _scene(api), _scene(api)
    made = []
    for sc in (scene, twin):
        fx = [_echo(oalgpu, 4), _equalizer(oalgpu, 4), _equalizer(oalgpu, 4, 0.5)]
        sc.set_slot_target(0, 1)
        sc.set_slot_target(1, 2)
        for slot, f in enumerate(fx):
            sc.set_slot_effect(slot, f)
        made += fx
    lib = oalgpu.lib
    lib.oalgpu_slot_set_target.argtypes = [C.c_void_p, C.c_uint32, C.c_int32]
    lib.oalgpu_slot_target.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)]
    refusals = [
        lambda: _refused(oalgpu, scene.set_slot_target, SLOTS, 0),              # slot out of range
        lambda: _refused(oalgpu, scene.set_slot_target, 0xffffffff, 0),
        lambda: _refused(oalgpu, scene.set_slot_target, 0, SLOTS),              # target out of range
        lambda: _refused(oalgpu, scene.set_slot_target, 0, -2),
        lambda: _refused(oalgpu, scene.set_slot_target, 3, 3),                  # itself
        lambda: _refused(oalgpu, scene.set_slot_target, 0, 0),
        lambda: _refused(oalgpu, scene.set_slot_target, 1, 0),                  # 0 -> 1 -> 0
        lambda: _refused(oalgpu, scene.set_slot_target, 2, 0),                  # 0 -> 1 -> 2 -> 0
        lambda: _refused(oalgpu, scene.set_slot_target, 2, 1),                  # 1 -> 2 -> 1
        lambda: _refused(oalgpu, scene.slot_target, SLOTS),
    ]
    before = _targets(scene)
    assert before == [1, 2, -1, -1]
    for k, n in enumerate(SIZES):
        if k in (1, 4):
            assert lib.oalgpu_slot_set_target(None, 0, 1) == ERR_INVALID
            assert lib.oalgpu_slot_target(None, 0, C.byref(C.c_int32(7))) == ERR_INVALID
            assert lib.oalgpu_slot_target(scene.h, 0, None) == ERR_INVALID
            for r in refusals:
                r()
                assert _targets(scene) == before
        if k == 5:              # the chain as long as the slots, and the cycle that would close it
            for sc in (scene, twin):
                sc.set_slot_target(2, 3)
            _refused(oalgpu, scene.set_slot_target, 3, 0)
            before = [1, 2, 3, -1]
            assert _targets(scene) == before
        scene.mix(n, post_process=True)
        twin.mix(n, post_process=True)
        _same(scene, twin, n, k)
    assert np.abs(scene.dry()).max() > 1e-3
    for sc in (scene, twin):
        for s in range(SLOTS):
            sc.set_slot_effect(s, None)
        sc.close()
    st.close_all(made)


def test_fit_rule_target_first_then_the_object():
    """on a slot that has a target the three setters measure against wet_channels; on a slot without one against the device's
    lines, as before"""
    oalgpu = _gpu()
    api = st.api_for("fast")
    scene, twin = _scene(api), _scene(api)
    wide_fx, fit_fx, twin_fx = _equalizer(oalgpu, NUM_DRY + st.NUM_REAL), _equalizer(oalgpu, st.WET), _equalizer(oalgpu, st.WET)
    wide_rev, wide_conv = _reverb(oalgpu, 5), _conv(oalgpu, 5)
    scene.set_slot_target(0, 1)
    twin.set_slot_target(0, 1)
    scene.set_slot_effect(0, fit_fx)                # exactly wet_channels lines: accepted
    twin.set_slot_effect(0, twin_fx)
    for k, n in enumerate(SIZES[:4]):
        if k == 2:
            _refused(oalgpu, scene.set_slot_effect, 0, wide_fx)
            _refused(oalgpu, scene.set_slot_reverb, 0, wide_rev)
            _refused(oalgpu, scene.set_slot_convolution, 0, wide_conv)
            assert _targets(scene) == [1, -1, -1, -1]
        scene.mix(n, post_process=True)
        twin.mix(n, post_process=True)
        _same(scene, twin, n, k)
    # the same objects on a slot without a target fit the device's lines
    scene.set_slot_effect(2, wide_fx)
    scene.set_slot_reverb(2, wide_rev)
    scene.set_slot_convolution(3, wide_conv)
    scene.mix(1024, post_process=True)
    assert np.isfinite(scene.dry()).all()
    for s in range(SLOTS):
        scene.set_slot_effect(s, None); scene.set_slot_reverb(s, None); scene.set_slot_convolution(s, None)
    twin.set_slot_effect(0, None)
    scene.close(); twin.close()
    st.close_all(wide_fx, fit_fx, twin_fx, wide_rev, wide_conv)


@pytest.mark.parametrize("what", ["effect", "reverb", "convolution"])
def test_fit_rule_object_first_then_the_target(what):
    """an attached object with more output lines than a wet bus has: the target is refused, the slot keeps feeding the device"""
    oalgpu = _gpu()
    api = st.api_for("fast")
    scene, twin = _scene(api), _scene(api)
    make = {"effect": lambda: _equalizer(oalgpu, NUM_DRY + st.NUM_REAL), "reverb": lambda: _reverb(oalgpu, 5),
            "convolution": lambda: _conv(oalgpu, 5)}[what]
    objs = [make(), make()]
    for sc, obj in zip((scene, twin), objs):
        st.attach(sc, 0, obj)
    for k, n in enumerate(SIZES[:4]):
        if k == 2:
            _refused(oalgpu, scene.set_slot_target, 0, 1)
            assert _targets(scene) == [-1, -1, -1, -1]
        scene.mix(n, post_process=True)
        twin.mix(n, post_process=True)
        _same(scene, twin, n, k)
    # without the object the target is accepted, and the object is then refused from its own side
    for s in range(SLOTS):
        scene.set_slot_effect(s, None); scene.set_slot_reverb(s, None); scene.set_slot_convolution(s, None)
    scene.set_slot_target(0, 1)
    with pytest.raises(oalgpu.OalgpuError):
        st.attach(scene, 0, objs[0])
    for s in range(SLOTS):
        twin.set_slot_effect(s, None); twin.set_slot_reverb(s, None); twin.set_slot_convolution(s, None)
    scene.close(); twin.close()
    st.close_all(objs)


def test_accepted_limits():
    """a chain through every slot with effects of exactly wet_channels lines, re-targeted between updates"""
    oalgpu = _gpu()
    api = st.api_for("exact")
    scene, plain = _scene(api), _scene(api)
    fx = [_echo(oalgpu, st.WET) if s == 0 else _equalizer(oalgpu, st.WET, 0.9) for s in range(SLOTS)]
    for s in range(SLOTS - 1):
        scene.set_slot_target(s, s + 1)
    for s in range(SLOTS):
        scene.set_slot_effect(s, fx[s])
    assert _targets(scene) == [1, 2, 3, -1]
    for k, n in enumerate(SIZES[:5]):
        if k == 3:              # turned round: 3 -> 2 -> 1 -> 0 -> device, one link at a time (no step closes a cycle)
            for s in range(SLOTS):
                scene.set_slot_target(s, None)
            for s in range(1, SLOTS):
                scene.set_slot_target(s, s - 1)
            assert _targets(scene) == [-1, 0, 1, 2]
        scene.mix(n, post_process=True)
        plain.mix(n, post_process=True)
        # only the last slot of the chain reaches the device's lines, every wet bus on the way has taken its feeder's output
        assert not np.array_equal(bits(scene.dry()[:, :n]), bits(plain.dry()[:, :n])), k
        head = 0 if k < 3 else SLOTS - 1
        assert np.array_equal(bits(scene.wet(head)[:, :n]), bits(plain.wet(head)[:, :n])), k
    st.check_kernel(scene, "exact")
    for s in range(SLOTS):
        scene.set_slot_effect(s, None)
    scene.close(); plain.close()
    st.close_all(fx)
