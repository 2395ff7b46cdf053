"""Scenes and the expected result of effect slot targets (oalgpu_slot_set_target, include/oalgpu.h; GetEffectTarget and the slot
sort of ProcessContexts, alc/alu.cpp:627-632 and :2209-2257), shared by tests/test_gpu_slot_targets.py and
tests/test_gpu_slot_target_rules.py.

A scene is built twice: one copy with the chain, one without effects.  The kernels are deterministic, so the copy without
effects gives the chained copy's voices-only dry block and wet buses, bit for bit.  The expected result is composed from them
on the host in the documented order, with the compiled reference's effect states: by descending depth; within one depth the
convolutions and effects by ascending slot index (a slot's convolution before its effect), then the depth's EAX reverbs by
ascending slot index; each state reads its slot's wet block and adds into its target's wet block, or into the dry lines."""
import ctypes as C

import numpy as np

import oracle_lib as ol
from crossfeed_cases import SIZES            # (1024, 17, 47, 128, 129, 1000, 1, 1024): ragged updates

f32p = C.POINTER(C.c_float)
NUM_DRY, NUM_REAL, WET, RATE = 4, 2, 4, 48000
LINE = 1024

# property sets of the kinds that are bit-identical to the reference (tests/test_effects.py)
EQ_A = [200.0, 2.0, 500.0, 0.5, 1.0, 3000.0, 3.0, 0.7, 6000.0, 0.3]
EQ_B = [100.0, 0.2, 800.0, 4.0, 0.3, 5000.0, 0.4, 1.0, 9000.0, 5.0]
ECHO_A = [0.004, 0.002, 0.2, 0.8, 0.5]              # taps inside the first update
ECHO_B = [0.01, 0.003, 0.5, 0.5, -1.0]
MOD_SQUARE = [30.0, 2000.0, 2]                      # square carrier: no sinf
MOD_SAW = [1000.0, 200.0, 1]
COMP_ON = [1]
KIND_EQ, KIND_MOD, KIND_ECHO, KIND_COMP = 0, 1, 2, 4


def fp(a):
    return a.ctypes.data_as(f32p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def reference():
    """the compiled reference with the effect entry points tests/test_effects.py drives, or None"""
    if not ol.available("ref"):
        return None
    L = ol.load("ref")
    L.L.oal_set_simd(1)
    R = L.L
    R.oal_effect_create.restype = C.c_void_p
    R.oal_effect_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    R.oal_effect_update.argtypes = [C.c_void_p, f32p, C.c_float]
    R.oal_effect_process.argtypes = [C.c_void_p, f32p, f32p, C.c_uint32]
    R.oal_effect_destroy.argtypes = [C.c_void_p]
    return L


def api_for(mode, flags=0):
    import oalgpu
    return oalgpu.Api(oalgpu.MATH_EXACT if mode == "exact" else oalgpu.MATH_FAST, ctx_flags=flags)


def check_kernel(scene, mode):
    """which voice kernel ran (tests/test_gpu_crossfeed.py::_check_kernel): EXACT the serial one, FAST a wavefront kernel"""
    name = scene.voice_kernel_name()
    if mode == "exact":
        assert name == "VoiceMixKernel<true, LINES>", name
    else:
        assert name and not name.startswith("VoiceMixKernel"), name


def build_scene(lib, num_slots, hrtf=False, nvoices=5, product=True, num_dry=NUM_DRY, flags=None):
    """4-6 looping voices, each with dry gains and sends into two slots (voice v: slots v % S and (v + 1) % S)"""
    kw = dict(max_voices=8) if product else {}
    if product and flags is not None:
        kw["flags"] = flags
    sc = lib.make_scene(sample_rate=RATE, num_dry=num_dry, num_real=NUM_REAL, num_sends=2, num_slots=num_slots,
                        wet_channels=WET, hrtf=hrtf, **kw)
    if hrtf:
        cc = np.zeros((num_dry, 128, 2), np.float32)
        cc[:, :64] = np.random.default_rng(5).uniform(-0.2, 0.2, (num_dry, 64, 2))
        sc.set_direct_hrtf(cc, [1.0, 0.8, 0.8, 0.8][:num_dry], 400.0 / RATE, 64)
    buf = sc.add_buffer(np.random.default_rng(6).uniform(-1, 1, 6000).astype(np.float32), ol.FMT_FLOAT)
    for v in range(nvoices):
        sc.add_voice(buf, True, position=v * 700)
        r = np.random.default_rng(50 + v)
        sends = [(v % num_slots, r.uniform(0.1, 0.4, WET), None), ((v + 1) % num_slots, r.uniform(0.05, 0.3, WET), None)]
        if hrtf:
            p = ol.make_voice_params(60211, ol.RS_BSINC24, hrtf=(0.2 * v, 0.9 * v, 2.0, 0.0, 0.1), sends=sends)
        else:
            p = ol.make_voice_params(60211 + 977 * v, ol.RS_BSINC24 if v % 2 else ol.RS_LINEAR,
                                     dry_gains=r.uniform(0.0, 0.2, num_dry), sends=sends)
        sc.set_params(v, p)
    return sc


def effect_gains(L, kind, props, slot_gain, nlines):
    """what the reference's update() resolves against identity AmbiMaps (tests/test_effects.py::targets_for)"""
    if kind in (KIND_EQ, KIND_MOD, KIND_COMP):
        return np.arange(4, dtype=np.uint32), np.full(4, slot_gain, np.float32)
    assert kind == KIND_ECHO
    x = np.float32(props[4])
    z = np.float32(np.sqrt(np.float32(1.0) - x * x))
    g = np.zeros((2, nlines), np.float32)
    for tap, sx in enumerate((x, -x)):
        coeffs = L.direction_coeffs([-sx, 0.0, -z])
        g[tap] = (np.float32(1.0) * coeffs[:nlines]) * np.float32(slot_gain)
    return None, g


class RefEffect:
    """the reference's EffectState of one of the small kinds: process(wet[4][1024], out[nlines][1024], n) adds into out"""
    what = "effect"

    def __init__(self, L, kind, props, gain=1.0, nlines=WET):
        self.L, self.kind, self.props, self.gain, self.nlines = L, kind, props, gain, nlines
        self.h = L.L.oal_effect_create(kind, RATE, nlines, 0, -1)
        assert self.h
        L.L.oal_effect_update(self.h, fp(np.asarray(props, np.float32)), gain)

    def process(self, wet, out, n):
        self.L.L.oal_effect_process(self.h, fp(wet), fp(out), n)

    def product(self, mode):
        """the oalgpu_effect with the same properties"""
        import oalgpu
        fx = oalgpu.Effect(self.kind, self.nlines, 4, RATE, oalgpu.MATH_EXACT if mode == "exact" else oalgpu.MATH_FAST)
        tg, gains = effect_gains(self.L, self.kind, self.props, self.gain, self.nlines)
        fx.update(self.props, tg, gains)
        return fx

    def close(self):
        if self.h:
            self.L.L.oal_effect_destroy(self.h)
            self.h = None


class RefReverb:
    what = "reverb"

    def __init__(self, L, props, gain=0.7, nlines=WET):
        self.nlines = nlines
        self.state = L.make_reverb(nlines)
        self.state.update(ol.ReverbProps.make(**props), gain)

    def process(self, wet, out, n):
        self.state.process_n(wet, out, n)

    def product(self, mode):
        """fed the reference's own parameter block, like tests/test_reverb.py::test_gpu_matches_oracle"""
        import oalgpu
        rev = oalgpu.Reverb(self.nlines)
        rev.set_params(self.state.get_params())
        return rev

    def close(self):
        self.state.close()


class RefConv:
    what = "convolution"

    def __init__(self, L, ir, gain=0.8, nlines=WET):
        self.L, self.ir, self.gain, self.nlines = L, ir, gain, nlines
        self.state = L.make_convolution(nlines, ir)
        self.state.update(gain)

    def process(self, wet, out, n):
        self.state.process(wet[0, :n], out)

    def product(self, mode):
        import oalgpu
        conv = oalgpu.Convolution(self.nlines, self.ir)
        conv.set_target_gains(self.L.direction_coeffs([0.0, 0.0, -1.0])[:self.nlines] * np.float32(self.gain))
        return conv

    def close(self):
        self.state.close()


def attach(scene, slot, obj):
    {"effect": scene.set_slot_effect, "reverb": scene.set_slot_reverb, "convolution": scene.set_slot_convolution}[obj_kind(obj)](slot, obj)


def obj_kind(obj):
    import oalgpu
    return "effect" if isinstance(obj, oalgpu.Effect) else ("reverb" if isinstance(obj, oalgpu.Reverb) else "convolution")


def install(scene, mode, targets, chain):
    """chain: {slot: [reference states]}; attaches their product twins and sets the targets; -> the product objects"""
    made = []
    for slot, target in enumerate(targets):
        if target >= 0:
            scene.set_slot_target(slot, target)
    for slot, states in chain.items():
        for st in states:
            obj = st.product(mode)
            attach(scene, slot, obj)
            made.append(obj)
    return made


def compose(targets, chain, dry, wets, n):
    """The documented order over the voices-only `dry` ([lines][1024]) and `wets` (per slot [4][1024]): -> (dry, wets) after
    the effect leg.  The reference states advance by one update."""
    import oalgpu
    dry = np.array(dry, np.float32)
    wets = [np.array(w, np.float32) for w in wets]
    order, depth = oalgpu.slot_order(targets)

    def run(st, slot):
        src = np.ascontiguousarray(wets[slot])
        if targets[slot] >= 0:
            dst = np.ascontiguousarray(wets[targets[slot]][:st.nlines])
            st.process(src, dst, n)
            wets[targets[slot]][:st.nlines] = dst
        else:
            dst = np.ascontiguousarray(dry[:st.nlines])
            st.process(src, dst, n)
            dry[:st.nlines] = dst

    for d in range(int(depth.max()) if len(depth) else 0, -1, -1):
        slots = [int(s) for s in order if depth[s] == d]
        assert slots == sorted(slots)
        for what in (("convolution", "effect"), ("reverb",)):
            for slot in slots:
                for kind in what:
                    for st in chain.get(slot, []):
                        if st.what == kind:
                            run(st, slot)
    return dry, wets


def close_all(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            x.close()
