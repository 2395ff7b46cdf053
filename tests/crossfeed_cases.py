"""The bs2b crossfeed's reference side: the compiled reference's own Bs2b::bs2b_processor (core/bs2b.cpp in
oracle/_ref/liboalref.so, called through its C++ symbols), a float32 restatement of cross_feed, and the stereo scenes the GPU
tests run.

A bs2b_processor is 44 bytes, every member zero by default: int level, srate; float a0_lo, b1_lo, a0_hi, a1_hi, b1_hi (offsets
8-24); history[2] of {lo, hi} (offsets 28-40).  set_params(int, int) fills the constants; cross_feed(std::span<float>,
std::span<float>) takes each span by value as (pointer, size) and filters in place.  cross_feed runs between FPUCtl::Set and
FPUCtl::Reset so that the reference flushes denormals as the GPU does.

DeviceBase::Process(Bs2bPostProcess) (alc/alu.cpp:407-434) itself needs a live DeviceBase; what it does around cross_feed is
copy the direct lines out, zero them, decode, and add them back -- one float32 add per sample, numpy here."""
import ctypes as C

import numpy as np

import oracle_lib as ol
from stabilizer_cases import Span, _Ftz, _ftz, _span

F32 = np.float32
_SET_PARAMS = "_ZN4Bs2b14bs2b_processor10set_paramsEii"
_CROSS_FEED = "_ZN4Bs2b14bs2b_processor10cross_feedESt4spanIfLm18446744073709551615EES2_"
_FPU_SET = "_ZN6FPUCtl3SetEv"
_FPU_RESET = "_ZN6FPUCtl5ResetEj"
LEVELS = (1, 2, 3, 4, 5, 6)                      # Bs2b::LowCLevel .. HighECLevel


def available():
    if not ol.available("ref"):
        return False
    L = _ref()
    return all(hasattr(L, s) for s in (_SET_PARAMS, _CROSS_FEED, _FPU_SET, _FPU_RESET))


def _ref():
    return ol.load("ref").L


class RefBs2b:
    """One bs2b_processor of the compiled reference with fresh (zero) history."""

    def __init__(self, level, rate):
        L = _ref()
        self.mem = np.zeros(16, np.float32)                         # 64 bytes: the 44-byte object
        self._cross = getattr(L, _CROSS_FEED)
        self._cross.argtypes = [C.c_void_p, Span, Span]
        self._cross.restype = None
        f = getattr(L, _SET_PARAMS)
        f.argtypes = [C.c_void_p, C.c_int, C.c_int]
        f.restype = None
        f(self.mem.ctypes.data, level, rate)
        assert tuple(self.mem[:2].view(np.int32)) == (level, rate)

    @property
    def constants(self):
        """a0_lo, b1_lo, a0_hi, a1_hi, b1_hi"""
        return self.mem[2:7].copy()

    def cross_feed(self, left, right):
        """-> the filtered (left, right); the inputs are not changed"""
        lo = np.ascontiguousarray(left, np.float32).copy()
        ro = np.ascontiguousarray(right, np.float32).copy()
        with _Ftz():
            self._cross(self.mem.ctypes.data, _span(lo, len(lo)), _span(ro, len(ro)))
        return lo, ro


class Restated:
    """cross_feed serially in float32, every product and sum rounded on its own: four first-order chains"""

    def __init__(self, constants):
        self.k = [F32(v) for v in constants]
        self.z = np.zeros(4, np.float32)                            # history[0].lo, .hi, history[1].lo, .hi

    def cross_feed(self, left, right):
        a0lo, b1lo, a0hi, a1hi, b1hi = self.k
        n = len(left)
        lo, ro = np.zeros(n, np.float32), np.zeros(n, np.float32)
        z = self.z
        with np.errstate(under="ignore"):
            for i in range(n):
                xl, xr = _ftz(left[i]), _ftz(right[i])
                hi_l = _ftz(_ftz(a0hi * xl) + z[1])
                z[1] = _ftz(_ftz(a1hi * xl) + _ftz(b1hi * hi_l))
                lo_l = _ftz(_ftz(a0lo * xl) + z[0])
                z[0] = _ftz(b1lo * lo_l)
                lo_r = _ftz(_ftz(a0lo * xr) + z[2])
                z[2] = _ftz(b1lo * lo_r)
                hi_r = _ftz(_ftz(a0hi * xr) + z[3])
                z[3] = _ftz(_ftz(a1hi * xr) + _ftz(b1hi * hi_r))
                lo[i] = _ftz(hi_l + lo_r)
                ro[i] = _ftz(lo_l + hi_r)
        return lo, ro


def add_direct(filtered, direct):
    """alu.cpp:432-433: one float32 add per sample, flushed as the reference's FPU mode flushes it"""
    with np.errstate(under="ignore"):
        return _ftz(np.asarray(filtered, np.float32) + np.asarray(direct, np.float32))


# ---- the stereo scenes ----

NVOICES = 8
SIZES = (1024, 17, 47, 128, 129, 1000, 1, 1024)

LAYOUTS = {
    # a stereo device over a first-order 2D dry bus (W, Y, X), single-band decoder
    "stereo": dict(num_dry=3, ambi=[0, 1, 3], dual=False),
    # the same over a first-order 3D dry bus (W, Y, Z, X), dual-band decoder
    "stereo dual band": dict(num_dry=4, ambi=[0, 1, 2, 3], dual=True),
}


def decoder_matrices(layout, left=0, right=1):
    """(hf, lf or None): 2 x 25, row `left` the left speaker's"""
    nd = LAYOUTS[layout]["num_dry"]
    hf = np.zeros((2, 25), np.float32)
    if nd == 3:
        hf[left, :3] = (0.5, 0.29, 0.23)          # W, Y, X
        hf[right, :3] = (0.5, -0.29, 0.23)
        return hf, None
    hf[left, :4] = (0.46, 0.31, 0.05, 0.21)       # W, Y, Z, X
    hf[right, :4] = (0.46, -0.31, 0.05, 0.21)
    lf = np.zeros((2, 25), np.float32)
    lf[left, :4] = (0.54, 0.25, 0.03, 0.17)
    lf[right, :4] = (0.54, -0.25, 0.03, 0.17)
    return hf, lf


def build_scene(api, layout="stereo", rate=48000, dedicated=False, dedicated_gains=(0.7, -0.45), max_voices=NVOICES,
                level=1.0):
    """A stereo device of LAYOUTS[layout] at `rate` with eight looping voices panned around the circle by
    oalgpu_voice_set_pan.  dedicated: one send into slot 0, whose dedicated effect feeds the two real lines with
    dedicated_gains (the direct signal the crossfeed keeps out of its filter; zero gains = the slot runs and adds nothing).
    Returns (scene, effect or None, per-update hook)."""
    import oalgpu
    lay = LAYOUTS[layout]
    nd = lay["num_dry"]
    rng = np.random.default_rng(7)
    sc = api.make_scene(sample_rate=rate, num_dry=nd, num_real=2, num_sends=1 if dedicated else 0,
                        num_slots=1 if dedicated else 0, wet_channels=4, hrtf=False, max_voices=max_voices)
    sc.set_ambi_map(np.array(lay["ambi"], np.uint8), np.ones(nd, np.float32))
    buf = sc.add_buffer(rng.uniform(-1, 1, 9000).astype(np.float32), ol.FMT_FLOAT, loop_start=0, loop_end=9000)
    fx = None
    if dedicated:
        fx = oalgpu.Effect(oalgpu.EFFECT_DEDICATED, nd + 2, 4, rate, api.mode)
        gains = np.zeros(nd + 2, np.float32)
        gains[nd:] = dedicated_gains
        fx.update(None, None, gains)
        sc.set_slot_effect(0, fx)
    for v in range(NVOICES):
        sc.add_voice(buf, looping=True, position=(v * 977) % 8000, frac=(v * 4099) % 65536)

    def update(k):
        if k % 3:
            return
        voices, pans = [], []
        for v in range(NVOICES):
            az = 2.0 * np.pi * (v + 0.37 * k) / NVOICES
            el = np.radians(-30.0 + 9.0 * v) if nd == 4 else 0.0
            d = [float(np.sin(az) * np.cos(el)), float(np.sin(el)), float(-np.cos(az) * np.cos(el))]
            snd = [(0, np.zeros(4, np.float32), None)] if dedicated else []
            sc.set_params(v, ol.make_voice_params([60211, 48000, 71000][v % 3], ol.RS_BSINC24, dry_gains=np.zeros(nd),
                                                  direct_filter=ol.default_filter(active=v % 2, gain_hf=0.6), sends=snd))
            voices.append(v)
            pans.append(d + [0.0, level * (0.25 + 0.05 * v)] + [0.3 + 0.05 * v] + [0.0] * 5)
        sc.set_pan(voices, pans)

    return sc, fx, update
