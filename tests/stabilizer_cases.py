"""The front stabilizer's and the distance compensation's reference side, and the speaker scenes their GPU tests run.

Front stabilizer.  DeviceBase::Process(StablizerPostProcess) (alc/alu.cpp:329-405) itself needs a live DeviceBase and cannot be
reached without changing oracle/, so the expected value is composed of the pieces that can be called:
  * the decode is oracle_lib.BFormatDec (the harness's oal_bformatdec_*, the reference's own BFormatDec::process);
  * the filters are the compiled reference's own BandSplitter::init / ::process / ::processAllPass (core/filters/splitter.cpp in
    oracle/_ref/liboalref.so, called through their C++ symbols).  A BandSplitter is four floats (mCoeff, mLpZ1, mLpZ2, mApZ1);
    spans pass by value as (pointer, size) structures; every call runs between FPUCtl::Set and FPUCtl::Reset so that the reference
    flushes denormals as the GPU does;
  * the four pan constants are the host libm's cosf / sinf (the glibc the reference links) of float32 arguments;
  * only the glue of alu.cpp:339-357 and :389-404 -- float32 adds, subtracts and products, one rounding each -- is numpy.

Distance compensation.  ApplyDistanceComp is file-local in alc/alu.cpp and the bridge renders without ChannelDelays, so the
expected value is the statement out[t] = gain * x[t - delay] over the concatenated run (one float32 product per sample, zeros
before the run's start), with a line of delay 0 left alone.  init_distance_comp restates InitDistanceComp
(alc/panning.cpp:301-371) in float32."""
import ctypes as C
import ctypes.util

import numpy as np

import oracle_lib as ol

F32 = np.float32
_INIT = "_ZN12BandSplitter4initEf"
_PROCESS = "_ZN12BandSplitter7processESt4spanIKfLm18446744073709551615EES0_IfLm18446744073709551615EES3_"
_ALLPASS = "_ZN12BandSplitter14processAllPassESt4spanIfLm18446744073709551615EE"
_FPU_SET = "_ZN6FPUCtl3SetEv"
_FPU_RESET = "_ZN6FPUCtl5ResetEj"


def available():
    if not ol.available("ref"):
        return False
    L = _ref()
    return all(hasattr(L, s) for s in (_INIT, _PROCESS, _ALLPASS, _FPU_SET, _FPU_RESET))


def _ref():
    return ol.load("ref").L


class Span(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("size", C.c_size_t)]


def _span(a, n):
    return Span(a.ctypes.data, n)


class _Ftz:
    """FPUCtl::Set ... FPUCtl::Reset around the reference's filters"""

    def __enter__(self):
        L = _ref()
        self._set = getattr(L, _FPU_SET)
        self._set.argtypes = []
        self._set.restype = C.c_uint
        self._reset = getattr(L, _FPU_RESET)
        self._reset.argtypes = [C.c_uint]
        self._reset.restype = None
        self.state = self._set()

    def __exit__(self, *exc):
        self._reset(self.state)


class RefBandSplitter:
    """One BandSplitter of the compiled reference: the object is self.mem (mCoeff, mLpZ1, mLpZ2, mApZ1)."""

    def __init__(self, f0norm=None):
        L = _ref()
        self.mem = np.zeros(4, np.float32)
        self._init = getattr(L, _INIT)
        self._init.argtypes = [C.c_void_p, C.c_float]
        self._init.restype = None
        self._process = getattr(L, _PROCESS)
        self._process.argtypes = [C.c_void_p, Span, Span, Span]
        self._process.restype = None
        self._allpass = getattr(L, _ALLPASS)
        self._allpass.argtypes = [C.c_void_p, Span]
        self._allpass.restype = None
        if f0norm is not None:
            self.init(f0norm)

    def init(self, f0norm):
        self._init(self.mem.ctypes.data, F32(f0norm))

    @property
    def coeff(self):
        return self.mem[0]

    def process(self, x):
        """-> (hp, lp) of x"""
        x = np.ascontiguousarray(x, np.float32)
        hp, lp = np.zeros_like(x), np.zeros_like(x)
        with _Ftz():
            self._process(self.mem.ctypes.data, _span(x, len(x)), _span(hp, len(x)), _span(lp, len(x)))
        return hp, lp

    def all_pass(self, x):
        y = np.ascontiguousarray(x, np.float32).copy()
        with _Ftz():
            self._allpass(self.mem.ctypes.data, _span(y, len(y)))
        return y


def pan_constants():
    """mid_lf, mid_hf, center_lf, center_hf of alu.cpp:384-387: std::cos / std::sin of float arguments = the host libm's cosf / sinf"""
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.cosf.argtypes = m.sinf.argtypes = [C.c_float]
    m.cosf.restype = m.sinf.restype = C.c_float
    half_pi = F32(F32(np.pi) * F32(0.5))
    third = F32(F32(F32(1.0) / F32(3.0)) * half_pi)
    quarter = F32(F32(F32(1.0) / F32(4.0)) * half_pi)
    return F32(m.cosf(third)), F32(m.cosf(quarter)), F32(m.sinf(third)), F32(m.sinf(quarter))


def _ftz(a):
    """the flush of FPUCtl (FTZ / DAZ) and of the GPU, for the glue's results"""
    a = np.asarray(a, np.float32)
    return np.where(np.abs(a) < np.finfo(np.float32).tiny, F32(0.0) * a, a).astype(np.float32)


class RefStabilizer:
    """DeviceBase::Process(StablizerPostProcess) composed as the module's docstring says, with fresh state.
    decode(real, dry, n): accumulates the decoded feeds into real (nreal x 1024) -- oracle_lib.BFormatDec.process, or
    anything else that stands for the decode (the GPU's own decoded feeds, see feeds=)."""

    def __init__(self, nreal, left, right, center, xover_norm):
        self.n, self.l, self.r, self.c = nreal, left, right, center
        self.mid_filter = RefBandSplitter(xover_norm)
        self.chan = [RefBandSplitter(xover_norm) for _ in range(nreal)]
        self.k = pan_constants()

    def process(self, real, n, decode):
        """real: the direct real lines (nreal x >= n) of one update; decode(lines) adds the decoded feeds to the nreal x 1024
        array it is given; -> the stabilized real lines (nreal x n)"""
        out = np.zeros((self.n, 1024), np.float32)
        out[:, :n] = real[:, :n]
        left, right = out[self.l, :n].copy(), out[self.r, :n].copy()
        with np.errstate(under="ignore"):
            mid = _ftz(left + right)
            side = _ftz(left - right)
            out[self.l, :n] = 0.0
            out[self.r, :n] = 0.0
            decode(out)
            left, right = out[self.l, :n].copy(), out[self.r, :n].copy()
            side = _ftz(side + _ftz(left - right))
            tmp = _ftz(left + right)
            mid_hf, mid_lf = self.mid_filter.process(tmp)
            res = np.zeros((self.n, n), np.float32)
            for i in range(self.n):
                if i == self.l:
                    mid = self.chan[i].all_pass(mid)
                elif i == self.r:
                    side = self.chan[i].all_pass(side)
                else:
                    res[i] = self.chan[i].all_pass(out[i, :n])
            k_mid_lf, k_mid_hf, k_center_lf, k_center_hf = self.k
            m = _ftz(_ftz(_ftz(mid_lf * k_mid_lf) + _ftz(mid_hf * k_mid_hf)) + mid)
            c = _ftz(_ftz(mid_lf * k_center_lf) + _ftz(mid_hf * k_center_hf))
            res[self.l] = _ftz(_ftz(m + side) * F32(0.5))
            res[self.r] = _ftz(_ftz(m - side) * F32(0.5))
            res[self.c] = _ftz(res[self.c] + _ftz(c * F32(0.5)))
        return res


# ---- distance compensation ----

MAX_DELAY = 1023                     # DistanceComp::MaxDelay - 1


def init_distance_comp(rate, distances):
    """InitDistanceComp's arithmetic in float32: -> (delays, gains, any non-zero delay)"""
    d = np.asarray(distances, np.float32)
    delays = np.zeros(len(d), np.uint32)
    gains = np.ones(len(d), np.float32)
    maxdist = d.max()
    if not maxdist > 0.0:
        return delays, gains, False
    scale = F32(F32(rate) / F32(343.3))
    for i, dist in enumerate(d):
        delay = np.floor(F32(F32(F32(maxdist - dist) * scale) + F32(0.5)))
        delay = min(delay, F32(MAX_DELAY))
        if dist > 0.0:
            delays[i] = np.uint32(delay)
            gains[i] = F32(dist / maxdist)
    return delays, gains, bool(delays.any())


class DistanceCompExpected:
    """out[t] = gain * x[t - delay] over the concatenated updates, fresh (zero) history; lines beyond len(delays), and lines of
    delay 0, come through untouched"""

    def __init__(self, delays, gains):
        self.delays = [int(d) for d in delays]
        self.gains = np.asarray(gains, np.float32)
        self.hist = [np.zeros(d, np.float32) for d in self.delays]

    def process(self, lines, n):
        out = np.array(lines[:, :n], np.float32)
        for i, d in enumerate(self.delays):
            if d == 0:
                continue
            ext = np.concatenate([self.hist[i], out[i]])
            self.hist[i] = ext[n:].copy()
            with np.errstate(under="ignore"):
                out[i] = _ftz(ext[:n] * self.gains[i])
        return out


# ---- the speaker scenes ----

NVOICES = 8
SIZES = (1024, 17, 47, 128, 129, 1000, 1, 1024)

LAYOUTS = {
    # 7.1: 5 dry lines (second-order 2D: ACN 0, 1, 3, 4, 8), 8 real lines FL FR FC LFE BL BR SL SR, X71Config dual band
    "7.1": dict(num_dry=5, num_real=8, ambi=[0, 1, 3, 4, 8], left=0, right=1, center=2, dual=True),
    # a 4-line layout whose front lines sit at permuted indices (centre 0, right 1, a rear line 2, left 3), single band
    "permuted": dict(num_dry=3, num_real=4, ambi=[0, 1, 3], left=3, right=1, center=0, dual=False),
}


def decoder_matrices(layout):
    """(hf, lf or None): nreal x 25"""
    from oalgpu import synth
    if layout == "7.1":
        return synth.x71_decoder()
    hf = np.zeros((4, 25), np.float32)
    hf[3, :3] = (0.40, 0.33, 0.31)        # left  (W, Y, X)
    hf[1, :3] = (0.40, -0.33, 0.31)       # right
    hf[2, :3] = (0.35, 0.0, -0.45)        # rear
    hf[0, :3] = (0.05, 0.0, 0.08)         # a little of the decode on the centre line itself
    return hf, None


def build_scene(api, layout="7.1", dedicated=False, max_voices=NVOICES, no_real=False, level=1.0):
    """A speaker device of LAYOUTS[layout] with eight looping voices panned around the circle by oalgpu_voice_set_pan.
    dedicated: one send into slot 0, whose dedicated effect feeds the real lines (the direct signal the stabilizer moves out
    of its way).  no_real: the same dry lines and no real lines (the dry lines are the output).
    Returns (scene, effect or None, per-update hook)."""
    import oalgpu
    lay = LAYOUTS[layout]
    nd, nr = lay["num_dry"], 0 if no_real else lay["num_real"]
    rng = np.random.default_rng(5)
    sc = api.make_scene(num_dry=nd, num_real=nr, num_sends=1 if dedicated else 0, num_slots=1 if dedicated else 0,
                        wet_channels=4, hrtf=False, max_voices=max_voices)
    sc.set_ambi_map(np.array(lay["ambi"], np.uint8), np.ones(nd, np.float32))
    buf = sc.add_buffer(rng.uniform(-1, 1, 9000).astype(np.float32), ol.FMT_FLOAT, loop_start=0, loop_end=9000)
    fx = None
    if dedicated:
        fx = oalgpu.Effect(oalgpu.EFFECT_DEDICATED, nd + nr, 4, 48000, api.mode)
        gains = np.zeros(nd + nr, np.float32)
        gains[nd:] = np.array([0.7, -0.45, 0.2, 0.3, 0.15, -0.1, 0.05, 0.25], np.float32)[:nr]
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
            d = [float(np.sin(az)), 0.0, float(-np.cos(az))]
            snd = [(0, np.zeros(4, np.float32), None)] if dedicated else []
            sc.set_params(v, ol.make_voice_params([60211, 48000, 71000][v % 3], ol.RS_BSINC24, dry_gains=np.zeros(nd),
                                                  direct_filter=ol.default_filter(active=v % 2, gain_hf=0.6), sends=snd))
            voices.append(v)
            pans.append(d + [0.0, level * (0.25 + 0.05 * v)] + [0.3 + 0.05 * v] + [0.0] * 5)
        sc.set_pan(voices, pans)

    return sc, fx, update
