"""The stereo UHJ encoder's reference side: the compiled reference's own UhjEncoderIIR / UhjEncoder<256> / UhjEncoder<512>
(core/uhjfilter.cpp in oracle/_ref/liboalref.so, called through their C++ symbols), float32 / float64 restatements of the two
forms, and the UHJ device scenes the GPU tests run.

The encoders' constructors are inline, so an object is a zeroed, 64-byte-aligned block: every member's default is zero and
encode does not read the vptr.  encode(std::span<float> L, std::span<float> R, std::span<const std::span<const float>> in)
takes each span by value as (pointer, size) -- a Structure passed whole (the third one goes on the stack).  Every call runs
between FPUCtl::Set and FPUCtl::Reset so that the reference flushes denormals as the GPU does."""
import ctypes as C

import numpy as np

import oracle_lib as ol

_TAIL = "6encodeESt4spanIfLm18446744073709551615EES{0}_S{1}_IKS{1}_IKfLm18446744073709551615EELm18446744073709551615EE"
ENCODE = {0: "_ZN13UhjEncoderIIR" + _TAIL.format(1, 0),
          1: "_ZN10UhjEncoderILm256EE" + _TAIL.format(2, 1),
          2: "_ZN10UhjEncoderILm512EE" + _TAIL.format(2, 1)}
GET_DELAY = {0: "_ZN13UhjEncoderIIR8getDelayEv", 1: "_ZN10UhjEncoderILm256EE8getDelayEv",
             2: "_ZN10UhjEncoderILm512EE8getDelayEv"}
_FPU_SET = "_ZN6FPUCtl3SetEv"
_FPU_RESET = "_ZN6FPUCtl5ResetEj"
_OBJ_BYTES = 128 * 1024

F1 = np.array([0.479400865589, 0.876218493539, 0.976597589508, 0.997499255936], np.float32)   # Filter1Coeff
F2 = np.array([0.161758498368, 0.733028932341, 0.945349700329, 0.990599156684], np.float32)   # Filter2Coeff
F32 = np.float32


def available():
    if not ol.available("ref"):
        return False
    L = _ref()
    return all(hasattr(L, s) for s in list(ENCODE.values()) + [_FPU_SET, _FPU_RESET])


def _ref():
    return ol.load("ref").L


class Span(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("size", C.c_size_t)]


def _span(a, n):
    return Span(a.ctypes.data, n)


def ref_delay(quality):
    """UhjEncoder*::getDelay of the reference (it reads no member: called on a zeroed object)."""
    f = getattr(_ref(), GET_DELAY[quality])
    f.argtypes = [C.c_void_p]
    f.restype = C.c_size_t
    obj = RefUhjEncoder(quality)
    return int(f(obj.ptr))


class RefUhjEncoder:
    """One reference encoder of `quality` (0 IIR, 1 FIR-256, 2 FIR-512) with fresh state."""

    def __init__(self, quality):
        L = _ref()
        self._encode = getattr(L, ENCODE[quality])
        self._encode.argtypes = [C.c_void_p, Span, Span, Span]
        self._encode.restype = None
        self._set = getattr(L, _FPU_SET)
        self._set.argtypes = []
        self._set.restype = C.c_uint
        self._reset = getattr(L, _FPU_RESET)
        self._reset.argtypes = [C.c_uint]
        self._reset.restype = None
        raw = np.zeros(_OBJ_BYTES + 64, np.uint8)
        off = (-raw.ctypes.data) % 64
        self._raw = raw
        self.mem = raw[off:off + _OBJ_BYTES]
        self.ptr = self.mem.ctypes.data

    def encode(self, w, x, y, left, right):
        """encode of len(w) samples: returns the new (left, right); the inputs are not changed."""
        n = len(w)
        ins = [np.ascontiguousarray(a[:n], np.float32).copy() for a in (w, x, y)]
        lo = np.ascontiguousarray(left[:n], np.float32).copy()
        ro = np.ascontiguousarray(right[:n], np.float32).copy()
        spans = (Span * 3)(*[_span(a, n) for a in ins])
        state = self._set()
        try:
            self._encode(self.ptr, _span(lo, n), _span(ro, n), Span(C.addressof(spans), 3))
        finally:
            self._reset(state)
        return lo, ro


# ---- restatements ----

def _allpass(state, coeffs, x):
    """one sample through four sections (allpass_iir.hpp process), float32; state [..., 4, 2] updated in place"""
    for i in range(4):
        y = _ftz(_ftz(x * coeffs[i]) + state[..., i, 0])
        state[..., i, 0] = state[..., i, 1]
        state[..., i, 1] = _ftz(_ftz(y * coeffs[i]) - x)
        x = y
    return x


class IirRestated:
    """UhjEncoderIIR::encode, serially in float32: five cascades (S, WX, Y, L, R) side by side."""

    def __init__(self):
        self.state = np.zeros((5, 4, 2), np.float32)
        self.coeffs = np.stack([F1, F2, F1, F1, F1], axis=1)        # [section][cascade]
        self.carry = np.zeros(4, np.float32)                         # mDelayWX, mDelayY, mDirectDelay[0], [1]

    def encode(self, w, x, y, left, right):
        n = len(w)
        w, x, y = (np.asarray(a[:n], np.float32) for a in (w, x, y))
        inp = np.stack([F32(0.4698463) * w + F32(0.0757602682546) * x, F32(-0.17101005) * w + F32(0.208149636675) * x,
                        y, np.asarray(left[:n], np.float32), np.asarray(right[:n], np.float32)], axis=1)
        out = np.zeros_like(inp)
        with np.errstate(under="ignore"):
            for i in range(n):
                out[i] = _allpass(self.state, self.coeffs, _ftz(inp[i]))
        s = np.concatenate([[self.carry[0]], out[:-1, 0]]).astype(np.float32)
        yd = np.concatenate([[self.carry[1]], out[:-1, 2]]).astype(np.float32)
        ld = np.concatenate([[self.carry[2]], out[:-1, 3]]).astype(np.float32)
        rd = np.concatenate([[self.carry[3]], out[:-1, 4]]).astype(np.float32)
        self.carry = out[-1, [0, 2, 3, 4]].copy()
        d = out[:, 1] + F32(0.267586995182) * yd
        return (s + d) + ld, (s - d) + rd


def _ftz(a):
    """the flush of FPUCtl (FTZ / DAZ) and of the GPU"""
    return np.where(np.abs(a) < np.finfo(np.float32).tiny, np.float32(0.0), a).astype(np.float32)


def fir_taps(n):
    """SegmentedFilter<n>'s response (allpass_conv.hpp) in double: h[2i+1] for i < n/2, even taps zero."""
    half = n // 2
    h = np.zeros(n)
    for i in range(half):
        k = half - (2 * i + 1)
        w = 2.0 * np.pi / float(half - 1) * float(i)
        win = 0.3635819 - 0.4891775 * np.cos(w) + 0.1365995 * np.cos(2.0 * w) - 0.0106411 * np.cos(3.0 * w)
        h[2 * i + 1] = win * 2.0 / (np.pi * float(k))
    return h


class FirRestated:
    """UhjEncoder<N>::encode as a direct FIR in float64: jwx[t] = sum_k h[k] wx[t - 128 - k]; S, Y and the direct lines
    delayed by d = N/2 + 128."""

    def __init__(self, n):
        self.h = fir_taps(n)
        self.d = n // 2 + 128
        self.hist = np.zeros(n + 127)
        self.dl = np.zeros((4, self.d))

    def encode(self, w, x, y, left, right):
        n = len(w)
        w, x, y, lf, rf = (np.asarray(a[:n], np.float64) for a in (w, x, y, left, right))
        wx = np.concatenate([self.hist, -0.17101005 * w + 0.208149636675 * x])
        full = np.convolve(wx, self.h)                 # full[j] = sum_k h[k] wx[j - k]
        H = len(self.hist)
        jwx = full[H - 128 + np.arange(n)]
        ext = np.concatenate([self.dl, np.stack([0.4698463 * w + 0.0757602682546 * x, y, lf, rf])], axis=1)
        s, yd, ld, rd = ext[:, :n]
        self.hist = wx[n:]
        self.dl = ext[:, n:]
        dd = jwx + 0.267586995182 * yd
        return ld + (s + dd), rd + (s - dd)


def restated(quality):
    return IirRestated() if quality == 0 else FirRestated(256 if quality == 1 else 512)


# ---- the UHJ device scenes ----

NVOICES = 8


def build_scene(api, seed=1, dedicated=False, max_voices=NVOICES):
    """A stereo UHJ device: 3 dry lines (W, X, Y: AmbiMap {0, 3, 1}, scale 1), 2 real lines, voices panned around the
    circle with oalgpu_voice_set_pan.  dedicated: one send into slot 0, whose dedicated effect feeds the real lines 3-4
    (the direct input the encoder delays and adds to).  Returns (scene, effect or None, per-update hook)."""
    import oalgpu
    rng = np.random.default_rng(seed)
    sc = api.make_scene(num_dry=3, num_real=2, num_sends=1 if dedicated else 0, num_slots=1 if dedicated else 0,
                        wet_channels=4, hrtf=False, max_voices=max_voices)
    sc.set_ambi_map(np.array([0, 3, 1], np.uint8), np.ones(3, np.float32))
    buf = sc.add_buffer(rng.uniform(-1, 1, 9000).astype(np.float32), ol.FMT_FLOAT, loop_start=0, loop_end=9000)
    fx = None
    if dedicated:
        fx = oalgpu.Effect(oalgpu.EFFECT_DEDICATED, 5, 4, 48000, api.mode)
        gains = np.zeros(5, np.float32)
        gains[3], gains[4] = 0.7, -0.45                      # lines 3-4 of the bus block: the real lines
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
            sc.set_params(v, ol.make_voice_params([60211, 48000, 71000][v % 3], ol.RS_BSINC24, dry_gains=np.zeros(3),
                                                  direct_filter=ol.default_filter(active=v % 2, gain_hf=0.6), sends=snd))
            voices.append(v)
            pans.append(d + [0.0, 0.25 + 0.05 * v] + [0.3 + 0.05 * v] + [0.0] * 5)
        sc.set_pan(voices, pans)

    return sc, fx, update
