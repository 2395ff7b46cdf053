"""The stereo TSME encoder's reference side: the compiled reference's own TsmeEncoderIIR / TsmeEncoder<256> / TsmeEncoder<512>
(core/tsmefilter.cpp in oracle/_ref/liboalref.so, called through their C++ symbols exactly as tests/uhj_cases.py calls the UHJ
encoders), float32 / float64 restatements of the two forms, and the TSME device scene the GPU tests run.

An encoder object is a zeroed, 64-byte-aligned block (the constructors are inline, every member's default is zero and encode
does not read the vptr).  encode(std::span<float> L, std::span<float> R, std::span<const std::span<const float>> in) takes each
span by value as (pointer, size); the input-span array holds FOUR spans in the order W, Y, Z, X (ACN).  Every call runs between
FPUCtl::Set and FPUCtl::Reset so that the reference flushes denormals as the GPU does."""
import ctypes as C

import numpy as np

import oracle_lib as ol
import uhj_cases as uc
from uhj_cases import F1, F2, F32, Span, _allpass, _ftz, _span, fir_taps

_TAIL = "6encodeESt4spanIfLm18446744073709551615EES{0}_S{1}_IKS{1}_IKfLm18446744073709551615EELm18446744073709551615EE"
ENCODE = {0: "_ZN14TsmeEncoderIIR" + _TAIL.format(1, 0),
          1: "_ZN11TsmeEncoderILm256EE" + _TAIL.format(2, 1),
          2: "_ZN11TsmeEncoderILm512EE" + _TAIL.format(2, 1)}
GET_DELAY = {0: "_ZN14TsmeEncoderIIR8getDelayEv", 1: "_ZN11TsmeEncoderILm256EE8getDelayEv",
             2: "_ZN11TsmeEncoderILm512EE8getDelayEv"}
_OBJ_BYTES = 128 * 1024

# The worst |float64 direct-FIR restatement - reference| / line max that tests/test_tsme_host.py measures over its ragged run
# (the rounding of the reference's own float32 FFT path): FIR-256 1.453e-7, FIR-512 1.330e-7.  The GPU tests' bound is ten
# times the larger of the two: 1.453e-6.
FIR_RESTATEMENT_RATIO = 1.453e-7
FIR_GPU_BOUND = 10.0 * FIR_RESTATEMENT_RATIO


def available():
    if not ol.available("ref"):
        return False
    L = _ref()
    return all(hasattr(L, s) for s in list(ENCODE.values()) + list(GET_DELAY.values()) + [uc._FPU_SET, uc._FPU_RESET])


def _ref():
    return ol.load("ref").L


def ref_delay(quality):
    """TsmeEncoder*::getDelay of the reference (it reads no member: called on a zeroed object)."""
    f = getattr(_ref(), GET_DELAY[quality])
    f.argtypes = [C.c_void_p]
    f.restype = C.c_size_t
    return int(f(RefTsmeEncoder(quality).ptr))


class RefTsmeEncoder:
    """One reference encoder of `quality` (0 IIR, 1 FIR-256, 2 FIR-512) with fresh state."""

    def __init__(self, quality):
        L = _ref()
        self._encode = getattr(L, ENCODE[quality])
        self._encode.argtypes = [C.c_void_p, Span, Span, Span]
        self._encode.restype = None
        self._set = getattr(L, uc._FPU_SET)
        self._set.argtypes = []
        self._set.restype = C.c_uint
        self._reset = getattr(L, uc._FPU_RESET)
        self._reset.argtypes = [C.c_uint]
        self._reset.restype = None
        raw = np.zeros(_OBJ_BYTES + 64, np.uint8)
        off = (-raw.ctypes.data) % 64
        self._raw = raw
        self.mem = raw[off:off + _OBJ_BYTES]
        self.ptr = self.mem.ctypes.data

    def encode(self, w, y, z, x, left, right):
        """encode of len(w) samples: returns the new (left, right); the inputs are not changed."""
        n = len(w)
        ins = [np.ascontiguousarray(a[:n], np.float32).copy() for a in (w, y, z, x)]
        lo = np.ascontiguousarray(left[:n], np.float32).copy()
        ro = np.ascontiguousarray(right[:n], np.float32).copy()
        spans = (Span * 4)(*[_span(a, n) for a in ins])
        state = self._set()
        try:
            self._encode(self.ptr, _span(lo, n), _span(ro, n), Span(C.addressof(spans), 4))
        finally:
            self._reset(state)
        return lo, ro


# ---- restatements ----

class IirRestated:
    """TsmeEncoderIIR::encode, serially in float32: five cascades (S, WX, Y, L, R) side by side."""

    def __init__(self):
        self.state = np.zeros((5, 4, 2), np.float32)
        self.coeffs = np.stack([F1, F2, F1, F1, F1], axis=1)        # [section][cascade]
        self.carry = np.zeros(4, np.float32)                         # mDelayWXZ, mDelayY, mDirectDelay[0], [1]

    def encode(self, w, y, z, x, left, right):
        n = len(w)
        w, y, z, x = (np.asarray(a[:n], np.float32) for a in (w, y, z, x))
        with np.errstate(under="ignore"):
            s = _ftz(_ftz(_ftz(F32(0.288397341271) * w) + _ftz(F32(0.166565447888) * x)) + _ftz(F32(0.187684284734) * z))
            wx = _ftz(_ftz(F32(0.444008050325) * w) - _ftz(F32(0.256439256487) * x))
            inp = np.stack([s, wx, y, np.asarray(left[:n], np.float32), np.asarray(right[:n], np.float32)], axis=1)
            out = np.zeros_like(inp)
            for i in range(n):
                out[i] = _allpass(self.state, self.coeffs, _ftz(inp[i]))
            sd = np.concatenate([[self.carry[0]], out[:-1, 0]]).astype(np.float32)
            yd = np.concatenate([[self.carry[1]], out[:-1, 2]]).astype(np.float32)
            ld = np.concatenate([[self.carry[2]], out[:-1, 3]]).astype(np.float32)
            rd = np.concatenate([[self.carry[3]], out[:-1, 4]]).astype(np.float32)
            self.carry = out[-1, [0, 2, 3, 4]].copy()
            d = _ftz(out[:, 1] + _ftz(F32(0.333238912931) * yd))
            return _ftz(_ftz(sd + d) + ld), _ftz(_ftz(sd - d) + rd)


class FirRestated:
    """TsmeEncoder<N>::encode as a direct FIR in float64: jwx[t] = sum_k h[k] wx[t - 128 - k]; S, Y and the direct lines
    delayed by d = N/2 + 128."""

    def __init__(self, n):
        self.h = fir_taps(n)
        self.d = n // 2 + 128
        self.hist = np.zeros(n + 127)
        self.dl = np.zeros((4, self.d))

    def encode(self, w, y, z, x, left, right):
        n = len(w)
        w, y, z, x, lf, rf = (np.asarray(a[:n], np.float64) for a in (w, y, z, x, left, right))
        wx = np.concatenate([self.hist, 0.444008050325 * w + -0.256439256487 * x])
        full = np.convolve(wx, self.h)                 # full[j] = sum_k h[k] wx[j - k]
        H = len(self.hist)
        jwx = full[H - 128 + np.arange(n)]
        s = 0.288397341271 * w + 0.166565447888 * x + 0.187684284734 * z
        ext = np.concatenate([self.dl, np.stack([s, y, lf, rf])], axis=1)
        sd, yd, ld, rd = ext[:, :n]
        self.hist = wx[n:]
        self.dl = ext[:, n:]
        dd = jwx + 0.333238912931 * yd
        return ld + (sd + dd), rd + (sd - dd)


def restated(quality):
    return IirRestated() if quality == 0 else FirRestated(256 if quality == 1 else 512)


# ---- the TSME device scene ----

NVOICES = 8


def build_scene(api, seed=1, dedicated=False, max_voices=NVOICES, level=1.0):
    """A stereo TSME device as InitTsmePanning sets it up: 4 dry lines (W, Y, Z, X: AmbiMap {0, 1, 2, 3}, scale 1), 2 real
    lines, voices panned over the sphere (elevations from -50 to +55 degrees, so Z carries signal) with
    oalgpu_voice_set_pan.  dedicated: one send into slot 0, whose dedicated effect feeds the real lines 4-5 (the direct input
    the encoder delays and adds to).  Returns (scene, effect or None, per-update hook)."""
    import oalgpu
    rng = np.random.default_rng(seed)
    sc = api.make_scene(num_dry=4, num_real=2, num_sends=1 if dedicated else 0, num_slots=1 if dedicated else 0,
                        wet_channels=4, hrtf=False, max_voices=max_voices)
    sc.set_ambi_map(np.array([0, 1, 2, 3], np.uint8), np.ones(4, np.float32))
    buf = sc.add_buffer(rng.uniform(-1, 1, 9000).astype(np.float32), ol.FMT_FLOAT, loop_start=0, loop_end=9000)
    fx = None
    if dedicated:
        fx = oalgpu.Effect(oalgpu.EFFECT_DEDICATED, 6, 4, 48000, api.mode)
        gains = np.zeros(6, np.float32)
        gains[4], gains[5] = 0.7, -0.45                      # lines 4-5 of the bus block: the real lines
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
            el = np.radians(-50.0 + 15.0 * v)
            d = [float(np.sin(az) * np.cos(el)), float(np.sin(el)), float(-np.cos(az) * np.cos(el))]
            snd = [(0, np.zeros(4, np.float32), None)] if dedicated else []
            sc.set_params(v, ol.make_voice_params([60211, 48000, 71000][v % 3], ol.RS_BSINC24, dry_gains=np.zeros(4),
                                                  direct_filter=ol.default_filter(active=v % 2, gain_hf=0.6), sends=snd))
            voices.append(v)
            pans.append(d + [0.0, level * (0.25 + 0.05 * v)] + [0.3 + 0.05 * v] + [0.0] * 5)
        sc.set_pan(voices, pans)

    return sc, fx, update
