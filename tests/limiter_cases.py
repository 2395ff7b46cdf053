"""The output limiter's reference side: the compiled reference's own Compressor (core/mastering.cpp in oracle/_ref/liboalref.so,
called through its C++ symbols), and the loud scenes the limiter tests run.

Compressor::Params is 48 bytes -- a u32, an f32, the flag bitset as a u32, nine f32 -- the layout of oalgpu_limiter_params
(oalgpu.LimiterParams).  Create returns its unique_ptr through the hidden first argument; process(unsigned,
std::span<FloatBufferLine>) takes the span as (pointer, count) of 1024-float rows."""
import ctypes as C

import numpy as np

import oracle_lib as ol

_CREATE = "_ZN10Compressor6CreateENS_6ParamsE"
_PROCESS = "_ZN10Compressor7processEjSt4spanISt5arrayIfLm1024EELm18446744073709551615EE"
_DTOR = "_ZN10CompressorD1Ev"


def available():
    if not ol.available("ref"):
        return False
    return hasattr(_ref(), _CREATE)


def _ref():
    return ol.load("ref").L


class RefCompressor:
    """One reference Compressor over `nch` lines."""

    def __init__(self, params, nch):
        import oalgpu
        L = _ref()
        self._create = getattr(L, _CREATE)
        self._create.argtypes = [C.POINTER(C.c_void_p), oalgpu.LimiterParams]
        self._create.restype = None
        self._process = getattr(L, _PROCESS)
        self._process.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t]
        self._process.restype = None
        self._dtor = getattr(L, _DTOR)
        self._dtor.argtypes = [C.c_void_p]
        p = oalgpu.LimiterParams.from_buffer_copy(params)
        p.num_channels = nch
        self.nch = nch
        ptr = C.c_void_p()
        self._create(C.byref(ptr), p)
        self.h = ptr
        self.buf = np.zeros((nch, 1024), np.float32)

    def process(self, lines, n):
        """Compressor::process on a copy of lines[:, :n]; returns the limited lines (nch x n)."""
        self.buf[:] = 0.0
        self.buf[:, :n] = lines[:self.nch, :n]
        self._process(self.h, n, self.buf.ctypes.data_as(C.c_void_p), self.nch)
        return self.buf[:, :n].copy()

    def close(self):
        if self.h:
            self._dtor(self.h)          # (the object's storage is left to the process: operator delete is not needed here)
            self.h = None


def loud_buffer(seed, length=24000):
    """Noise bursts with silent gaps, a quiet stretch and isolated clicks shorter than the 2 ms hold."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, length).astype(np.float32)
    env = np.zeros(length, np.float32)
    env[0:2500] = 1.0
    env[2500:4000] = np.linspace(1.0, 0.0, 1500)
    env[9000:12000] = 0.03
    env[15000:16500] = 1.0
    x *= env
    x[7000:7012] = 1.0                  # transients inside the gaps
    x[13500:13520] = -1.0
    x[20000:20005] = 1.0
    return x


class LoudSynth:
    """oalgpu.synth with the scene's source buffers replaced by loud_buffer()s scaled by `scale` (bench.build_scene takes
    the synth module as an argument)."""

    def __init__(self, scale):
        from oalgpu import synth
        self._synth = synth
        self.scale = scale

    def __getattr__(self, name):
        return getattr(self._synth, name)

    def scene_buffers(self, config_id, nvoices, sample_fmt="f32"):
        return [(loud_buffer(s) * np.float32(self.scale)).astype(np.float32) for s in range(4)]


# the parameter sets of the tests: (name, change to the device default)
PARAM_SETS = {
    "device default": {},
    "no hold": {"hold_time": 0.0},
    "no look-ahead": {"look_ahead_time": 0.0},
    "no automation": {"auto_flags": 0, "ratio": 4.0, "knee_db": 6.0, "threshold_db": -6.0, "attack_time": 0.005,
                      "release_time": 0.05},
    "pre-gain": {"pre_gain_db": -3.5},
    "post-gain without declip": {"auto_flags": 1 | 2 | 4 | 8, "post_gain_db": 1.5},
}


def limiter_params(rate, name, sample_type=2, dither_depth=0.0):
    import oalgpu
    _, p = oalgpu.limiter_device_params(rate, sample_type, dither_depth)
    for k, v in PARAM_SETS[name].items():
        setattr(p, k, v)
    return p
