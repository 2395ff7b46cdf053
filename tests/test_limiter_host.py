"""The output limiter's host side (no GPU): the device-default rule of UpdateDeviceParams (alc/alc.cpp:1724-1775) and
CreateDeviceLimiter (alc.cpp:1079-1090) for every DevFmtType, and the look-ahead Compressor::Create derives, against the
number of leading zeros the compiled reference's Compressor puts out."""
import ctypes as C
import ctypes.util
import math

import numpy as np
import pytest

import limiter_cases as lc

LIBM = C.CDLL(ctypes.util.find_library("m"))
LIBM.log10f.argtypes = [C.c_float]
LIBM.log10f.restype = C.c_float
F32 = np.float32
DEPTHS = {0: 128.0, 1: 128.0, 2: 32768.0, 3: 32768.0, 4: 8388608.0, 5: 8388608.0, 6: 8388608.0}


def expected_threshold_db(fmt, dither):
    thr = {0: F32(127.0) / F32(128.0), 1: F32(127.0) / F32(128.0), 2: F32(32767.0) / F32(32768.0),
           3: F32(32767.0) / F32(32768.0)}.get(fmt, F32(1.0))
    if dither > 0.0:
        thr = F32(thr - F32(1.0) / F32(dither))
    return F32(F32(LIBM.log10f(float(thr))) * F32(20.0))


@pytest.mark.parametrize("fmt", range(7))
@pytest.mark.parametrize("dithered", [False, True])
def test_device_default_rule(fmt, dithered):
    import oalgpu
    depth = DEPTHS[fmt] if dithered else 0.0
    on, p = oalgpu.limiter_device_params(48000, fmt, depth)
    assert on == (fmt != oalgpu.OUT_F32)              # on by default for every integer format, off for float
    assert p.num_channels == 0 and p.sample_rate == 48000.0
    assert p.auto_flags == 0x1f                       # AutoKnee .. AutoDeclip
    assert (p.look_ahead_time, p.hold_time) == (F32(0.001), F32(0.002))
    assert (p.pre_gain_db, p.post_gain_db, p.knee_db) == (0.0, 0.0, 0.0)
    assert math.isinf(p.ratio) and p.ratio > 0
    assert (p.attack_time, p.release_time) == (F32(0.02), F32(0.2))
    want = expected_threshold_db(fmt, depth)
    assert F32(p.threshold_db) == want, (fmt, depth, p.threshold_db, want)
    if fmt == oalgpu.OUT_I16 and not dithered:
        assert abs(p.threshold_db - 20.0 * math.log10(32767.0 / 32768.0)) < 1e-6
    if fmt in (4, 5, 6) and not dithered:
        assert p.threshold_db == 0.0


def test_bad_arguments_are_refused():
    import oalgpu
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.limiter_device_params(48000, 7, 0.0)
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.limiter_device_params(0, 2, 0.0)
    with pytest.raises(oalgpu.OalgpuError):
        oalgpu.limiter_device_params(48000, 2, -1.0)
    _, p = oalgpu.limiter_device_params(48000, 2, 0.0)
    p.sample_rate = 0.0
    assert oalgpu.limiter_look_ahead(p) == 0


@pytest.mark.parametrize("rate", [22050, 44100, 48000, 96000, 192000])
def test_look_ahead_is_the_reference_delay(rate):
    import oalgpu
    if not lc.available():
        pytest.skip("needs the compiled reference")
    _, p = oalgpu.limiter_device_params(rate, oalgpu.OUT_I16, 0.0)
    la = oalgpu.limiter_look_ahead(p)
    assert la == min(1023, int(np.round(F32(0.001) * F32(rate))))
    for name in ("device default", "no look-ahead"):
        q = lc.limiter_params(rate, name)
        comp = lc.RefCompressor(q, 2)
        x = np.full((2, 1024), 0.25, np.float32)
        out = comp.process(x, 1024)
        comp.close()
        lead = int(np.argmax(out[0] != 0.0))
        assert lead == oalgpu.limiter_look_ahead(q), (rate, name, lead)
        assert np.all(out[:, :lead] == 0.0) and out[0, lead] != 0.0
