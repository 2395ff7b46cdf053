"""DESIGN.md 3.26's second table: the calling thread's wall clock for 1024 moved mono sources on a near-field context (five dry
lines, channels per order 1, 2, 2, control distance 1.5), two ways:

  * oalgpu_voice_set_source_props: the params kernel, SourceNfcKernel, the two installs, one stream synchronise;
  * the path a host had to take before: oalgpu_voice_set_params with host-built records (oalgpu_source_params_host's, built
    outside the timed region) plus 1024 oalgpu_voice_set_nfc calls (a host-side adjust and a one-workgroup launch each), then
    oalgpu_sync -- the same end state: every voice's parameters and NFC coefficients installed.

Medians of 50 after 5 warm-ups, an update between the calls.  The 1024 calls are made from a Python loop through ctypes; what
that loop costs by itself (1024 calls of oalgpu_version) is measured beside them and reported, not subtracted.

    python tools/measure_nfc_calls.py [out.json]        (needs a GPU; prints one JSON line)"""
import ctypes as C
import json
import os
import sys
import time

here = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(here, "..", "openal-soft_amd"), os.path.join(here, "..", "tests")]
import numpy as np
import oalgpu
import source_param_cases as sc
import channel_source_cases as cc

N, AVG, RATE = 1024, 1.5, 48000
cfg = dict(hrtf=False, sample_rate=RATE, frequency=44100, num_dry=5, num_real=0, num_sends=0, num_slots=0, wet_channels=4,
           dry_map=([0, 1, 3, 4, 8], [1.0] * 5))
api = oalgpu.Api(oalgpu.MATH_FAST)
s = oalgpu.Scene(api, sample_rate=RATE, num_dry=5, num_real=0, max_voices=N, max_buffers=16)
s.set_ambi_map(*cfg["dry_map"])
s.set_nfc(float(np.float32(343.3) / np.float32(AVG) / np.float32(RATE)), [1, 2, 2])
s.set_nfc_distance(AVG)
rng = np.random.default_rng(7)
buf = s.add_buffer(rng.uniform(-1, 1, 8000).astype(np.float32), oalgpu.FMT_FLOAT)
voices = np.array([s.add_voice(buf, True, position=(i * 13) % 4000, frequency=44100) for i in range(N)], np.uint32)
lis = sc.listener(distance_model=sc.INVERSE_CLAMPED)
s.set_listener(sc.listener_struct(lis))
srcs = [sc.source(position=[float(x) for x in rng.uniform(-4, 4, 3)], gain=0.05) for _ in range(N)]
props = sc.props_array(srcs)
desc = sc.context_desc(cfg, max_voices=N)
host = oalgpu.source_params_host(desc, sc.listener_struct(lis), props, 44100, dry_map=cfg["dry_map"])
w0, _ = oalgpu.channel_source_nfc_host(desc, sc.listener_struct(lis), cc.sources_array([cc.channel_source(x, cc.MONO, cc.ON) for x in srcs]),
                                       44100, AVG)
w0 = [float(x) for x in w0]
ids = [int(v) for v in voices]

L = oalgpu.lib
L.oalgpu_voice_set_source_props.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
L.oalgpu_voice_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
L.oalgpu_voice_set_nfc.argtypes = [C.c_void_p, C.c_uint32, C.c_float]
pv, pp, ph = voices.ctypes.data_as(C.c_void_p), C.cast(props, C.c_void_p), C.cast(host, C.c_void_p)
set_nfc, version, h = L.oalgpu_voice_set_nfc, L.oalgpu_version, s.h


def from_props():
    assert L.oalgpu_voice_set_source_props(h, pv, pp, N) == 0


def by_hand():
    assert L.oalgpu_voice_set_params(h, pv, ph, N) == 0
    for v, w in zip(ids, w0):
        set_nfc(h, v, w)
    s.sync()


def loop_alone():
    for v, w in zip(ids, w0):
        version()


res = {"context": "near-field, five dry lines, no sends", "sources": N}
for name, fn in (("oalgpu_voice_set_source_props", from_props), ("oalgpu_voice_set_params + 1024 oalgpu_voice_set_nfc", by_hand),
                 ("python loop of 1024 ctypes calls alone", loop_alone)):
    ts = []
    for k in range(55):
        t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
        if k >= 5:
            ts.append((t1 - t0) * 1e6)
        s.mix(256); s.sync()
    ts.sort()
    res[name] = {"median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1)}
res["ratio"] = round(res["oalgpu_voice_set_params + 1024 oalgpu_voice_set_nfc"]["median_us"] / res["oalgpu_voice_set_source_props"]["median_us"], 1)
s.close()
print(json.dumps(res), flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
