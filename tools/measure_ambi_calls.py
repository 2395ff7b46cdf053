"""DESIGN.md 3.28's second table: the calling thread's wall clock around oalgpu_voice_set_ambi_sources against
oalgpu_voice_set_params fed host-built records (oalgpu_ambi_source_params_host's) of the same 64 third-order sources = 1024
channel voices, on a fourth-order dry-line context with one send; medians of 50 calls after 5 warm-ups, an update between the
calls.  Both calls end in the same stream synchronise, so the figures include the kernels they launch.  Beside them the bytes
each call hands over.

    python tools/measure_ambi_calls.py [out.json]        (needs a GPU; prints one JSON line)"""
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
import ambi_source_cases as ac
from oalgpu import synth

nsrc, nch = 64, 16
cfg = ac.device_cfg(4, False, 1)
api = oalgpu.Api(oalgpu.MATH_FAST)
s = oalgpu.Scene(api, sample_rate=48000, num_dry=cfg["num_dry"], num_real=2, num_sends=1, num_slots=1, wet_channels=4, hrtf=False,
                 max_voices=nsrc * nch, max_buffers=nsrc * nch + 16)
s.set_ambi_map(*cfg["dry_map"])
s.set_ambi_order(4, False)
s.set_ambi_upsampler(3, False, ac.UPSAMPLERS[(3, False)])
lcg = synth.Lcg(7)
buf = s.add_buffer(np.array([lcg.uniform(-1, 1) for _ in range(4000 * nch)], np.float32), oalgpu.FMT_FLOAT, frame_step=nch)
voices = []
for i in range(nsrc):
    first = s.add_ambi_voice(buf, nch, True, position=(i * 13) % 2000, frequency=44100)
    voices.append(list(range(first, first + nch)))
lis, env = sc.LISTENERS[0], sc.ENVIRONMENTS[0]
s.set_listener(sc.listener_struct(lis))
e = env[0]; s.set_slot_send_environment(0, e["active"], e["room_rolloff"], e["decay_time"], e["air_absorption_gain_hf"])
pool = [c for c in ac.table()[0] if c["group"] == "third_on_fourth"]
css = [ac.for_cfg(pool[i % len(pool)]["cs"], cfg) for i in range(nsrc)]
arr = ac.sources_array(css, voices)
host, _, _ = ac.params_host(cfg, lis, env, css)
recs = (oalgpu.VoiceParams * (nsrc * nch))()
ids = (C.c_uint32 * (nsrc * nch))()
for i in range(nsrc):
    for ch in range(nch):
        recs[nch * i + ch] = host[i * oalgpu.MAX_AMBI_CHANNELS + ch]; ids[nch * i + ch] = voices[i][ch]
L = oalgpu.lib
L.oalgpu_voice_set_ambi_sources.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
L.oalgpu_voice_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
pa, pr, pi = C.cast(arr, C.c_void_p), C.cast(recs, C.c_void_p), C.cast(ids, C.c_void_p)
res = {"context": "fourth-order dry lines, one send", "sources": nsrc, "records": nsrc * nch,
       "bytes_in": {"oalgpu_voice_set_params": C.sizeof(recs) + C.sizeof(ids), "oalgpu_voice_set_ambi_sources": C.sizeof(arr)}}
for name, fn in (("oalgpu_voice_set_params", lambda: L.oalgpu_voice_set_params(s.h, pi, pr, nsrc * nch)),
                 ("oalgpu_voice_set_ambi_sources", lambda: L.oalgpu_voice_set_ambi_sources(s.h, pa, nsrc))):
    ts = []
    for k in range(55):
        t0 = time.perf_counter(); rc = fn(); t1 = time.perf_counter()
        assert rc == 0
        if k >= 5:
            ts.append((t1 - t0) * 1e6)
        s.mix(256); s.sync()
    ts.sort()
    res[name] = {"median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1)}
s.close()
print(json.dumps(res), flush=True)
if len(sys.argv) > 1:
    json.dump([res], open(sys.argv[1], "w"), indent=1)
