"""DESIGN.md 3.25's second table: the calling thread's wall clock around oalgpu_voice_set_channel_sources against
oalgpu_voice_set_params fed host-built records (oalgpu_channel_source_params_host's) of the same 512 stereo sources = 1024 channel
voices, on an HRTF context with one send and on a dry-line context with two; medians of 50 calls after 5 warm-ups, an update
between the calls.  Both calls end in the same stream synchronise, so the figures include the kernels they launch.

    python tools/measure_channel_calls.py [out.json]        (needs a GPU; prints one JSON line per context)"""
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
import bridge_lib as bl
from oalgpu import synth

MHR_PATH = os.path.join(bl.GOLDEN, "default_hrtf.mhr")
MHR = open(MHR_PATH, "rb").read()
out = []
for which, cfg in (("hrtf, one send", sc.HRTF_CFG), ("dry lines, two sends", sc.DRY_CFG)):
    nsrc = 512
    api = oalgpu.Api(oalgpu.MATH_FAST)
    if cfg["hrtf"]:
        api.hrtf_load(MHR_PATH)
    s = oalgpu.Scene(api, sample_rate=48000, num_dry=cfg["num_dry"], num_real=2, num_sends=cfg["num_sends"], num_slots=cfg["num_slots"],
                     wet_channels=4, hrtf=cfg["hrtf"], max_voices=2 * nsrc, max_buffers=2 * nsrc + 16)
    if cfg["hrtf"]:
        s.set_direct_hrtf_from_store(synth.AMBI_POINTS_1O, synth.AMBI_MATRIX_1O, synth.AMBI_ORDER_HF_GAIN_1O, 400.0)
    else:
        s.set_ambi_map(*cfg["dry_map"])
    lcg = synth.Lcg(7)
    buf = s.add_buffer(np.array([lcg.uniform(-1, 1) for _ in range(8000)], np.float32), oalgpu.FMT_FLOAT, frame_step=2)
    voices = [[s.add_ambi_voice(buf, 2, True, position=(i * 13) % 4000, frequency=44100)] for i in range(nsrc)]
    voices = [[v[0], v[0] + 1] for v in voices]
    lis, env = cc.LISTENERS[0], sc.ENVIRONMENTS[0]
    s.set_listener(sc.listener_struct(lis))
    for i in range(cfg["num_slots"]):
        e = env[i]; s.set_slot_send_environment(i, e["active"], e["room_rolloff"], e["decay_time"], e["air_absorption_gain_hf"])
    pool = [c for c in cc.table()[0] if c["lis"] == 0 and c["env"] == 0 and c["cs"]["channels"] == cc.STEREO]
    css = [cc.for_cfg(pool[i % len(pool)]["cs"], cfg) for i in range(nsrc)]
    arr = cc.sources_array(css, voices)
    host = oalgpu.channel_source_params_host(sc.context_desc(cfg), sc.listener_struct(lis), arr, 44100, slots=sc.env_array(env, cfg),
                                             dry_map=cfg["dry_map"], wet_maps=(cfg["wet_map"][0] * cfg["num_slots"], cfg["wet_map"][1] * cfg["num_slots"]),
                                             mhr=MHR if cfg["hrtf"] else None)
    recs = (oalgpu.VoiceParams * (2 * nsrc))()
    ids = (C.c_uint32 * (2 * nsrc))()
    for i in range(nsrc):
        for ch in range(2):
            recs[2 * i + ch] = host[i * 8 + ch]; ids[2 * i + ch] = voices[i][ch]
    L = oalgpu.lib
    L.oalgpu_voice_set_channel_sources.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.oalgpu_voice_set_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    pa, pr, pi = C.cast(arr, C.c_void_p), C.cast(recs, C.c_void_p), C.cast(ids, C.c_void_p)
    res = {"context": which, "sources": nsrc, "records": 2 * nsrc}
    for name, fn in (("oalgpu_voice_set_params", lambda: L.oalgpu_voice_set_params(s.h, pi, pr, 2 * nsrc)),
                     ("oalgpu_voice_set_channel_sources", lambda: L.oalgpu_voice_set_channel_sources(s.h, pa, nsrc))):
        ts = []
        for k in range(55):
            t0 = time.perf_counter(); rc = fn(); t1 = time.perf_counter()
            assert rc == 0
            if k >= 5:
                ts.append((t1 - t0) * 1e6)
            s.mix(256, post_process=cfg["hrtf"]); s.sync()
        ts.sort()
        res[name] = {"median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1)}
    s.close()
    out.append(res)
    print(json.dumps(res), flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
