"""Measurement aid: what an attached context (oalgpu_context_attach) costs a device context's step.
  * period of the config-3 step loop (parameter block + oalgpu_mix_update, 4096 HRTF voices, FAST) alone, and with an attached
    6-line context of 64 voices on the device context's dry and real lines;
  * BusMergeKernel's own duration: two HIP events around oalgpu_post_process of a lines device context that has nothing else
    behind its buses (no slots, no post stage), its attached context's reduction long done.
python tools/attach_period.py [quick]"""
import ctypes as C
import gc, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "openal-soft_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import numpy as np
import oalgpu
from oalgpu import synth
import bench
import oracle_lib as ol
quick = len(sys.argv) > 1
V = 4096
api = oalgpu.Api(oalgpu.MATH_FAST)
mhr = open(os.path.join(ROOT, "tests", "golden", "default_hrtf.mhr"), "rb").read(); api._mhr = mhr


def lines_context(nvoices, num_dry, num_real=0):
    rng = np.random.default_rng(3)
    sc = api.make_scene(num_dry=num_dry, num_real=num_real, hrtf=False, max_voices=nvoices)
    buf = sc.add_buffer(rng.uniform(-1, 1, 9000).astype(np.float32), ol.FMT_FLOAT, loop_start=0, loop_end=9000)
    for v in range(nvoices):
        sc.add_voice(buf, looping=True, position=(v * 701) % 8000, frac=(v * 4099) % 65536)
        sc.set_params(v, ol.make_voice_params([60211, 48000, 71000][v % 3], ol.RS_BSINC24, dry_gains=rng.uniform(0.0, 0.02, num_dry)))
    return sc


sc, script = bench.build_scene(oalgpu, synth, api, 3, V, 0, mhr, 0)
allv = list(range(V)); moving = [v for v in allv if script.is_moving(v)]
sc.set_params_batch(allv, bench.param_array(oalgpu, script, allv, 0))
blocks = [sc.param_block(moving, bench.param_array(oalgpu, script, moving, k + 1)) for k in range(48)]
child = lines_context(64, 6)
gc.collect(); gc.disable()


def run(n):
    for k in range(n):
        sc.apply_block(blocks[k % len(blocks)])
        sc.mix(1024, post_process=True)


def period(n=300 if quick else 1000):
    run(n); sc.sync()
    out = []
    for _ in range(3):
        t0 = time.perf_counter(); run(n); sc.sync()
        out.append((time.perf_counter() - t0) / n * 1e6)
    return " ".join("%.2f" % x for x in out)


print("voice kernel:", sc.voice_kernel_name())
print("us per step, 4096 HRTF voices, no attachment         :", period())
sc.attach(child, [0, 1, 2, 3, 4, 5])
print("us per step, with an attached 6-line context (64 v.) :", period())
child.detach()
print("us per step, detached again                          :", period())

# ---- the merge kernel alone
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
dev = oalgpu.Scene(api, num_dry=4, num_real=2, max_voices=2, flags=oalgpu.CTX_SERIAL)
dev.attach(child, [0, 1, 2, 3, 4, 5])
stream = dev.bus_device_ptr()[2]
e0, e1 = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
times = []
for k in range(60):
    dev.mix_voices(1024); dev.sync()
    assert hip.hipEventRecord(e0, stream) == 0
    dev.post_process(1024)                   # nothing but BusMergeKernel: six destination lines, one contributor each
    assert hip.hipEventRecord(e1, stream) == 0
    dev.sync()
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
    times.append(ms.value * 1e3)
times = sorted(times[10:])
print("BusMergeKernel (6 lines x 1024 frames), us between two events around its launch: median %.2f, min %.2f, max %.2f"
      % (times[len(times) // 2], times[0], times[-1]))
