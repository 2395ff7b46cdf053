"""Measurement aid: what the config-3 step loop (parameter block + oalgpu_mix_update, a synchronisation every K steps, as bench.py
times it) was launched as -- voice launches by the updates they covered, updates on the one-launch reduce-and-shift
(oalgpu_context_launch_stats) -- and its period.  python tools/launch_span_stats.py [xflags [K [blocks]]]"""
import os, sys, time, gc
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "openal-soft_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import oalgpu
from oalgpu import synth
import bench
xf = int(sys.argv[1]) if len(sys.argv) > 1 else 16
K = int(sys.argv[2]) if len(sys.argv) > 2 else 20
nblocks = int(sys.argv[3]) if len(sys.argv) > 3 else 50
V = 4096
api = oalgpu.Api(oalgpu.MATH_FAST, ctx_flags=xf)
mhr = open(os.path.join(ROOT, "tests", "golden", "default_hrtf.mhr"), "rb").read(); api._mhr = mhr
sc, script = bench.build_scene(oalgpu, synth, api, 3, V, 0, mhr, 0)
allv = list(range(V)); moving = [v for v in allv if script.is_moving(v)]
sc.set_params_batch(allv, bench.param_array(oalgpu, script, allv, 0))
blocks = [sc.param_block(moving, bench.param_array(oalgpu, script, moving, k + 1)) for k in range(48)]
gc.collect(); gc.disable()
def block(n):
    for k in range(n):
        sc.apply_block(blocks[k % len(blocks)])
        sc.mix(1024, post_process=True)
    sc.sync()
for _ in range(20): block(K)
s0, p0 = sc.launch_stats()
t0 = time.perf_counter()
for _ in range(nblocks): block(K)
dt = time.perf_counter() - t0
s1, p1 = sc.launch_stats()
spans = [b - a for a, b in zip(s0, s1)]
print("xflags", xf, "K", K, "blocks", nblocks, ": period %.2f us per step" % (dt / (K * nblocks) * 1e6))
print("  voice launches that covered 1 / 2 / 3 / 4 updates:", spans, "= %.2f updates per launch" % (K * nblocks / max(1, sum(spans))))
print("  updates on the one-launch reduce-and-shift: %d of %d" % (p1 - p0, K * nblocks))
