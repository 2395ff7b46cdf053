"""The parameter stage of multi-channel and non-spatialized sources without a GPU: the numpy restatement
(tests/channel_source_cases.py) against the compiled reference, the case table's construction rules, the tolerances' derivation,
oalgpu_channel_source_params_host -- csrc/dev_source_channels.hpp compiled for the host, the functions ChannelParamsKernel runs --
against the restatement over the whole table, and its agreement with oalgpu_source_params_host for mono 3D sources."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bridge_lib as bl
import channel_source_cases as cc
import oalgpu
import source_param_cases as sc
from oalgpu import synth

needs_bridge = pytest.mark.skipif(not bl.available(), reason="needs oracle/_ref/liboalbridge.so (the compiled reference)")
MHR = open(os.path.join(bl.GOLDEN, "default_hrtf.mhr"), "rb").read()
ENTRY_POINTS = ("oalgpu_voice_set_channel_sources", "oalgpu_param_block_create_from_channel_sources", "oalgpu_channel_source_params_host")


@pytest.fixture(scope="module")
def tables():
    return cc.table()


def test_the_new_entry_points_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "oalgpu.h")).read()
    so = os.path.join(os.path.dirname(os.path.abspath(oalgpu.__file__)), "..", "liboalgpu.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout.split()
    for name in ENTRY_POINTS:
        assert "int " + name + "(" in header, name
        assert name in exported and hasattr(oalgpu.lib, name), name
    assert C.sizeof(oalgpu.ChannelSource) == C.sizeof(oalgpu.SourceProps) + 52


@needs_bridge
def test_restatement_step_equals_the_compiled_reference():
    """mStep of 50 stereo sources of the bridge (spatialize Auto: CalcNonAttnVoiceParams), pitches below one, at 48000 / 44100 and
    above MaxPitch, every resampler: the reference's own code in MODE_CPU against the restatement, exactly"""
    b = bl.Bridge(bl.MODE_CPU)
    try:
        buf = b.add_buffer_interleaved(np.zeros((4000, 2), np.float32), 2)
        lcg = synth.Lcg(0x5EED0062)
        lis = sc.listener(distance_model=sc.INVERSE_CLAMPED)
        cfg = dict(sc.DRY_CFG, num_dry=3, num_sends=0, num_slots=0, dry_map=([0, 1, 3], [1.0, 1.0, 1.0]))
        srcs = []
        for k in range(50):
            pitch = [lcg.uniform(0.3, 1.08), 48000.0 / 44100.0, lcg.uniform(1.09, 9.0), lcg.uniform(10.5, 14.0), 1.0][k % 5]
            pos = [lcg.uniform(-6.0, 6.0), lcg.uniform(-2.0, 2.0), lcg.uniform(-6.0, 6.0)]
            gain, gain_hf, rs = lcg.uniform(0.05, 1.0), (1.0, 0.5, 0.8)[k % 3], k % 10
            h = b.add_source_stereo(buf, True, 0, gain, pos, rs, pitch, gain_hf)
            srcs.append((h, cc.channel_source(sc.source(position=pos, gain=gain, pitch=pitch, resampler=rs, direct=[1.0, gain_hf, 5000.0, 1.0, 250.0]),
                                              cc.STEREO, cc.AUTO)))
        b.render(64)
        steps = set()
        for h, cs in srcs:
            want = b.source_state(h)[3]
            assert not cc.attenuated(cs)
            assert cc.calc(cs, lis, [], cfg)[0]["step"] == want, (cs["src"]["pitch"], want)
            steps.add(want)
        assert min(steps) < 65536 < max(steps) and 65536 in steps and (10 << 16) in steps
    finally:
        b.close()


def _features(case, cfg):
    """the branches a case takes, as the restatement takes them"""
    cs = cc.for_cfg(case["cs"], cfg)
    base, channels = cc.calc(cs, cc.LISTENERS[case["lis"]], sc.ENVIRONMENTS[case["env"]], cfg)
    src = cs["src"]
    multi = cs["channels"] != cc.MONO
    f = {"layout_" + cc.LAYOUT_NAMES[cs["channels"]], "spatialize_%d" % cs["spatialize"], "hrtf" if cfg["hrtf"] else "dry_lines",
         "route_attenuated" if base["branch"]["route"] else "route_plain"}
    if base["branch"]["route"]:
        f.add("distance" if base["branch"]["has_distance"] else "at_listener")
        dist, radius = float(base["distance"]), src["radius"]
        f.add("radius_zero" if radius == 0.0 else ("radius_below" if radius < dist else "radius_above"))
        if not base["branch"]["has_distance"] and radius > 0.0 and multi and cfg["hrtf"] and any(s >= 0 for s in base["send_slot"]):
            f.add("send_spread_quirk")                      # alu.cpp:1302 shows: sends panned with `spread`, the HRIRs with 0
    else:
        f.add("src_clamp_%d" % base["branch"]["src_clamp"])
    if base["branch"].get("dry_ceiling"):
        f.add("gain_mix_max")
    for ch in channels:
        if ch["short"] is not None:
            f.add("warp_short" if ch["short"] else "warp_long")
        if ch["silent"]:
            f.add("lfe")
    if multi:
        f.add("panning_%d" % int(np.sign(cs["panning"])))
    if cs["channels"] == cc.STEREO and tuple(cs["stereo_pan"]) != cc.DEFAULT_STEREO_PAN:
        f.add("stereo_pan_moved")
    if any(src["send"][i][0] >= 0 and base["send_slot"][i] < 0 for i in range(cfg["num_sends"])):
        f.add("inactive_slot")
    return f


FEATURES = ["layout_" + n for n in cc.LAYOUT_NAMES] + ["spatialize_0", "spatialize_1", "spatialize_2", "hrtf", "dry_lines", "route_attenuated",
                                                        "route_plain", "distance", "at_listener", "radius_zero", "radius_below", "radius_above",
                                                        "send_spread_quirk", "warp_short", "warp_long", "panning_-1", "panning_0", "panning_1",
                                                        "stereo_pan_moved", "lfe", "inactive_slot", "src_clamp_-1", "src_clamp_0", "src_clamp_1",
                                                        "gain_mix_max"]


def test_case_table_covers_every_branch_and_drops_little(tables):
    """about 300 channel sources, every branch at least 8 times among the kept ones; the +-4 ulp exclusions and the short warps take
    at most 10 % of the table and no group of it entirely; no kept warp is shorter than 1e-3"""
    kept, dropped = tables
    total = len(kept) + len(dropped)
    assert 280 <= total <= 340 and len(dropped) <= total // 10, (len(kept), len(dropped))
    built, left = {}, {}
    for cases, count in ((kept + dropped, built), (kept, left)):
        for c in cases:
            count[c["tag"]] = count.get(c["tag"], 0) + 1
    assert not [g for g, n in built.items() if n < 8], {g: n for g, n in built.items() if n < 8}
    assert not [g for g in built if left.get(g, 0) == 0]
    seen = {}
    for c in kept:
        for f in _features(c, sc.DRY_CFG) | _features(c, sc.HRTF_CFG):
            seen[f] = seen.get(f, 0) + 1
        for cfg in (sc.DRY_CFG, sc.HRTF_CFG):
            _, channels = cc.calc(cc.for_cfg(c["cs"], cfg), cc.LISTENERS[c["lis"]], sc.ENVIRONMENTS[c["env"]], cfg)
            assert all(ch["length"] is None or ch["length"] >= cc.MIN_LENGTH for ch in channels), c["tag"]
    assert not [f for f in FEATURES if seen.get(f, 0) < 8], {f: seen.get(f, 0) for f in FEATURES if seen.get(f, 0) < 8}


def test_tolerances_follow_the_reference_noise(tables):
    """the restatement in float32 against the same formulas in float64 over this table: where a class stays under
    source_param_cases.NOISE its tolerance is source_param_cases.TOLERANCE, where not, 8 x the figure measured here"""
    noise = cc.measure_noise(tables[0])
    print({k: "%.3g" % v for k, v in noise.items()}, cc.TOLERANCE)
    for k, v in noise.items():
        assert v <= cc.NOISE[k] * 1.005, (k, v, cc.NOISE[k])
        if cc.NOISE[k] <= sc.NOISE[k]:
            assert cc.TOLERANCE[k] == sc.TOLERANCE[k], k
        else:
            assert 0.99 * cc.NOISE[k] <= v and 8.0 * v <= cc.TOLERANCE[k] <= 8.5 * v, (k, v, cc.TOLERANCE[k])


def _host(cfg, lis, env, css):
    return oalgpu.channel_source_params_host(sc.context_desc(cfg), sc.listener_struct(lis), cc.sources_array(css), cfg["frequency"],
                                             slots=sc.env_array(env, cfg), dry_map=cfg["dry_map"],
                                             wet_maps=(cfg["wet_map"][0] * cfg["num_slots"], cfg["wet_map"][1] * cfg["num_slots"]),
                                             mhr=MHR if cfg["hrtf"] else None)


@pytest.mark.parametrize("cfg", [sc.DRY_CFG, sc.HRTF_CFG], ids=["dry_lines", "hrtf"])
def test_host_function_against_the_restatement(tables, cfg):
    """oalgpu_channel_source_params_host (glibc) over the whole table: mStep, resampler, FilterActive and send slots exactly, the
    rest within the tolerances; the channels a layout does not have zeroed.  (No HRIR indices for channel positions: see
    channel_source_cases.integer_results.)"""
    kept, _ = tables
    checked = 0
    zero = bytes(C.sizeof(oalgpu.VoiceParams))
    for li, lis in enumerate(cc.LISTENERS):
        for ei, env in enumerate(sc.ENVIRONMENTS):
            cases = [c for c in kept if c["lis"] == li and c["env"] == ei]
            if not cases:
                continue
            css = [cc.for_cfg(c["cs"], cfg) for c in cases]
            out = _host(cfg, lis, env, css)
            for i, (c, cs) in enumerate(zip(cases, css)):
                base, channels = cc.calc(cs, lis, env, cfg)
                for k in range(oalgpu.MAX_SOURCE_CHANNELS):
                    vp = out[i * oalgpu.MAX_SOURCE_CHANNELS + k]
                    if k >= len(channels):
                        assert bytes(vp) == zero, (c["tag"], k)
                        continue
                    cc.check_voice_params(vp, base, channels[k], cfg, "%s channel %d" % (c["tag"], k))
                    assert vp.resampler == cs["src"]["resampler"]
                checked += 1
    assert checked == len(kept)


@pytest.mark.parametrize("cfg", [sc.DRY_CFG, sc.HRTF_CFG], ids=["dry_lines", "hrtf"])
@pytest.mark.parametrize("mode", [cc.ON, cc.AUTO], ids=["on", "auto"])
def test_mono_source_equals_the_mono_stage_bit_for_bit(cfg, mode):
    """a MONO source with spatialize On or Auto over source_param_cases' kept cases: the record oalgpu_source_params_host makes of
    its props, byte for byte, whatever `panning` and `stereo_pan` say.  Both host functions fill their records through the same
    code (api_sources.hip: FillVoiceParams), so this pins the route, the mono leg and the zeroing of the other seven records, not
    the arithmetic: that oalgpu_source_params_host still computes what it did is test_source_params_host.py's claim (against the
    restatement), and that ChannelParamsKernel equals SourceParamsKernel is
    test_gpu_channel_sources.py::test_mono_auto_equals_the_mono_stage_on_the_device's."""
    kept, _ = sc.table(MHR)
    zero = bytes(C.sizeof(oalgpu.VoiceParams))
    for li, lis in enumerate(sc.LISTENERS):
        for ei, env in enumerate(sc.ENVIRONMENTS):
            srcs = [sc.for_cfg(c["src"], cfg) for c in kept if c["lis"] == li and c["env"] == ei]
            if not srcs:
                continue
            want = oalgpu.source_params_host(sc.context_desc(cfg), sc.listener_struct(lis), sc.props_array(srcs), cfg["frequency"],
                                             slots=sc.env_array(env, cfg), dry_map=cfg["dry_map"],
                                             wet_maps=(cfg["wet_map"][0] * cfg["num_slots"], cfg["wet_map"][1] * cfg["num_slots"]),
                                             mhr=MHR if cfg["hrtf"] else None)
            got = _host(cfg, lis, env, [cc.channel_source(s, cc.MONO, mode, (0.3, -1.0), 0.5) for s in srcs])
            for i in range(len(srcs)):
                assert bytes(got[i * oalgpu.MAX_SOURCE_CHANNELS]) == bytes(want[i]), (li, ei, i)
                assert all(bytes(got[i * oalgpu.MAX_SOURCE_CHANNELS + k]) == zero for k in range(1, oalgpu.MAX_SOURCE_CHANNELS))


def test_host_function_refuses_what_it_cannot_compute():
    lis = oalgpu.ListenerParams.default()
    good = cc.channel_source(sc.source(), cc.STEREO)
    with pytest.raises(oalgpu.OalgpuError, match="without a data set"):
        oalgpu.channel_source_params_host(sc.context_desc(sc.HRTF_CFG), lis, cc.sources_array([good]), 44100)
    desc = sc.context_desc(sc.DRY_CFG)
    bad = sc.source(); bad["send"][0][0] = 5
    with pytest.raises(oalgpu.OalgpuError, match="send slot out of range"):
        oalgpu.channel_source_params_host(desc, lis, cc.sources_array([cc.channel_source(bad, cc.QUAD)]), 44100)
    for field, value in (("channels", 7), ("channels", -1), ("spatialize", 3), ("spatialize", -1)):
        with pytest.raises(oalgpu.OalgpuError, match="channels or spatialize out of range"):
            oalgpu.channel_source_params_host(desc, lis, cc.sources_array([dict(good, **{field: value})]), 44100)
    with pytest.raises(oalgpu.OalgpuError, match="bad arguments"):
        oalgpu.channel_source_params_host(desc, lis, cc.sources_array([good]), 0)
    L = oalgpu.lib
    arr = cc.sources_array([good])
    out = (oalgpu.VoiceParams * oalgpu.MAX_SOURCE_CHANNELS)()
    L.oalgpu_channel_source_params_host.argtypes = [C.c_void_p] * 8 + [C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    args = [C.cast(C.pointer(desc), C.c_void_p), C.cast(C.pointer(lis), C.c_void_p), None, None, None, None, None, None, 0, 44100]
    assert L.oalgpu_channel_source_params_host(*args, None, 1, out) == -2
    assert L.oalgpu_channel_source_params_host(*args, arr, 1, None) == -2
    assert L.oalgpu_channel_source_params_host(None, *args[1:], arr, 1, out) == -2
    assert L.oalgpu_channel_source_params_host(*args, arr, 1, out) == 0
