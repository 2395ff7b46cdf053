"""The 3D source parameter stage without a GPU: the numpy restatement of CalcAttnVoiceParams / CalcPanningAndFilters
(tests/source_param_cases.py) against the compiled reference, the case table's construction rules, the tolerances' derivation,
and oalgpu_source_params_host -- csrc/dev_source.hpp compiled for the host, the same functions SourceParamsKernel runs --
against the restatement over the whole table."""
import os

import numpy as np
import pytest

import bridge_lib as bl
import oalgpu
import oracle_lib as ol
import source_param_cases as sc
from oalgpu import synth

needs_bridge = pytest.mark.skipif(not bl.available(), reason="needs oracle/_ref/liboalbridge.so (built where /root/reference is mounted)")
MHR = open(os.path.join(bl.GOLDEN, "default_hrtf.mhr"), "rb").read()


@pytest.fixture(scope="module")
def tables():
    return sc.table(MHR)


def test_the_new_entry_points_are_declared_and_exported():
    for name in ("oalgpu_context_set_listener", "oalgpu_slot_set_send_environment", "oalgpu_voice_set_source_props",
                 "oalgpu_param_block_create_from_sources", "oalgpu_source_params_host"):
        assert hasattr(oalgpu.lib, name), name


@needs_bridge
def test_restatement_step_equals_the_compiled_reference():
    """mStep of 200 seeded sources the bridge can reach (InverseClamped, RefDistance 1, MaxDistance FLT_MAX, rolloff 1; any position,
    gain, pitch, gain_hf, resampler; one send into an EAX reverb slot), the reference's own CalcAttnVoiceParams in MODE_CPU against
    the restatement: exactly.  Pitches cross 1.0 (in output samples: 48000 / 44100) and exceed MaxPitch."""
    b = bl.Bridge(bl.MODE_CPU, num_sends=1)
    try:
        slot = b.add_reverb_slot(ol.ReverbProps.make(), 1.0)
        buf = b.add_buffer(np.zeros(48000, np.float32))
        lcg = synth.Lcg(0x5EED0052)
        lis = sc.listener(distance_model=sc.INVERSE_CLAMPED)
        env = [dict(active=1, room_rolloff=0.0, decay_time=1.49, air_absorption_gain_hf=0.994)]
        cfg = dict(sc.DRY_CFG, num_dry=3, num_sends=1, num_slots=1, dry_map=([0, 1, 3], [1.0, 1.0, 1.0]))
        srcs = []
        for k in range(200):
            pos = [lcg.uniform(-6.0, 6.0), lcg.uniform(-2.0, 2.0), lcg.uniform(-6.0, 6.0)]
            pitch = [lcg.uniform(0.3, 1.08), 48000.0 / 44100.0, lcg.uniform(1.09, 9.0), lcg.uniform(10.5, 14.0), 1.0][k % 5]
            gain, gain_hf, rs = lcg.uniform(0.05, 1.0), (1.0, 0.5, 0.8)[k % 3], k % 10
            h = b.add_source_ex(buf, True, 0, gain, pos, rs, pitch, gain_hf, slot, 0.5, 0.7)
            s = sc.source(position=pos, gain=gain, pitch=pitch, resampler=rs, direct=[1.0, gain_hf, 5000.0, 1.0, 250.0])
            s["send"][0] = [0, 0.5, 0.7, 5000.0, 1.0, 250.0]
            srcs.append((h, s))
        b.render(64)
        steps = set()
        for h, s in srcs:
            want = b.source_state(h)[3]
            assert sc.calc(s, lis, env, cfg)["step"] == want, (s["pitch"], s["position"], want)
            steps.add(want)
        assert min(steps) < 65536 < max(steps) and 65536 in steps and (10 << 16) in steps
    finally:
        b.close()


def _group(tag):
    if tag.startswith("resampler"):
        return tag.split("_", 1)         # counts for the resampler and for the step's side of one
    if tag.startswith("cone_") and "_no_" in tag:
        return [tag.split("_no_")[0], "cone_no_" + tag.split("_no_")[1]]
    return [tag]


def test_case_table_covers_every_branch_and_drops_little(tables):
    """about 400 sources, every branch at least 8 times as built; the +-4 ulp exclusions take at most 10 % of them and no branch
    entirely"""
    kept, dropped = tables
    total = len(kept) + len(dropped)
    assert 380 <= total <= 500 and len(dropped) <= total // 10, (len(kept), len(dropped))
    built, left = {}, {}
    for cases, count in ((kept + dropped, built), (kept, left)):
        for c in cases:
            for g in _group(c["tag"]):
                count[g] = count.get(g, 0) + 1
    assert not [g for g, n in built.items() if n < 8], {g: n for g, n in built.items() if n < 8}
    assert not [g for g in built if left.get(g, 0) == 0]
    # ... and the branches as the restatement takes them, over the kept cases
    seen = {}
    for c in kept:
        for cfg in (sc.DRY_CFG, sc.HRTF_CFG):
            r = sc.calc(sc.for_cfg(c["src"], cfg), sc.LISTENERS[c["lis"]], sc.ENVIRONMENTS[c["env"]], cfg)
            for k, v in list(r["branch"].items()) + [("rs_kind", r["rs"][0]), ("step_side", int(np.sign(r["step"] - 65536))),
                                                      ("max_pitch", r["step"] == 10 << 16)]:
                seen[(k, v)] = seen.get((k, v), 0) + 1
    for want in [("cone", 1), ("cone", 2), ("cone", 3), ("doppler", 0), ("doppler", 1), ("doppler", 2), ("doppler", 3),
                 ("beyond_ref", True), ("beyond_ref", False), ("clamp", "ref>max"), ("clamp", "lo"), ("clamp", "hi"), ("clamp", "in"),
                 ("has_distance", False), ("has_direction", True), ("spread", 0), ("spread", 1), ("spread", 2), ("absorb", True),
                 ("absorb", False), ("dry_ceiling", True), ("dry_clamp", -1), ("dry_clamp", 1), ("lin_dry", True), ("lin_dry", False),
                 ("rs_kind", 0), ("rs_kind", 1), ("rs_kind", 2), ("rs_kind", 3), ("rs_kind", 4), ("step_side", -1), ("step_side", 0),
                 ("step_side", 1), ("max_pitch", True)]:
        assert seen.get(want, 0) >= 8, (want, seen.get(want, 0))


def test_tolerances_are_eight_times_the_reference_noise(tables):
    """the restatement in float32 against the same formulas in float64 over the table: the reference's own rounding noise per output
    class; the device is allowed 8 x that (source_param_cases.TOLERANCE)"""
    noise = sc.measure_noise(tables[0])
    print({k: "%.3g" % v for k, v in noise.items()}, sc.TOLERANCE)
    for k, v in noise.items():
        assert v <= sc.NOISE[k] and 8.0 * v <= sc.TOLERANCE[k] <= 10.0 * v, (k, v, sc.NOISE[k], sc.TOLERANCE[k])


@pytest.mark.parametrize("cfg", [sc.DRY_CFG, sc.HRTF_CFG], ids=["dry_lines", "hrtf"])
def test_host_function_against_the_restatement(tables, cfg):
    """oalgpu_source_params_host (glibc) over the whole table: mStep, resampler, FilterActive and send slots exactly, the rest
    within the tolerances"""
    kept, _ = tables
    desc = sc.context_desc(cfg)
    checked = 0
    for li, lis in enumerate(sc.LISTENERS):
        for ei, env in enumerate(sc.ENVIRONMENTS):
            cases = [c for c in kept if c["lis"] == li and c["env"] == ei]
            if not cases:
                continue
            srcs = [sc.for_cfg(c["src"], cfg) for c in cases]
            out = oalgpu.source_params_host(desc, sc.listener_struct(lis), sc.props_array(srcs), cfg["frequency"],
                                            slots=sc.env_array(env, cfg), dry_map=cfg["dry_map"],
                                            wet_maps=(cfg["wet_map"][0] * cfg["num_slots"], cfg["wet_map"][1] * cfg["num_slots"]),
                                            mhr=MHR if cfg["hrtf"] else None)
            for c, s, vp in zip(cases, srcs, out):
                r = sc.calc(s, lis, env, cfg)
                sc.check_voice_params(vp, r, cfg, c["tag"])
                assert vp.resampler == s["resampler"]
                if cfg["hrtf"]:      # the direction lands on the same HRIRs with the same delays (what the exclusions guard)
                    mine = sc.hrir_blend(MHR, cfg, dict(ev=vp.hrtf_ev, az=vp.hrtf_az, hrtf_dist=vp.hrtf_dist, spread=vp.hrtf_spread))
                    assert mine[:2] == sc.hrir_blend(MHR, cfg, r)[:2], c["tag"]
                checked += 1
    assert checked == len(kept)


def test_host_function_refuses_what_it_cannot_compute():
    desc = sc.context_desc(sc.HRTF_CFG)
    props = sc.props_array([sc.source()])
    with pytest.raises(oalgpu.OalgpuError, match="without a data set"):
        oalgpu.source_params_host(desc, oalgpu.ListenerParams.default(), props, 44100)
    bad = sc.source(); bad["send"][0][0] = 5
    with pytest.raises(oalgpu.OalgpuError, match="out of range"):
        oalgpu.source_params_host(sc.context_desc(sc.DRY_CFG), oalgpu.ListenerParams.default(), sc.props_array([bad]), 44100)
