"""CPU side of the loop-edge cases (tests/loop_edge_cases.py): the window arithmetic the cases are placed with, the
branch every case sits on, and the liveness of the cases -- on the oracle, each edge voice's output depends on the edge
it was placed at, so a kernel that got the edge wrong cannot agree with the oracle by accident."""
import numpy as np
import pytest

import loop_edge_cases as lc
import oracle_lib as ol
from test_tolerance_model import multi_voice_tolerance


def test_calc_buffer_size_hand_computed():
    # ext = 1 at step <= 1.0: ((dst - 1) * step + frac) >> 16, + 1 + MaxResamplerEdge
    assert lc.calc_buffer_size(0, 65536, 1024) == (1024, 1023 + 1 + 24)
    assert lc.calc_buffer_size(12345, 65536, 1024) == (1024, 1048)
    assert lc.calc_buffer_size(0, 1, 1024) == (1024, 0 + 1 + 24)
    assert lc.calc_buffer_size(65535, 1, 1024) == (1024, 1 + 1 + 24)
    assert lc.calc_buffer_size(777, 60211, 1024) == (1024, ((1023 * 60211 + 777) >> 16) + 25)
    assert lc.calc_buffer_size(0, 131072, 500) == (500, 1000 + 24)
    assert lc.calc_buffer_size(0, 65537, 1) == (1, 1 + 24)           # ext = 0 above 1.0: one whole step
    # saturated: 1304 source samples at most, the dst count cut to a multiple of 4
    assert lc.calc_buffer_size(0, 131072, 1024) == (640, 1304)
    assert lc.calc_buffer_size(3, 655360, 1024) == (((1280 << 16) - 3) // 655360 & ~3, 1304)
    assert lc.calc_buffer_size(0, 655360, 1) == (1, 10 + 24)


def test_classifier_hand_computed():
    f32, u8 = ol.FMT_FLOAT, ol.FMT_UBYTE
    b = lc.BufSpec(2000, 100, 1000, f32, 1)
    assert lc.classify(b, True, 1000, 5, 60211, 1024) == "past-loop-end"
    assert lc.classify(b._replace(le=2000), True, 2000, 5, 60211, 1024) == "end-clamp"     # loop end == length: no rule
    assert lc.classify(b, True, 0, 0, 65536, 1024) == "copy"
    assert lc.classify(b, True, 0, 1, 65536, 1024) == "one-wrap"           # 0 + 1048 > 1000: the window wraps
    assert lc.classify(b._replace(le=1048), True, 0, 1, 65536, 1024) == "linear"
    assert lc.classify(b._replace(le=1047), True, 0, 1, 65536, 1024) == "one-wrap"
    assert lc.classify(b, True, 500, 1, 65536, 1024) == "one-wrap"         # 1048 <= 500 + 900
    # (le - pos) + (le - ls) == bsrc: covered; one less: the generic loop
    assert lc.classify(lc.BufSpec(700, 0, 600, f32, 1), True, 152, 1, 65536, 1024) == "one-wrap"
    assert lc.classify(lc.BufSpec(700, 0, 600, f32, 1), True, 153, 1, 65536, 1024) == "generic"
    assert lc.classify(b._replace(fmt=u8), True, 0, 1, 60211, 1024) == "generic"
    assert lc.classify(b, True, 0, 1, 131072, 1024) == "generic"           # 1304 source samples > 1088
    assert lc.classify(b, False, 1000, 1, 60211, 1024) == "end-clamp"
    assert lc.classify(b, False, 912, 1, 60211, 1024) == "linear"          # 912 + 1088 == 2000
    assert lc.classify(b._replace(fs=2), False, 0, 1, 60211, 1024) == "end-clamp"


# the branch each family of cases is placed on (the name's prefix), where the first window fits the register gather
EXPECT = {"boundary_inside": "one-wrap", "boundary_equal": "one-wrap", "boundary_outside": "generic",
          "boundary_len_shorter": "generic", "boundary_len_longer": "one-wrap",
          "linear_limit_len-1": "linear", "linear_limit_len+0": "linear", "linear_limit_len+1": "one-wrap",
          "linear_limit_loopend-1": "linear", "linear_limit_loopend+0": "linear", "linear_limit_loopend+1": "one-wrap",
          "oneshot_linear_limit-1": "linear", "oneshot_linear_limit+0": "linear", "oneshot_linear_limit+1": "end-clamp",
          "at_loop_end": "past-loop-end", "past_loop_end": "past-loop-end", "u8_": "generic",
          "view2_i16_long_loop": "one-wrap"}


@pytest.mark.parametrize("step", lc.STEPS)
def test_every_case_sits_on_its_branch(step):
    voices = lc.scene(step)
    names = [v.name for v in voices]
    assert len(set(names)) == len(names)
    fits = lc.calc_buffer_size(12345, step, lc.todo_of(step)[0])[1] <= lc.WINDOW
    seen = set()
    for v in voices:
        assert v.buf.ls < v.buf.le <= v.buf.n and v.pos >= 0
        for prefix, branch in EXPECT.items():
            if v.name.startswith(prefix) and (fits or branch == "past-loop-end"):
                assert v.branch == branch, (step, v.name, v.branch)
                seen.add(prefix)
    assert "at_loop_end" in seen and "past_loop_end" in seen
    if fits:
        assert {"boundary_equal", "boundary_outside", "linear_limit_len+0", "linear_limit_len+1"} <= seen
    assert {v.branch for v in voices} >= ({"linear", "one-wrap", "end-clamp", "generic", "past-loop-end"} if fits
                                          else {"generic", "past-loop-end"})
    if step == lc.FRAC_ONE:
        assert {v.branch for v in lc.scene(step, frac_zero=True)} >= {"copy", "past-loop-end"}


def _oracle():
    L = ol.load("ref" if ol.available("ref") else "port")
    L.L.oal_set_simd(1)
    return L


def _single(L, step, i, **kw):
    buses, ints, _ = lc.run(L, step, "dry", only=[i], **kw)
    return np.concatenate(buses).astype(np.float64), ints


def _bound(want):
    return multi_voice_tolerance(1, 1, float(np.abs(want).max()))


@pytest.mark.parametrize("step", lc.STEPS)
def test_sentinel_cases_reach_their_loop_end(step):
    """Every looping case whose run carries it to its loop end, inside a buffer that goes on past it, sounds different
    by more than 100x the tolerance when the loop end is moved to the buffer's end: the wrap happened, and a kernel that
    read on past the loop end (or wrapped to 0) would be off by that much."""
    L = _oracle()
    advance = (sum(lc.todo_of(step)) * step) >> 16
    checked = 0
    for i, v in enumerate(lc.scene(step)):
        if not v.looping or v.buf.le == v.buf.n or v.pos >= v.buf.le or v.pos + advance + 2 < v.buf.le:
            continue
        want, _ = _single(L, step, i)
        other, _ = _single(L, step, i, loop_end_to_len=True)
        assert np.abs(want).max() > 1e-3, v.name
        assert np.abs(other - want).max() > 100 * _bound(want), (step, v.name)
        checked += 1
    assert checked >= 8, checked


@pytest.mark.parametrize("step", lc.STEPS)
def test_past_the_loop_end_plays_on_unlooped(step):
    """A looping voice at or past its loop end plays the rest of the buffer: it differs from the same voice started one
    sample before the loop end (which wraps), and -- where the run carries it to the buffer's end -- stops."""
    L = _oracle()
    advance = (sum(lc.todo_of(step)) * step) >> 16
    cases = [(i, v) for i, v in enumerate(lc.scene(step)) if v.branch == "past-loop-end"]
    assert len(cases) >= 4
    for i, v in cases:
        want, ints = _single(L, step, i)
        other, _ = _single(L, step, i, move_in=True)
        assert np.abs(other - want).max() > 100 * _bound(want), (step, v.name)
        if v.pos + advance >= v.buf.n + 2:
            assert ints[-1][0][0] in (ol.VOICE_STOPPING, ol.VOICE_STOPPED) and ints[-1][0][3] == 0, (step, v.name, ints[-1])
        else:
            assert ints[-1][0][0] == ol.VOICE_PLAYING and v.buf.le <= ints[-1][0][1] < v.buf.n, (step, v.name, ints[-1])
