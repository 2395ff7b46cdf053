"""Reads a rocprofv3 --kernel-trace CSV (..._kernel_trace.csv) of a run on the deferring path and prints what lies around the
bounded-run voice launches (VoiceWave16Kernel<..., SPAN = true>, RunMixSpan in csrc/api.hip):
* the idle time of the main queue between two consecutive span launches, start(k+1) - end(k), by the updates launch k+1 covers
  (duration / 26.7 us, rounded and held to 1 .. 4, the most a launch covers: with a host that runs ahead, the sets the launch
  writes whose reductions it finds unfinished -- the trace has no record of the guards themselves);
* behind the last span launch of a block (nothing follows on the main queue for 40 us): the time from its end to the end of the
  last reduce-and-shift kernel behind it, and how many of them ran there.
usage: python tools/span_gaps.py TRACE.csv [us per covered update]"""
import bisect
import csv
import re
import sys
from collections import defaultdict

rows = list(csv.DictReader(open(sys.argv[1])))
per_update = float(sys.argv[2]) if len(sys.argv) > 2 else 26.7
ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows), key=lambda e: e[0])
voice = [e for e in ev if "VoiceWave16Kernel" in e[2]]
# the bounded-run form: the last template argument (SPAN) is true
span = [e for e in voice if (re.search(r"VoiceWave16Kernel<([^>]*)>", e[2]) or [None, ""])[1].split(",")[-1].strip() in ("true", "1")]
shift = [e for e in ev if "BusReduceShift" in e[2]]


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def covered(e):
    return min(4, max(1, round((e[1] - e[0]) / 1e3 / per_update)))


print(f"span launches {len(span)}, voice launches {len(voice)}, reduce-and-shift launches {len(shift)}")
gaps = defaultdict(list)
ends = []
is_span = set(span)
following = {}                                  # voice launch -> the next one on the main queue (the launches do not overlap)
for a, b in zip(voice, voice[1:]):
    following[a] = b
shift_starts = [s[0] for s in shift]
for e in span:
    nxt = following.get(e)
    if nxt is not None and nxt in is_span and nxt[0] - e[1] < 40_000:
        gaps[covered(nxt)].append((nxt[0] - e[1]) / 1e3)
    else:
        lim = nxt[0] if nxt is not None else e[1] + 200_000
        lo, hi = bisect.bisect_left(shift_starts, e[1] - 1_000), bisect.bisect_left(shift_starts, lim)
        behind = [s for s in shift[lo:hi] if s[1] <= e[1] + 200_000]
        if behind:
            ends.append(((max(s[1] for s in behind) - e[1]) / 1e3, len(behind), covered(e)))
print("idle gap of the main queue in front of a span launch, by the updates that launch covers:")
for n in sorted(gaps):
    g = gaps[n]
    print(f"  {n} update(s): {len(g):5d} gaps, median {med(g):6.2f} us, p10 {sorted(g)[len(g) // 10]:6.2f}, p90 {sorted(g)[len(g) * 9 // 10]:6.2f}")
print("drain behind a block's last span launch (its end to the end of the last reduce-and-shift kernel behind it):")
by = defaultdict(list)
for d, n, c in ends:
    by[(c, n)].append(d)
for (c, n) in sorted(by):
    d = by[(c, n)]
    print(f"  launch over {c} update(s), {n} reduce-and-shift launch(es) behind it: {len(d):4d} blocks, median {med(d):6.2f} us, min {min(d):6.2f}, max {max(d):6.2f}")
