#!/usr/bin/env python
"""Per-call summary of a rocprofv3 kernel trace of tools/c4_lbl_run.py: the span of each ansfm_cirsrad_ck_scatter call, the time
of its Hansen walk, phase-matrix and chain kernels, and how much of the walk / phase matrices ran while chains ran (the
union of the chain kernels' intervals).  Calls are cut at k_layer_prep_lbl.

    python3 tools/summarize_lbl_windows.py prof_c4_lbl/run_kernel_trace.csv     # one JSON line per call
"""
import csv
import json
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
calls = []; cur = None
for r in rows:
    n = r["Kernel_Name"]
    if "k_layer_prep_lbl" in n:
        cur = []; calls.append(cur)
    if cur is not None:
        cur.append((n, int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Stream_Id"])))
def union(iv):
    iv = sorted(iv); tot = 0; s0 = e0 = None
    for s, e in iv:
        if e0 is None or s > e0:
            if e0 is not None: tot += e0 - s0
            s0, e0 = s, e
        else: e0 = max(e0, e)
    if e0 is not None: tot += e0 - s0
    return tot
def inter(a, b):   # total length of intervals a covered by union of b
    out = 0
    bu = sorted(b)
    for s, e in a:
        for bs, be in bu:
            lo, hi = max(s, bs), min(e, be)
            if hi > lo: out += hi - lo
    return out
res = []
for i, c in enumerate(calls):
    walk = [(s, e) for n, s, e, _ in c if "hansen" in n]
    phase = [(s, e) for n, s, e, _ in c if "k_ms_phase" in n]
    chain = [(s, e) for n, s, e, _ in c if "chain" in n]
    # merge chain intervals first so that overlap is not double counted
    cu = []
    for s, e in sorted(chain):
        if cu and s <= cu[-1][1]: cu[-1] = (cu[-1][0], max(cu[-1][1], e))
        else: cu.append((s, e))
    span = max(e for _, _, e, _ in c) - min(s for _, s, _, _ in c)
    ms = lambda x: round(x / 1e6, 3)
    res.append(dict(call=i, kernels=len(c), span_ms=ms(span), walk_launches=len(walk), walk_ms=ms(sum(e - s for s, e in walk)),
                    walk_hidden_by_chains_ms=ms(inter(walk, cu)), phase_ms=ms(sum(e - s for s, e in phase)),
                    phase_hidden_by_chains_ms=ms(inter(phase, cu)),
                    chain_launches=len(chain), chain_busy_ms=ms(union(chain)),
                    walk_max_ms=ms(max((e - s for s, e in walk), default=0))))
for r in res: print(json.dumps(r))
