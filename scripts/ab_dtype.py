#!/usr/bin/env python3
"""A/B of the timed step between dtypes inside ONE process on one box: an f64 and an 'f32x' context (the exact form with fp32 products) on the same
problem, alternated at least three times.  Per visit: `regions` timed regions of `steps` steps with no HIP event inside them (the step, as
bench.py times it), then the same regions once more with the two HIP events around the ordinate + row product kernel alone
(jx_timing_enable(2): the producer; a pair of events also spans the command processor's hand-over, see jx_event_bracket_time).  Printed per
visit: median and minimum step, median producer; at the end per dtype the median over visits, the spread between visits (max - min of
their medians), and whether the difference between the dtypes clears five times the larger spread.

    python3 scripts/ab_dtype.py --side 512 --points 500 --walkers 1024
    python3 scripts/ab_dtype.py --side 1024 --points 1000 --walkers 8192 --steps 60      (GPU box; run each under its own timeout)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from joxsz_amd import datasets                                      # noqa: E402
from joxsz_amd.posterior import JoxszPosterior                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--side', type=int, default=512)
ap.add_argument('--points', type=int, default=500)
ap.add_argument('--walkers', type=int, default=1024)
ap.add_argument('--steps', type=int, default=300)
ap.add_argument('--regions', type=int, default=9)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--dtypes', default='f64,f32x')
args = ap.parse_args()
assert args.rounds >= 3

W = args.walkers
pb = datasets.synthetic_problem(S=args.side, N=args.points, seed=0)
big = np.ascontiguousarray(datasets.walker_ball(pb, W, spread=0.03, seed=1))
dtypes = args.dtypes.split(',')
posts = {}
for dt in dtypes:
    post = JoxszPosterior(pb, device=0, max_batch=W, dtype=dt)
    c = post.ctx
    assert c.chunk >= W, 'the launch sequence is split: chunk %d < %d walkers' % (c.chunk, W)
    tp, lp = c.dev_alloc(big.nbytes), c.dev_alloc(8 * W)
    c.h2d(tp, big)
    for _ in range(20):
        c.eval_device(tp, W, lp)
    c.sync()
    out = np.empty(W)
    c.d2h(out, lp)
    posts[dt] = (post, tp, lp, out)
    print('%-5s %s | %s | chunk %d | %d of %d walkers finite' % (dt, c.conv_layout, c.exact_info(), c.chunk, int(np.isfinite(out).sum()), W), flush=True)
if len(dtypes) == 2:
    a, b = posts[dtypes[0]][3], posts[dtypes[1]][3]
    fin = np.isfinite(a)
    assert np.array_equal(np.isfinite(b), fin)
    rel = np.abs(a[fin] - b[fin]) / np.abs(a[fin])
    print('log-posterior %s against %s over %d walkers: relative difference max %.3e median %.3e' % (dtypes[1], dtypes[0], int(fin.sum()), rel.max(), np.median(rel)), flush=True)


def visit(dt):
    post, tp, lp, _ = posts[dt]
    c = post.ctx
    c.timing_enable(False)
    for _ in range(10):
        c.eval_device(tp, W, lp)
    c.sync()
    us = []
    for _ in range(args.regions):
        t = time.perf_counter()
        for _ in range(args.steps):
            c.eval_device(tp, W, lp)
        c.sync()
        us.append((time.perf_counter() - t) / args.steps * 1e6)
    prod = []
    c.timing_enable(2)
    for _ in range(args.regions):
        c.timing_reset()
        for _ in range(args.steps):
            c.eval_device(tp, W, lp)
        c.sync()
        tm = c.timing()
        prod.append(1e3 * tm['abel_map_ms'] / max(1, tm['launches']))
    c.timing_enable(False)
    return float(np.median(us)), float(min(us)), float(np.median(prod))


res = {dt: [] for dt in dtypes}
for rnd in range(args.rounds):
    for dt in dtypes:
        r = visit(dt)
        res[dt].append(r)
        print('visit %d %-5s step median %.2f us  min %.2f us | producer median %.2f us' % ((rnd, dt) + r), flush=True)
summ = {}
for dt in dtypes:
    st, pr = np.array([r[0] for r in res[dt]]), np.array([r[2] for r in res[dt]])
    summ[dt] = (float(np.median(st)), float(st.max() - st.min()), float(np.median(pr)), float(pr.max() - pr.min()))
    print('%-5s %d^2 / %d points / %d walkers: step %.2f us (spread between visits %.2f) | producer %.2f us (spread %.2f) | %.4f ms per 1024 walkers' % (
        (dt, args.side, args.points, W) + summ[dt] + (summ[dt][0] * 1e-3 * 1024 / W,)), flush=True)
if len(dtypes) == 2:
    a, b = summ[dtypes[0]], summ[dtypes[1]]
    for what, k in (('step', 0), ('producer', 2)):
        d, sp = b[k] - a[k], max(a[k + 1], b[k + 1])
        print('%s: %s - %s = %+.2f us (%+.1f %%), five times the spread = %.2f us: %s' % (what, dtypes[1], dtypes[0], d, 100 * d / a[k], 5 * sp,
                                                                                       'clears it' if abs(d) > 5 * sp else 'does not clear it'), flush=True)
for dt in dtypes:
    posts[dt][0].close()
