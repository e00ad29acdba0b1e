"""Measurements of the per-lane reset (profiles/lane_reset/README.md), 2^20 lanes unless --lanes says otherwise.

  python tools/lane_reset_bench.py plain  [--steps N] [--reps R]     step(a) of deep_sea/10, catch/0, cartpole/0: us per step
  python tools/lane_reset_bench.py closed [--steps N] [--reps R]     cartpole/0, catch/0: step(a) against step(a, reset_mask=m),
                                                                    density 1/64, alternated in one process
  python tools/lane_reset_bench.py marks  [--steps N]                every family x densities 0, 1/64, 1/2, 1: N x {mark_reset(m);
                                                                    step(a)} per segment, segments separated by one calib_fill
                                                                    launch — run it under `rocprofv3 --kernel-trace` and give
                                                                    the trace to `segments`
  python tools/lane_reset_bench.py segments <kernel_trace.csv>       average us of every kernel per (family, density) segment

`plain` uses nothing this feature added, so it also runs on an older tree (A/B of two checkouts in one GPU visit: only
numbers of one visit compare, boxes differ by +-5 %).  One JSON line per result on stdout.
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.environ.get('BSX_BENCH_TREE'):       # A/B: measure the package of another checkout
  ROOT = os.environ['BSX_BENCH_TREE']
sys.path.insert(0, ROOT)

PLAIN_IDS = ('deep_sea/10', 'catch/0', 'cartpole/0')
MARK_IDS = ('deep_sea/10', 'deep_sea_stochastic/0', 'catch/0', 'bandit/0', 'memory_len/0', 'umbrella_length/0',
            'discounting_chain/0', 'cartpole/0', 'cartpole_swingup/0', 'mountain_car/0', 'mnist/0')
DENSITIES = (0.0, 1.0 / 64, 0.5, 1.0)


def _env(bsuite_id, lanes):
  import warnings
  import bsuite_amd
  kw = {}
  if bsuite_id.startswith('mnist'):
    import numpy as np
    rng = np.random.default_rng(7)         # a stand-in dataset in the table's format (no dataset files on the box)
    kw = dict(images=rng.integers(-128, 128, size=(96, 28, 28), dtype=np.int8), labels=rng.integers(0, 10, size=96).astype(np.uint8))
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    return bsuite_amd.load_from_id(bsuite_id, batch=lanes, seed=1, **kw)


def _actions(env, lanes, n=8):
  import torch
  na = env.action_spec().num_values
  g = torch.Generator(device='cuda').manual_seed(0)
  return [torch.randint(0, na, (lanes,), generator=g, device='cuda', dtype=torch.int32) for _ in range(n)]


def _time(fn, steps):
  import torch
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for s in range(steps):
    fn(s)
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / steps * 1e6


def plain(args):
  for bsuite_id in PLAIN_IDS:
    env = _env(bsuite_id, args.lanes)
    acts = _actions(env, args.lanes)
    step = lambda s: env.step(acts[s & 7])
    _time(step, 50)
    us = [round(_time(step, args.steps), 3) for _ in range(args.reps)]
    print(json.dumps(dict(mode='plain', tree=ROOT, bsuite_id=bsuite_id, lanes=args.lanes, steps=args.steps, us_per_step=us)), flush=True)
    del env


def closed(args):
  import torch
  for bsuite_id in ('cartpole/0', 'catch/0'):
    env = _env(bsuite_id, args.lanes)
    acts = _actions(env, args.lanes)
    g = torch.Generator(device='cuda').manual_seed(1)
    masks = [torch.rand(args.lanes, generator=g, device='cuda') < 1.0 / 64 for _ in range(8)]
    step = lambda s: env.step(acts[s & 7])
    masked = lambda s: env.step(acts[s & 7], reset_mask=masks[s & 7])
    _time(step, 50), _time(masked, 50)
    a, b = [], []
    for _ in range(args.reps):               # alternated: plain, masked, plain, masked, ...
      a.append(round(_time(step, args.steps), 3))
      b.append(round(_time(masked, args.steps), 3))
    print(json.dumps(dict(mode='closed', bsuite_id=bsuite_id, lanes=args.lanes, steps=args.steps, density=1.0 / 64,
                          us_per_step_plain=a, us_per_step_masked=b)), flush=True)
    del env


def marks(args):
  import torch
  from bsuite_amd import _native
  sep = torch.zeros(1024, dtype=torch.float32, device='cuda')
  stream = lambda: torch.cuda.current_stream().cuda_stream
  order = []
  for bsuite_id in MARK_IDS:
    env = _env(bsuite_id, args.lanes)
    acts = _actions(env, args.lanes)
    g = torch.Generator(device='cuda').manual_seed(2)
    masks = {d: [torch.rand(args.lanes, generator=g, device='cuda') < d for _ in range(4)] for d in DENSITIES}
    _native.check(_native.lib.bsx_calib_fill(sep.data_ptr(), 4096, 0, stream()), 'separator')
    for s in range(20):                      # warm-up: a segment of its own, dropped by `segments`
      env.step(acts[s & 7])
    order.append([bsuite_id, 'warmup'])
    torch.cuda.synchronize()
    for d in DENSITIES:
      _native.check(_native.lib.bsx_calib_fill(sep.data_ptr(), 4096, 0, stream()), 'separator')
      for s in range(args.steps):
        env.mark_reset(masks[d][s & 3])
        env.step(acts[s & 7])
      order.append([bsuite_id, d])
    torch.cuda.synchronize()
    del env
  print(json.dumps(dict(mode='marks', lanes=args.lanes, steps=args.steps, segments=order)), flush=True)


def segments(args):
  """Kernel trace of a `marks` run -> average us of every kernel per segment (dispatches in start order; a calib_fill
  launch opens each segment; each family's warm-up segment is dropped, as are torch's own kernels)."""
  order = [(i, d) for i in MARK_IDS for d in ('warmup',) + DENSITIES]
  rows = []
  with open(args.trace) as f:
    for r in csv.DictReader(f):
      rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
  rows.sort()
  seg = -1
  acc = {}
  for t0, t1, name in rows:
    if 'calib_fill_kernel' in name:
      seg += 1
      continue
    if seg < 0 or seg >= len(order) or name.startswith(('void at::', 'at::')):
      continue
    short = name.split('(')[0]
    n, tot = acc.get((seg, short), (0, 0))
    acc[(seg, short)] = (n + 1, tot + (t1 - t0))
  assert seg + 1 == len(order), (seg + 1, len(order))
  for (s, short), (n, tot) in sorted(acc.items()):
    if order[s][1] == 'warmup':
      continue
    print(json.dumps(dict(bsuite_id=order[s][0], density=order[s][1], kernel=short, calls=n, avg_us=round(tot / n / 1e3, 3))))


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('mode', choices=('plain', 'closed', 'marks', 'segments'))
  ap.add_argument('trace', nargs='?')
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--steps', type=int, default=300)
  ap.add_argument('--reps', type=int, default=3)
  a = ap.parse_args()
  dict(plain=plain, closed=closed, marks=marks, segments=segments)[a.mode](a)
