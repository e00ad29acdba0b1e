"""lambda_returns / td_lambda (one launch of csrc/returns.hip) against the loop they replace — utils.returns.torch_scan, the
definition in separate torch operations, run on the same device tensors: T iterations of about a dozen small launches, which
is what a user of the [T,B] layout wrote before the call existed.  One process, one JSON line per (shape, mode, variant).

  python tools/bench_returns.py [--shapes 1048576x32,16384x1000] [--kernel-calls 200] [--loop-calls 4] [--reps 5]
                                [--kernel-only] [--out FILE]

Shapes are BxT.  Modes: `returns` = lambda_returns without values (reads reward, discount, step_type; writes returns: 13 bytes
per element) and `td` = td_lambda (reads values [T+1,B] too, writes td_errors too: 21 bytes per element + 4 B).  The trajectory is
synthesised with the episode structure of a recorded catch rollout: episodes of 9 transitions behind a FIRST row, each lane at
its own phase, reward 0 on FIRST rows, discount 0 on LAST rows.  gamma = 0.99, lambda = 0.9.
Variants, alternated inside each repetition: `kernel` and `loop`.  Per row: every repetition's us per call on HIP events
(`us_reps`, in the order measured), their median, the algorithmic bytes per call and GB/s; for the kernel that rate as a
fraction of this box's copy rate (bsx_calib_copy, one read and one write per 16 bytes, measured in the same run); then
loop / kernel per repetition.  --kernel-only skips the loop and is what the A/B of the tuning build's knobs
(BSX_NATIVE_LIB=.../libbsuite_amd_tuning.so BSX_RETURNS_POLICY=0..3 BSX_RETURNS_AHEAD=4|8|16, read once per process) runs.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

GAMMA, LAMBDA, EPISODE = 0.99, 0.9, 9


def synthesise(torch, T, B, dev, seed=0):
  g = torch.Generator(device=dev).manual_seed(seed)
  phase = torch.randint(0, EPISODE + 1, (B,), generator=g, device=dev)
  pos = (torch.arange(T, device=dev)[:, None] + phase[None, :]) % (EPISODE + 1)           # 0 = FIRST, EPISODE = LAST
  step_type = torch.where(pos == 0, 0, torch.where(pos == EPISODE, 2, 1)).to(torch.int8)
  reward = torch.randn((T, B), generator=g, device=dev) * (pos != 0)
  discount = (pos != EPISODE).to(torch.float32)
  values = torch.randn((T + 1, B), generator=g, device=dev)
  return reward.contiguous(), discount.contiguous(), step_type.contiguous(), values.contiguous()


def copy_rate(torch, dev, n=1 << 30):
  """(R + W) bytes per second of bsx_calib_copy with one store per load, in GB/s."""
  from bsuite_amd import _native  # pylint: disable=import-outside-toplevel
  src = torch.empty(n, dtype=torch.uint8, device=dev)
  dst = torch.empty(n, dtype=torch.uint8, device=dev)
  st = torch.cuda.current_stream(dev).cuda_stream
  for _ in range(3):
    _native.check(_native.lib.bsx_calib_copy(dst.data_ptr(), src.data_ptr(), n, 1, st), 'bsx_calib_copy')
  c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  c0.record()
  for _ in range(10):
    _native.lib.bsx_calib_copy(dst.data_ptr(), src.data_ptr(), n, 1, st)
  c1.record()
  torch.cuda.synchronize(dev)
  return 2 * n * 10 / (c0.elapsed_time(c1) * 1e-3) / 1e9


def _time(torch, run, calls):
  ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  ev0.record()
  for _ in range(calls):
    run()
  ev1.record()
  torch.cuda.synchronize()
  return ev0.elapsed_time(ev1) * 1e3 / calls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='1048576x32,16384x1000')
  ap.add_argument('--kernel-calls', type=int, default=200)
  ap.add_argument('--loop-calls', type=int, default=4)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--kernel-only', action='store_true')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  import torch  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import returns as R  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_returns.py measures on the GPU; none is visible')
  dev = torch.device('cuda:0')
  out = open(a.out, 'a') if a.out else None
  knobs = {k: os.environ[k] for k in ('BSX_NATIVE_LIB', 'BSX_RETURNS_POLICY', 'BSX_RETURNS_AHEAD') if k in os.environ}
  knobs['BSX_NATIVE_LIB'] = os.path.basename(knobs['BSX_NATIVE_LIB']) if 'BSX_NATIVE_LIB' in knobs else None

  def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if out:
      out.write(line + '\n')
      out.flush()

  copy = None if a.kernel_only else copy_rate(torch, dev)
  for shape in a.shapes.split(','):
    B, T = (int(x) for x in shape.split('x'))
    reward, discount, step_type, values = synthesise(torch, T, B, dev)
    ret, td = torch.empty_like(reward), torch.empty_like(reward)
    for mode in ('returns', 'td'):
      n_bytes = T * B * 13 if mode == 'returns' else T * B * 21 + 4 * B
      if mode == 'returns':
        kernel = lambda: R.lambda_returns(reward, discount, gamma=GAMMA, lambda_=LAMBDA, step_type=step_type, out=ret)
        loop = lambda: R.torch_scan(reward, discount, gamma=GAMMA, lambda_=LAMBDA, step_type=step_type, out=ret)
      else:
        kernel = lambda: R.td_lambda(reward, discount, values, gamma=GAMMA, lambda_=LAMBDA, step_type=step_type)
        loop = lambda: R.torch_scan(reward, discount, values, gamma=GAMMA, lambda_=LAMBDA, step_type=step_type, want_td=True)
      runs = {'kernel': (kernel, a.kernel_calls)}
      if not a.kernel_only:
        runs['loop'] = (loop, a.loop_calls)
      # the two compute the same numbers (checked once per mode, outside the timed windows) ...
      got = kernel()
      got = (got, None) if mode == 'returns' else (got.returns, got.td_errors)
      got = tuple(None if x is None else x.clone() for x in got)
      want = loop()
      for x, y in zip(got, want):
        if x is not None and not torch.equal(x.view(torch.int32), y.view(torch.int32)):
          raise SystemExit(f'{shape} {mode}: the kernel and the torch loop differ')
      for run, _ in runs.values():                                           # ... and both are warm
        for _ in range(3):
          run()
      order = tuple(runs)
      samples = {v: [] for v in order}
      for rep in range(a.reps):
        for v in (order if rep % 2 == 0 else order[::-1]):
          samples[v].append(_time(torch, *runs[v]))
      case = dict(lanes=B, T=T, mode=mode, gamma=GAMMA, lambda_=LAMBDA, bytes_per_call=n_bytes, **knobs)
      for v in order:
        us = statistics.median(samples[v])
        row = dict(case, variant=v, calls=runs[v][1], us_per_call=us, us_reps=samples[v], gb_per_s=n_bytes / (us * 1e-6) / 1e9, reps=a.reps)
        if v == 'kernel' and copy is not None:
          row.update(copy_gb_per_s=copy, fraction_of_copy_rate=row['gb_per_s'] / copy)
        emit(bench.sig(row))
      if 'loop' in runs:
        emit(bench.sig(dict(case, variant='ratio', loop_over_kernel_reps=[x / y for x, y in zip(samples['loop'], samples['kernel'])])))
    del reward, discount, step_type, values, ret, td
    torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
