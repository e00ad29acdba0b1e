"""evaluate_mlp2 / rollout_mlp2 against the only way the policy ran before them, and against their neighbours — one process:
cartpole, cartpole_swingup and mountain_car at 2^20 lanes, T = 32, one JSON line per (workload, policy, variant).

  python tools/bench_mlp2.py [--lanes 1048576] [--T 32] [--steps 256] [--eager-steps 32] [--reps 3] [--out FILE]
  python tools/bench_mlp2.py --wrapped-step [--root TREE --label parent] [--out FILE]     # the eager wrapped step of catch and deep_sea

Policies: `s64` (one shared 64 x 64 triple), `s16` (one shared 16 x 16 triple), `pop16` (a population of --population
16 x 16 triples, policy_index = lane * P // B: the lanes of a wave name one triple).
Variants, alternated inside each repetition (each has its own resident environment, warmed up past its first resets):
  eager       obs -> mlp2_select(obs) -> step(a), step by step: how this policy ran before these calls (the yardstick);
  evaluate    evaluate_mlp2 with the same arguments;
  fused       rollout_mlp2, the last observation passed back in;
  mlp64_eval  evaluate_mlp with one hidden layer of 64 units  \\  for context only: the neighbouring calls
  mlp64_roll  rollout_mlp  with one hidden layer of 64 units   >  (s64 rows only)
  open_loop   rollout(actions), a [T,B] action tensor made beforehand  /
Per row: every repetition's us per step on HIP events (`us_event_reps`, in the order measured), their median, env-steps/s,
and for the two new calls the fraction of the fp32 vector rate that 2 H1 H2 + 2 H1 (D + 1) + 6 H2 operations per lane-step
imply (--peak-tflops, default 157.3: 256 CUs x 128 lanes x 2 ops x 2.4 GHz); then eager / fused and eager / evaluate per
repetition.

--wrapped-step times what paid for the new kernel, the wrapped lane advance of deep_sea (one kernel for both draw
streams): the eager step of catch (catch_noise/0) and of deep_sea under RewardNoise at 2^20 lanes — and, because those two
boards are small enough for the one-launch fused step, of deep_sea N = 20 and of both families with index observations,
whose steps launch the lane advance itself (--envs).  --root names the tree whose package is imported (a checkout of the parent commit with its own library): run the two trees alternately, process by
process, and compare."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN = dict(s64=(64, 64), s16=(16, 16), pop16=(16, 16))


def make_triples(torch, D, H1, H2, P, dev, seed=0):
  """w1 [P, H1, D+1], w2 [P, H2, H1+1], w3 [P, 3, H2+1]: Gaussian weights at the scale of a freshly initialised network
  (1 / sqrt(fan-in)), so that units of both layers switch on and off and all three actions occur."""
  g = torch.Generator(device=dev).manual_seed(seed)
  w1 = torch.randn((P, H1, D + 1), generator=g, device=dev) / (D + 1) ** 0.5
  w2 = torch.randn((P, H2, H1 + 1), generator=g, device=dev) / (H1 + 1) ** 0.5
  w3 = torch.randn((P, 3, H2 + 1), generator=g, device=dev) / (H2 + 1) ** 0.5
  return w1.contiguous(), w2.contiguous(), w3.contiguous()


def _time(torch, run, steps):
  ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  ev0.record()
  run(steps)
  ev1.record()
  torch.cuda.synchronize()
  return ev0.elapsed_time(ev1) * 1e3 / steps


def _sig(x, n=5):
  if isinstance(x, float):
    return float(f'{x:.{n}g}') if x == x and abs(x) != float('inf') else None
  if isinstance(x, dict):
    return {k: _sig(v, n) for k, v in x.items()}
  if isinstance(x, (list, tuple)):
    return [_sig(v, n) for v in x]
  return x


def wrapped_step(a, emit):
  """us per eager step of the two wrapped pair families, every repetition."""
  sys.path.insert(0, os.path.abspath(a.root) if a.root else ROOT)
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  from bsuite_amd.environments import catch, deep_sea  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import wrappers  # pylint: disable=import-outside-toplevel
  dev = torch.device('cuda:0')
  B = a.lanes
  noise = lambda env: wrappers.RewardNoise(env, noise_scale=0.1, seed=1)     # pylint: disable=unnecessary-lambda-assignment
  # the first two are one fused launch per step (boards of at most 128 cells); the others launch the lane advance on its
  # own: a board too large to fuse (advance + store stream), and index observations (advance + decode: no board at all)
  envs = dict(catch_noise=lambda: bsuite_amd.load_from_id('catch_noise/0', batch=B, device=dev, seed=42),
              deep_sea_noise=lambda: noise(deep_sea.DeepSea(size=10, seed=42, batch=B, device=dev)),
              deep_sea20_noise=lambda: noise(deep_sea.DeepSea(size=20, seed=42, batch=B, device=dev)),
              deep_sea_noise_index=lambda: noise(deep_sea.DeepSea(size=10, seed=42, batch=B, device=dev, observation_mode='index')),
              catch_noise_index=lambda: noise(catch.Catch(seed=42, batch=B, device=dev, observation_mode='index')))
  envs = {k: v for k, v in envs.items() if k in a.envs.split(',')}
  for name, make in envs.items():
    env = make()
    n_act = 3 if name.startswith('catch') else 2
    acts = torch.randint(n_act, (B,), generator=torch.Generator(device=dev).manual_seed(2), device=dev, dtype=torch.int32)
    env.reset()

    def run(n, env=env, acts=acts):
      for _ in range(n):
        env.step(acts)
    run(16)
    reps = [_time(torch, run, a.steps) for _ in range(a.reps)]
    emit(_sig(dict(mode='wrapped_step', tree=a.label, env=name, lanes=B, steps=a.steps,
                   us_event_reps=reps, us_per_step_event=statistics.median(reps))))
    del env, run
    torch.cuda.empty_cache()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--T', type=int, default=32)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--eager-steps', type=int, default=32)
  ap.add_argument('--population', type=int, default=1024)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--workloads', default='cartpole,cartpole_swingup,mountain_car')
  ap.add_argument('--policies', default='s64,s16,pop16')
  ap.add_argument('--variants', default='eager,evaluate,fused,mlp64_eval,mlp64_roll,open_loop')
  ap.add_argument('--peak-tflops', type=float, default=157.3)
  ap.add_argument('--wrapped-step', action='store_true')
  ap.add_argument('--root', default=None)
  ap.add_argument('--label', default='this')
  ap.add_argument('--envs', default='catch_noise,deep_sea_noise,deep_sea20_noise,deep_sea_noise_index,catch_noise_index')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  out = open(a.out, 'a') if a.out else None

  def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if out:
      out.write(line + '\n')
      out.flush()

  if a.wrapped_step:
    return wrapped_step(a, emit)
  sys.path.insert(0, ROOT)
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import observations  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_mlp2.py measures on the GPU; none is visible')
  dev = torch.device('cuda:0')
  kinds = a.variants.split(',')
  B, T = a.lanes, a.T
  n_fused = max(1, a.steps // T) * T
  for w in a.workloads.split(','):
    for policy in a.policies.split(','):
      H1, H2 = HIDDEN[policy]
      P = a.population if policy == 'pop16' else 1
      pidx = (torch.arange(B, device=dev, dtype=torch.int64) * P // B).to(torch.int32) if P > 1 else None
      runs, steps_of = {}, {}

      def fresh():
        env = bsuite_amd.load_from_id(w + '/0', batch=B, device=dev, seed=42)
        return env, env.observation_spec().shape[-1]

      env, D = fresh()
      triples = make_triples(torch, D, H1, H2, P, dev)
      pol = tuple(t[0].contiguous() for t in triples) if P == 1 else triples
      kw = dict(policy_index=pidx)
      if 'eager' in kinds:
        own = pol if P == 1 else tuple(t[pidx.long()] for t in pol)      # (gathered once: the loop is not charged for it)
        state = dict(obs=env.reset().observation)

        def eager(n, env=env, own=own, state=state):
          obs = state['obs']
          for _ in range(n):
            obs = env.step(observations.mlp2_select(*own, obs)).observation
          state['obs'] = obs

        runs['eager'], steps_of['eager'] = eager, a.eager_steps
        eager(4)
      for name, method, args in (('evaluate', 'evaluate_mlp2', pol), ('fused', 'rollout_mlp2', pol),
                                 ('mlp64_eval', 'evaluate_mlp', None), ('mlp64_roll', 'rollout_mlp', None)):
        if name not in kinds or (args is None and policy != 's64'):
          continue
        env, D = fresh()
        if args is None:
          w1, _, w3 = make_triples(torch, D, 64, 64, 1, dev)
          args, kw_ = (w1[0].contiguous(), w3[0].contiguous()), {}
        else:
          kw_ = kw
        state = dict(obs=env.reset().observation.clone())

        def closed(n, call=getattr(env, method), args=args, state=state, rec=method.startswith('rollout'), kw_=kw_):
          obs = state['obs']
          for _ in range(n // T):
            r = call(*args, obs, T, **kw_)
            obs = r[0].observation[-1] if rec else r.observation
          state['obs'] = obs

        runs[name], steps_of[name] = closed, n_fused
        closed(2 * T)                                                      # warm-up (allocates the outputs)
      if 'open_loop' in kinds and policy == 's64':
        env, _ = fresh()
        acts = torch.randint(3, (T, B), generator=torch.Generator(device=dev).manual_seed(2), device=dev, dtype=torch.int32)

        def open_loop(n, env=env, acts=acts):
          for _ in range(n // T):
            env.rollout(acts)

        runs['open_loop'], steps_of['open_loop'] = open_loop, n_fused
        open_loop(2 * T)
      order = tuple(runs)
      samples = {v: [] for v in order}
      for rep in range(a.reps):
        for v in (order if rep % 2 == 0 else order[::-1]):
          samples[v].append(_time(torch, runs[v], steps_of[v]))
      case = dict(workload=w, policy=policy, hidden=[H1, H2], population=P, T=T, lanes=B)
      ops = 2 * H1 * H2 + 2 * H1 * (D + 1) + 6 * H2
      for v in order:
        us = statistics.median(samples[v])
        row = dict(case, variant=v, steps=steps_of[v], us_per_step_event=us, us_event_reps=samples[v], env_steps_per_s=B / (us * 1e-6))
        if v in ('evaluate', 'fused'):
          row['policy_ops_per_lane_step'] = ops
          row['fraction_of_fp32_vector_rate'] = ops * B / (us * 1e-6) / (a.peak_tflops * 1e12)
        emit(_sig(row))
      for v in ('fused', 'evaluate'):
        if v in runs and 'eager' in runs:
          emit(_sig(dict(case, variant=v, eager_over_this_reps=[e / f for e, f in zip(samples['eager'], samples[v])])))
      del runs
      torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
