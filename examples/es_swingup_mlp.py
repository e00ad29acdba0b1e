"""An evolution-strategies loop on cartpole_swingup whose whole inner loop — a population of one-hidden-layer policies,
each run on its own group of lanes for T closed-loop steps — is ONE launch per generation: `env.evaluate_mlp`.

    python examples/es_swingup_mlp.py [--population 256] [--lanes-per-policy 64] [--hidden 16] [--steps 200] [--generations 5]

Generation g perturbs the current mean pair (w1 [H, 9], w2 [3, H+1]) with antithetic Gaussian noise, marks every lane for a
reset, scores the P perturbed pairs in one call — lanes grouped by policy (policy_index = lane // lanes_per_policy), the
layout evaluate_mlp reads fastest — and moves the mean along the noise weighted by the centred ranks of the scores.  A
policy's score is the sum of rewards of its lanes over the T steps (`return_sum`), reduced on the device with index_add_.

It is an example of the call, not a tuned learner: it prints each generation's mean and best score and makes no claim about
what they reach.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
import bsuite_amd  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--population', type=int, default=256, help='perturbed pairs per generation (even: antithetic)')
  ap.add_argument('--lanes-per-policy', type=int, default=64)
  ap.add_argument('--hidden', type=int, default=16)
  ap.add_argument('--steps', type=int, default=200)
  ap.add_argument('--generations', type=int, default=5)
  ap.add_argument('--sigma', type=float, default=0.1)
  ap.add_argument('--lr', type=float, default=0.05)
  a = ap.parse_args()
  if a.population < 2 or a.population % 2:
    ap.error('--population must be even and at least 2')
  dev = torch.device('cuda:0')
  P, H, B = a.population, a.hidden, a.population * a.lanes_per_policy
  env = bsuite_amd.load_from_id('cartpole_swingup/0', batch=B, device=dev, seed=0)
  D = env.observation_spec().shape[-1]
  g = torch.Generator(device=dev).manual_seed(0)
  mean1 = torch.randn((H, D + 1), generator=g, device=dev) * 0.1
  mean2 = torch.randn((3, H + 1), generator=g, device=dev) * 0.1
  policy_index = (torch.arange(B, device=dev) // a.lanes_per_policy).to(torch.int32)
  rows = policy_index.long()
  obs = env.reset().observation                      # (every lane is marked below: its row is never read)
  everyone = torch.ones(B, dtype=torch.bool, device=dev)
  for gen in range(a.generations):
    n1 = torch.randn((P // 2, H, D + 1), generator=g, device=dev)
    n2 = torch.randn((P // 2, 3, H + 1), generator=g, device=dev)
    n1, n2 = torch.cat([n1, -n1]), torch.cat([n2, -n2])
    w1, w2 = (mean1 + a.sigma * n1).contiguous(), (mean2 + a.sigma * n2).contiguous()
    env.mark_reset(everyone)                         # every generation scores whole episodes from their first step
    t0 = time.perf_counter()
    ev = env.evaluate_mlp(w1, w2, obs, a.steps, policy_index=policy_index)
    score = torch.zeros(P, dtype=torch.float64, device=dev).index_add_(0, rows, ev.return_sum) / a.lanes_per_policy
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    obs = ev.observation
    rank = score.argsort().argsort().to(torch.float32) / (P - 1) - 0.5               # centred ranks in [-0.5, 0.5]
    mean1 += a.lr / a.sigma * (rank.view(P, 1, 1) * n1).mean(dim=0)
    mean2 += a.lr / a.sigma * (rank.view(P, 1, 1) * n2).mean(dim=0)
    print(json.dumps(dict(generation=gen, mean_score=float(score.mean()), best_score=float(score.max()), lanes=B, steps=a.steps,
                          seconds=round(dt, 4), env_steps_per_s=round(B * a.steps / dt))))


if __name__ == '__main__':
  main()
