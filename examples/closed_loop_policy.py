"""Closed loop on the device: a batched environment stepped by a (random-weight) linear policy that
reads the observation tensor the engine just wrote — no host round trip anywhere in the loop.

    python examples/closed_loop_policy.py [bsuite_id] [lanes] [steps] [--observation-dtype float32|uint8|float16|bfloat16]

With a narrow --observation-dtype (deep_sea, catch) the engine writes the boards as bytes or 16-bit floats, and the policy
converts each board once, as it reads it: to float32 from uint8, not at all from float16 / bfloat16, whose weights and
matrix product stay in that type.

This is the batched counterpart of the reference run loop (bsuite/baselines/experiment.py:43-57):
`timestep = env.step(agent.select_action(timestep))`, with 2^20 environments per call.
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
  ap.add_argument('bsuite_id', nargs='?', default='deep_sea/10')
  ap.add_argument('lanes', nargs='?', type=int, default=1 << 20)
  ap.add_argument('steps', nargs='?', type=int, default=200)
  ap.add_argument('--observation-dtype', default='float32', choices=('float32', 'uint8', 'float16', 'bfloat16'))
  a = ap.parse_args()
  bsuite_id, lanes, steps = a.bsuite_id, a.lanes, a.steps
  env = bsuite_amd.load_from_id(bsuite_id, batch=lanes, seed=0, observation_dtype=a.observation_dtype)
  n_obs = int(torch.tensor(env.observation_spec().shape).prod())
  n_act = env.action_spec().num_values
  compute = env.observation_dtype if env.observation_dtype.is_floating_point else torch.float32
  g = torch.Generator(device='cuda').manual_seed(0)
  weights = torch.randn((n_obs, n_act), device='cuda', generator=g).to(compute)

  def policy(timestep):                           # greedy over a linear read-out of the observation
    board = timestep.observation.reshape(lanes, n_obs).to(compute)      # the one conversion (none for a float board)
    logits = board @ weights
    return logits.argmax(dim=1).to(torch.int32)

  ts = env.reset()
  for _ in range(20):
    ts = env.step(policy(ts))
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(steps):
    ts = env.step(policy(ts))
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  info = {k: float(v.sum()) for k, v in env.bsuite_info().items()}
  print(json.dumps(dict(bsuite_id=bsuite_id, observation_dtype=a.observation_dtype, lanes=lanes, steps=steps, ms_per_step=round(dt / steps * 1e3, 4),
                        env_steps_per_s=round(lanes * steps / dt), episodes_finished=int(env.episode_counters()[0]),
                        bsuite_info_sums=info)))


if __name__ == '__main__':
  main()
