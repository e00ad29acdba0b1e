"""Batched MountainCar (counterpart of bsuite/environments/mountain_car.py; kernel: csrc/mountain_car_env.h on the skeleton of csrc/small_obs.h)."""
from typing import Optional

import torch

from bsuite_amd import _native
from bsuite_amd.environments import base

NUM_EPISODES = 1000  # bsuite/experiments/mountain_car/sweep.py:19


class MountainCar(base.Environment):
  """Mountain Car, an underpowered car must power up a hill (mountain_car.py:29-57)."""

  _info_keys = ('raw_return',)
  _info_pending_column = 'steps'            # the running episode's -t (bsx_bsuite_info)

  def __init__(self, max_steps: int = 1000, seed: Optional[int] = None, **engine_kwargs):
    if max_steps < 1:
      raise ValueError('max_steps must be >= 1')
    super().__init__(obs_shape=(1, 3), num_actions=3, seed=seed, **engine_kwargs)
    self._max_steps = max_steps
    self._cfg = _native.MountainCarCfg(max_steps, 0)
    self.bsuite_num_episodes = NUM_EPISODES

  def _state_tensors(self):
    return dict(state=torch.zeros((2, self._batch), dtype=torch.float32, device=self._device),
                steps=torch.full((self._batch,), 1 << 30, dtype=torch.int32, device=self._device))

  _abi_name = 'mountain_car'
  _linear_eval_abi = 'bsx_mountain_car_linear_evaluate'
  _mlp_eval_abi = 'bsx_mountain_car_mlp_evaluate'
  _linear_rollout_abi = 'bsx_mountain_car_linear_rollout'
  _mlp_rollout_abi = 'bsx_mountain_car_mlp_rollout'
  _mlp2_eval_abi = 'bsx_mountain_car_mlp2_evaluate'
  _mlp2_rollout_abi = 'bsx_mountain_car_mlp2_rollout'
  _linear_sample_abi = 'bsx_mountain_car_linear_sample'
  _mlp_sample_abi = 'bsx_mountain_car_mlp_sample'
  _linear_sample_eval_abi = 'bsx_mountain_car_linear_sample_evaluate'
  _mlp_sample_eval_abi = 'bsx_mountain_car_mlp_sample_evaluate'
  _mlp2_sample_abi = 'bsx_mountain_car_mlp2_sample'
  _mlp2_sample_eval_abi = 'bsx_mountain_car_mlp2_sample_evaluate'

  def _pending_info(self):
    # every step pays -1 (mountain_car.py:75-76): a running episode of t steps has earned -t; the
    # kernel folds it into raw_return when the episode ends (csrc/mountain_car_env.h)
    steps = self._state['steps']
    running = (steps & (1 << 30)) == 0
    return {0: -torch.where(running, steps & 0x3FFFFFFF, torch.zeros_like(steps)).to(torch.float64)}
