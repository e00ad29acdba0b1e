"""Batched MemoryChain (counterpart of bsuite/environments/memory_chain.py; kernel: csrc/memory_chain_env.h on the skeleton of csrc/small_obs.h)."""
from typing import Optional

import torch

from bsuite_amd import _native
from bsuite_amd.environments import base


class MemoryChain(base.Environment):
  """Context bits at t=0, query at t=L-1, answer rewarded on the last step (memory_chain.py:34-58)."""

  _info_keys = ('total_perfect', 'total_regret')
  _info_int_keys = ('total_perfect',)

  def __init__(self, memory_length: int, num_bits: int = 1, seed: Optional[int] = None,
               **engine_kwargs):
    if memory_length < 1 or not 1 <= num_bits <= 62:
      raise ValueError('memory_length must be >= 1 and num_bits in [1, 62]')
    super().__init__(obs_shape=(1, num_bits + 2), num_actions=2, seed=seed, **engine_kwargs)
    self._memory_length = memory_length
    self._num_bits = num_bits
    self._cfg = _native.MemoryChainCfg(memory_length, num_bits)
    self.bsuite_num_episodes = 10_000  # Overridden by experiment load() (memory_chain.py:58).

  def _mt_constructor_draws(self, rs):
    rs.binomial(1, 0.5, self._num_bits)      # memory_chain.py:49
    rs.randint(self._num_bits)               # memory_chain.py:50

  def _state_tensors(self):
    return dict(state=torch.full((self._batch,), 1 << 28, dtype=torch.int32, device=self._device),
                context=torch.zeros(self._batch, dtype=torch.int64, device=self._device))

  _abi_name = 'memory_chain'
