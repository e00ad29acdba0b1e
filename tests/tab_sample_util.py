"""What the CPU and the GPU tests of sample_policy / evaluate_sampled_policy share: the rule of bsx_gumbel_select_n
(bsuite_amd/csrc/bsx_tab_sample.h) restated in numpy, one rounding per operation (numpy never fuses a multiply into an add),
and the frequency case — the lanes, seeds and call indices at which the CPU test holds the restatement's action counts against
the softmax and the GPU test holds the device's counts against the restatement's, exactly."""
import numpy as np

from oracle import stream

STREAM_SAMPLE = 3


def np_log(x):
  """bsx_log restated from its specification (include/bsx_stream.h): exponent and mantissa from the bits, m into
  [~0.707, 1.414], s = (m - 1) / (m + 1), 2 atanh(s) as the odd series to s^25 by Horner's rule."""
  x = np.ascontiguousarray(x, np.float64)
  u = x.view(np.uint64)
  e = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
  m = ((u & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
  big = m > 1.4142135623730951
  m = np.where(big, m * 0.5, m)
  e = np.where(big, e + 1, e)
  s = (m - 1.0) / (m + 1.0)
  s2 = s * s
  p = np.full_like(s, 1.0 / 25.0)
  for d in range(23, 1, -2):
    p = p * s2
    p = p + 1.0 / d
  p = p * s2
  p = p + 1.0
  lm = 2.0 * s
  lm = lm * p
  return e.astype(np.float64) * 0.6931471805599453 + lm


def np_noise(words):
  u = (np.asarray(words, np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32
  return -np_log(-np_log(u))


def np_scores(logits, words, beta):
  """z [n, A] = float64(l) * beta + g: a multiply, then an add."""
  with np.errstate(all='ignore'):
    scaled = np.asarray(logits, np.float32).astype(np.float64) * np.asarray(beta, np.float64).reshape(-1, 1)
    return scaled + np_noise(words)


def np_argmax(z):
  """best = 0; a = 1 .. A-1 wins only with z_a > z_best."""
  best, z_best = np.zeros(z.shape[0], np.int32), z[:, 0].copy()
  with np.errstate(all='ignore'):
    for a in range(1, z.shape[1]):
      better = z[:, a] > z_best
      best = np.where(better, np.int32(a), best)
      z_best = np.where(better, z[:, a], z_best)
  return best


def np_select(logits, words, beta):
  logits = np.asarray(logits, np.float32)
  return np_argmax(np_scores(logits, words, np.broadcast_to(np.asarray(beta, np.float64), (logits.shape[0],))))


# ---------------------------------------------------------------------------------------------- the frequency case
# A fresh batch of B lanes from lane LANE0 on, one call of T steps (call indices 0 .. T-1), temperature 1, every row of the
# table the same: (0, ln 3) for two actions — P = (1/4, 3/4) — and (0, ln 2, ln 4) for three — P = (1/7, 2/7, 4/7).  The
# action of a step that does not reset does not depend on the state then, so the counts over the live steps are a function of
# the draws alone.  LIVE: the call indices at which no lane resets — deep_sea size 4 restarts every 5th call (FIRST at 0, 5,
# 10), catch 10 x 5 every 10th (FIRST at 0, 10).
# The sample seeds were picked as the first of 0, 1, 2, ... at which every action's frequency lies within 4 sigma of the
# softmax (sigma = sqrt(p (1 - p) / N)); test_tab_sample_host.py re-checks that they do and prints the deviations.
FREQ_B, FREQ_T, FREQ_LANE0 = 4096, 11, (1 << 32) - 17
FREQ_ROW = {2: (0.0, float(np.log(3.0))), 3: (0.0, float(np.log(2.0)), float(np.log(4.0)))}
FREQ_LIVE = {2: (1, 2, 3, 4, 6, 7, 8, 9), 3: (1, 2, 3, 4, 5, 6, 7, 8, 9)}
FREQ_SEED = {2: 0, 3: 0}
FREQ_FAMILY = {2: ('deep_sea', dict(size=4, mapping_seed=42)), 3: ('catch', dict())}


def freq_row(A):
  return np.asarray(FREQ_ROW[A], np.float64).astype(np.float32)


def restated_actions(A, seed=None):
  """int32 [len(FREQ_LIVE[A]), FREQ_B]: the restatement's action of every lane at every live call index."""
  seed = FREQ_SEED[A] if seed is None else seed
  lanes = np.uint64(FREQ_LANE0) + np.arange(FREQ_B, dtype=np.uint64)
  logits = np.ascontiguousarray(np.broadcast_to(freq_row(A), (FREQ_B, A)))
  return np.stack([np_select(logits, stream.words(seed, lanes, t, STREAM_SAMPLE, A), 1.0) for t in FREQ_LIVE[A]])


def restated_counts(A, seed=None):
  return np.bincount(restated_actions(A, seed).reshape(-1), minlength=A)
