"""CPU: sample_linear / sample_mlp (fused softmax-policy trajectories of cartpole, swing-up and mountain_car;
bsx_<family>_linear_sample, bsx_<family>_mlp_sample) without a GPU — the rule the kernel compiles (bsuite_amd/csrc/bsx_gumbel.h,
through gcc) against a numpy float32 / float64 restatement with one rounding per operation and against
utils.observations.linear_logits / mlp_logits / gumbel_select; the accuracy of bsx_log on the arguments the rule gives it; the
distribution of the drawn actions; every refusal of the Python entry points, all before any GPU use; the C ABI's declarations,
bindings, exports and argument checks; and the built library: ONE new kernel inside the kernel budget, paid for by the two
launches of an mnist group that became one kernel, inside the resource conditions, with nothing that waits inside its loops."""
import ctypes
import fractions
import inspect
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import _native
from bsuite_amd.environments import base, cartpole, catch, mountain_car
from bsuite_amd.utils import observations, wrappers
from oracle import stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bsuite_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')
SHIM = os.path.join(ROOT, 'tests', 'csrc', 'gumbel_shim.c')
KINDS = ('linear', 'mlp')
ENTRY = {(fam, kind): f'bsx_{fam}_{kind}_sample' for fam in ('cartpole', 'mountain_car') for kind in KINDS}
DIMS = [3, 6, 8]
HIDDEN = [1, 5, 64]
BETAS = [0.25, 1.0, 4.0]
STREAM_SAMPLE = 3


# ------------------------------------------------------------------------------------------ bsx_gumbel.h, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('gumbel') / 'gumbel_shim.so')
  subprocess.check_call(['gcc', '-O2', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-shared', '-fPIC', SHIM, '-o', so])
  lib = ctypes.CDLL(so)
  P, I64, I32, U64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64
  for name, args in (('shim_linear', [I64, I32, P, P, P, P, P, P, P]), ('shim_mlp', [I64, I32, I32, P, P, P, P, P, P, P, P]),
                     ('shim_select', [I64, P, P, P, P, P]), ('shim_noise', [I64, P, P]), ('shim_log', [I64, P, P]),
                     ('shim_draws', [U64, U64, I64, U64, P])):
    getattr(lib, name).restype = None
    getattr(lib, name).argtypes = args
  lib.shim_stream_sample.restype = ctypes.c_uint32
  return lib


_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _shim_linear(lib, w, o, words, beta):
  w, o = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(o, np.float32)
  words, beta = np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(beta, np.float64)
  n, D = o.shape
  assert w.shape == (n, 3, D + 1) and words.shape == (n, 3) and beta.shape == (n,)
  logits, action, greedy = np.full((n, 3), 7.0, np.float32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
  lib.shim_linear(n, D, _ptr(w), _ptr(o), _ptr(words), _ptr(beta), _ptr(logits), _ptr(action), _ptr(greedy))
  return logits, action, greedy


def _shim_mlp(lib, w1, w2, o, words, beta):
  w1, w2, o = (np.ascontiguousarray(x, np.float32) for x in (w1, w2, o))
  words, beta = np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(beta, np.float64)
  n, H, D1 = w1.shape
  assert w2.shape == (n, 3, H + 1) and o.shape == (n, D1 - 1) and words.shape == (n, 3) and beta.shape == (n,)
  logits, action, greedy = np.full((n, 3), 7.0, np.float32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
  lib.shim_mlp(n, D1 - 1, H, _ptr(w1), _ptr(w2), _ptr(o), _ptr(words), _ptr(beta), _ptr(logits), _ptr(action), _ptr(greedy))
  return logits, action, greedy


def _shim_select(lib, logits, words, beta):
  logits, words = np.ascontiguousarray(logits, np.float32), np.ascontiguousarray(words, np.uint32)
  beta = np.ascontiguousarray(np.broadcast_to(beta, (logits.shape[0],)), np.float64)
  z, action = np.full(logits.shape, 7.0, np.float64), np.full(logits.shape[0], -1, np.int32)
  lib.shim_select(logits.shape[0], _ptr(logits), _ptr(words), _ptr(beta), _ptr(z), _ptr(action))
  return z, action


def _shim_log(lib, x):
  x = np.ascontiguousarray(x, np.float64)
  y = np.empty_like(x)
  lib.shim_log(len(x), _ptr(x), _ptr(y))
  return y


# the restatement: numpy, one rounding per operation (numpy never fuses a multiply into an add)
def _np_log(x):
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


def _np_noise(words):
  u = (np.asarray(words, np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32
  return -_np_log(-_np_log(u))


def _np_scores(logits, words, beta):
  with np.errstate(all='ignore'):
    scaled = np.asarray(logits, np.float32).astype(np.float64) * np.asarray(beta, np.float64).reshape(-1, 1)
    return scaled + _np_noise(words)


def _np_argmax(z):
  """best = 0; a = 1, 2 wins only with z_a > z_best."""
  best, z_best = np.zeros(z.shape[0], np.int32), z[:, 0].copy()
  with np.errstate(all='ignore'):
    for a in (1, 2):
      better = z[:, a] > z_best
      best = np.where(better, np.int32(a), best)
      z_best = np.where(better, z[:, a], z_best)
  return best


def _np_select(logits, words, beta):
  return _np_argmax(_np_scores(logits, words, beta))


def _np_linear_logits(w, o):
  w, o = np.asarray(w, np.float32), np.asarray(o, np.float32)
  D = o.shape[1]
  with np.errstate(all='ignore'):
    l = w[:, :, D].copy()
    for d in range(D):
      prod = w[:, :, d] * o[:, d:d + 1]
      l = l + prod
  return l


def _np_mlp_logits(w1, w2, o):
  w1, w2, o = (np.asarray(x, np.float32) for x in (w1, w2, o))
  H, D = w1.shape[1], o.shape[1]
  with np.errstate(all='ignore'):
    s = w1[:, :, D].copy()
    for d in range(D):
      prod = w1[:, :, d] * o[:, d:d + 1]
      s = s + prod
    h = np.where(s > np.float32(0.0), s, np.float32(0.0)).astype(np.float32)
    l = w2[:, :, H].copy()
    for j in range(H):
      prod = w2[:, :, j] * h[:, j:j + 1]
      l = l + prod
  return l


def _words(rng, n):
  w = rng.randint(0, 1 << 32, (n, 3), dtype=np.uint64).astype(np.uint32)
  w[0], w[1], w[2], w[3] = 0, 0xFFFFFFFF, (0, 0xFFFFFFFF, 0), (0xFFFFFFFF, 0, 0xFFFFFFFF)        # the ends of the u grid
  return w


def test_the_shim_compiles_the_kernels_header(shim):
  assert shim.shim_stream_sample() == STREAM_SAMPLE
  text = open(os.path.join(CSRC, 'bsx_gumbel.h')).read()
  for fn in ('BSX_HD void bsx_linear_logits(', 'BSX_HD bsx_u32x4 bsx_gumbel_draws(', 'BSX_HD double bsx_gumbel_noise(',
             'BSX_HD double bsx_gumbel_score(', 'BSX_HD int32_t bsx_gumbel_select(', 'BSX_HD void bsx_mlp_logits('):
    assert fn in text, fn
  assert text.count('BSX_NO_CONTRACT') >= 3 and 'BSX_STREAM_SAMPLE' in text and 'bsx_log(' in text
  assert 'fma' not in text.lower().replace('no fma', '') and ' / ' not in re.sub(r'//.*', '', text)       # nothing divides
  assert '#include "../../bsuite_amd/csrc/bsx_gumbel.h"' in open(SHIM).read()
  assert re.search(r'#define BSX_STREAM_SAMPLE 3u\b', open(os.path.join(ROOT, 'include', 'bsx_stream.h')).read())
  dev = open(os.path.join(CSRC, 'bsx_gumbel_device.h')).read()
  assert '#include "bsx_gumbel.h"' in dev
  # the pinned headers and kernels are as they were: nothing of this feature in them
  for f in ('bsx_linear.h', 'bsx_mlp.h', 'bsx_trajectory.h', 'trajectory.hip', 'linear.hip', 'mlp.hip'):
    assert 'gumbel' not in open(os.path.join(CSRC, f)).read().lower(), f


@pytest.mark.parametrize('D', DIMS)
def test_linear_cases_against_the_restatement(shim, D):
  rng = np.random.RandomState(300 + D)
  n = 600
  w = (rng.standard_normal((n, 3, D + 1)) * rng.choice([1e-2, 1.0, 8.0], (n, 1, 1))).astype(np.float32)
  o = (rng.standard_normal((n, D)) * rng.choice([0.1, 1.0, 7.0], (n, 1))).astype(np.float32)
  words, beta = _words(rng, n), rng.choice(BETAS, n)
  logits, action, greedy = _shim_linear(shim, w, o, words, beta)
  want_l = _np_linear_logits(w, o)
  np.testing.assert_array_equal(_bits(logits), _bits(want_l))
  want = _np_select(want_l, words, beta)
  np.testing.assert_array_equal(action, want)
  # argmax of the logits is the existing greedy rule
  np.testing.assert_array_equal(greedy, _np_argmax(want_l.astype(np.float64)))
  assert sorted(set(action.tolist())) == [0, 1, 2] and (action != greedy).mean() > 0.05       # it samples
  # utils.observations: one matrix per lane, and a shared one
  tl = observations.linear_logits(torch.from_numpy(w), torch.from_numpy(o).reshape(n, 1, D))
  assert tl.dtype is torch.float32
  np.testing.assert_array_equal(_bits(tl.numpy()), _bits(want_l))
  np.testing.assert_array_equal(observations.linear_select(torch.from_numpy(w), torch.from_numpy(o)).numpy(), greedy)
  for b in BETAS:
    m = beta == b
    ta = observations.gumbel_select(tl[torch.from_numpy(m)], words[m], temperature=1.0 / b)
    assert ta.dtype is torch.int32
    np.testing.assert_array_equal(ta.numpy(), want[m])
    np.testing.assert_array_equal(observations.gumbel_select(tl[torch.from_numpy(m)], torch.from_numpy(words[m].astype(np.int64)), 1.0 / b).numpy(),
                                  want[m])
  shared = observations.linear_logits(torch.from_numpy(w[7]), torch.from_numpy(o))
  np.testing.assert_array_equal(_bits(shared.numpy()), _bits(_np_linear_logits(np.broadcast_to(w[7], w.shape), o)))


@pytest.mark.parametrize('H', HIDDEN)
@pytest.mark.parametrize('D', DIMS)
def test_hidden_layer_cases_against_the_restatement(shim, D, H):
  rng = np.random.RandomState(100 * D + H)
  n = 400
  w1 = (rng.standard_normal((n, H, D + 1)) * rng.choice([1e-3, 1.0, 50.0], (n, 1, 1))).astype(np.float32)
  w2 = (rng.standard_normal((n, 3, H + 1)) * rng.choice([1e-2, 0.3, 2.0], (n, 1, 1)) / np.sqrt(H)).astype(np.float32)
  o = (rng.standard_normal((n, D)) * rng.choice([0.1, 1.0, 7.0], (n, 1))).astype(np.float32)
  words, beta = _words(rng, n), rng.choice(BETAS, n)
  logits, action, greedy = _shim_mlp(shim, w1, w2, o, words, beta)
  want_l = _np_mlp_logits(w1, w2, o)
  np.testing.assert_array_equal(_bits(logits), _bits(want_l))
  want = _np_select(want_l, words, beta)
  np.testing.assert_array_equal(action, want)
  np.testing.assert_array_equal(greedy, _np_argmax(want_l.astype(np.float64)))                 # bsx_mlp_select
  assert sorted(set(action.tolist())) == [0, 1, 2] and (action != greedy).mean() > 0.05
  tl = observations.mlp_logits(torch.from_numpy(w1), torch.from_numpy(w2), torch.from_numpy(o).reshape(n, 1, D))
  assert tl.dtype is torch.float32
  np.testing.assert_array_equal(_bits(tl.numpy()), _bits(want_l))
  np.testing.assert_array_equal(observations.mlp_select(torch.from_numpy(w1), torch.from_numpy(w2), torch.from_numpy(o)).numpy(), greedy)
  for b in BETAS:
    m = beta == b
    np.testing.assert_array_equal(observations.gumbel_select(tl[torch.from_numpy(m)], words[m], temperature=1.0 / b).numpy(), want[m])
  shared = observations.mlp_logits(torch.from_numpy(w1[7]), torch.from_numpy(w2[7]), torch.from_numpy(o))
  np.testing.assert_array_equal(_bits(shared.numpy()),
                                _bits(_np_mlp_logits(np.broadcast_to(w1[7], w1.shape), np.broadcast_to(w2[7], w2.shape), o)))


def test_scores_of_every_kind_of_word_and_the_noise_is_finite(shim):
  rng = np.random.RandomState(5)
  w = np.concatenate([np.arange(0, 4096, dtype=np.uint64), (1 << 32) - 1 - np.arange(0, 4096, dtype=np.uint64),
                      (1 << 31) + np.arange(-2048, 2048).astype(np.int64).astype(np.uint64),
                      rng.randint(0, 1 << 32, 100000, dtype=np.uint64)]).astype(np.uint32)
  g = np.empty(len(w), np.float64)
  shim.shim_noise(len(w), _ptr(w), _ptr(g))
  np.testing.assert_array_equal(_bits(g), _bits(_np_noise(w)))
  assert np.isfinite(g).all()
  # word 0 is the most negative Gumbel variate, word 2^32 - 1 the most positive: -log(-log(2^-33)), -log(-log(1 - 2^-33))
  assert g[0] == g.min() and abs(g[0] + math.log(33 * math.log(2.0))) < 1e-12
  assert g[4096] == g.max() and abs(g[4096] - 33 * math.log(2.0)) < 1e-6
  # against the oracle's own restatement of the logarithm too
  u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
  assert ((u > 0) & (u < 1)).all()
  np.testing.assert_array_equal(_bits(_np_log(u)), _bits(stream._log(u)))                      # pylint: disable=protected-access
  # the z of three betas, bit for bit
  n = 3000
  logits = (rng.standard_normal((n, 3)) * 3).astype(np.float32)
  words = w[rng.randint(0, len(w), (n, 3))]
  for b in BETAS:
    z, action = _shim_select(shim, logits, words, b)
    want = _np_scores(logits, words, np.full(n, b))
    np.testing.assert_array_equal(_bits(z), _bits(want))
    np.testing.assert_array_equal(action, _np_argmax(want))
    np.testing.assert_array_equal(observations.gumbel_select(torch.from_numpy(logits), words, 1.0 / b).numpy(), action)


def test_ties_nan_and_infinite_logits(shim):
  nan, inf = np.float32('nan'), np.float32('inf')
  same = (0x9E3779B9,) * 3                       # one word for the three actions: equal noise, so equal logits tie
  lo, hi = 0x00000010, 0xFFFFFFF0                # g(lo) = -3.0.., g(hi) = +19.4..
  cases = [  # (logits, words, want)
      ((1, 1, 1), same, 0), ((0, 1, 1), same, 1), ((1, 0, 1), same, 0), ((0, 0, 1), same, 2), ((2, 1, 2), same, 0),
      ((1, 1, 0), same, 0), ((-0.0, 0.0, -0.0), same, 0), ((5, 5, 5), (0, 0, 0), 0), ((5, 5, 5), (0xFFFFFFFF,) * 3, 0),
      # a NaN z_a never wins; a NaN z_0 is never beaten
      ((nan, 1, 2), same, 0), ((nan, inf, inf), (lo, hi, hi), 0), ((0, nan, 2), same, 2), ((0, nan, -2), same, 0), ((0, 1, nan), same, 1),
      ((0, nan, nan), (lo, hi, hi), 0), ((nan, nan, nan), same, 0),
      # infinite logits: the noise is finite, so +inf always wins (the lowest of two), -inf never does unless all are
      ((-inf, -inf, -inf), (lo, hi, hi), 0), ((-inf, 0, inf), (hi, hi, lo), 2), ((inf, inf, 0), (lo, hi, hi), 0), ((0, inf, inf), (hi, lo, hi), 1),
      ((0, -inf, nan), same, 0), ((-inf, -inf, 0), (hi, hi, lo), 2), ((-inf, -1e30, -inf), (hi, lo, hi), 1),
      # the noise decides between equal logits
      ((0, 0, 0), (lo, hi, lo), 1), ((0, 0, 0), (lo, lo, hi), 2), ((0, 0, 0), (hi, lo, lo), 0), ((3, 3, 3), (lo, hi, hi), 1),
  ]
  logits = np.array([c[0] for c in cases], np.float32)
  words = np.array([c[1] for c in cases], np.uint32)
  for b in BETAS:
    z, action = _shim_select(shim, logits, words, b)
    np.testing.assert_array_equal(_bits(z), _bits(_np_scores(logits, words, np.full(len(cases), b))))
    np.testing.assert_array_equal(action, _np_argmax(z))
    for k, c in enumerate(cases):
      assert action[k] == c[2], (b, k, c)
    np.testing.assert_array_equal(observations.gumbel_select(torch.from_numpy(logits), words, 1.0 / b).numpy(), action)
  # the ties are ties: equal z, bit for bit
  z, _ = _shim_select(shim, logits[:2], words[:2], 1.0)
  assert z[0, 0] == z[0, 1] == z[0, 2] and z[1, 1] == z[1, 2] > z[1, 0]


def _round_f64(x):
  """A rational rounded to the nearest float64, ties to even: float(Fraction) is correctly rounded."""
  return float(x)


def _score(l, beta, g, fused):
  """z = l * beta + g in float64: two roundings, or — `fused` — one (exact rationals)."""
  F = fractions.Fraction
  if fused:
    return _round_f64(F(float(l)) * F(float(beta)) + F(float(g)))
  return _round_f64(F(_round_f64(F(float(l)) * F(float(beta)))) + F(float(g)))


def test_fma_contraction_would_flip_the_action(shim):
  """l * beta = 2^60 (1 + 2^-12)(1 + 2^-41) = 2^60 (1 + 2^-12 + 2^-41 + 2^-53) is a tie in float64 and rounds to even,
  P = 2^60 (1 + 2^-12 + 2^-41); its unit in the last place is 2^8, so a Gumbel variate (|g| < 23) added to P is lost.  A fused
  multiply-add keeps the 2^7 of the exact product: with g > 0 the sum lies above the tie and rounds UP to P + 2^8, with g < 0
  below it and rounds down to P.  Action 0 and action 1 have the same logit; action 0 draws g < 0 and action 1 g > 0: in
  separate operations z_0 = z_1 = P, a tie, action 0; fused, z_1 = P + 2^8 > z_0 = P, action 1."""
  l = np.float32(2.0 ** 60) * (np.float32(1.0) + np.float32(2.0 ** -12))
  beta = 1.0 + 2.0 ** -41
  exact = fractions.Fraction(float(l)) * fractions.Fraction(beta)
  P = 2.0 ** 60 * (1.0 + 2.0 ** -12 + 2.0 ** -41)
  assert exact == fractions.Fraction(P) + 2 ** 7 and float(exact) == P and np.spacing(P) == 2.0 ** 8
  words = np.array([[0x10000000, 0xC0000000, 0x10000000]], np.uint32)
  g = _np_noise(words)[0]
  assert g[0] < 0 < g[1] and g[2] == g[0]
  logits = np.array([[l, l, -np.float32('inf')]], np.float32)
  plain = [_score(l, beta, g[a], False) for a in (0, 1)]
  fused = [_score(l, beta, g[a], True) for a in (0, 1)]
  assert plain == [P, P] and fused == [P, P + 2.0 ** 8]
  z, action = _shim_select(shim, logits, words, beta)
  assert z[0, 0] == z[0, 1] == P and action.tolist() == [0]                                    # the header: two roundings
  np.testing.assert_array_equal(_bits(z), _bits(_np_scores(logits, words, np.array([beta]))))
  assert observations.gumbel_select(torch.from_numpy(logits), words, 1.0 / beta).tolist() == [0]
  assert 1.0 / (1.0 / beta) == beta                                                            # (the temperature round trip is exact here)
  # the same through the whole linear rule: the logit from a bias alone
  for D in DIMS:
    w = np.zeros((1, 3, D + 1), np.float32)
    w[0, :, D] = logits[0]
    got_l, a, _ = _shim_linear(shim, w, np.zeros((1, D), np.float32), words, np.array([beta]))
    np.testing.assert_array_equal(_bits(got_l), _bits(logits))
    assert a.tolist() == [0]


def test_bsx_log_is_within_4_ulp_of_libm_on_the_arguments_of_the_rule(shim):
  """The rule takes bsx_log of u in [2^-33, 1 - 2^-33] and of e = -log(u) in [1.16e-10, 22.9]: measured through the shim
  against math.log — 3 ulp on [1e-10, 23] (random arguments, log-uniform, and a dense band around 1), 2 ulp on the u grid (both
  ends, the middle and random words).  The bound is 4 ulp."""
  rng = np.random.RandomState(0)
  x = np.exp(rng.uniform(math.log(1e-10), math.log(23.0), 200000))
  x = np.concatenate([x, [1e-10, 23.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 0.5, 2.0, 1.4142135623730951,
                          np.nextafter(1.4142135623730951, 2.0), 0.7071067811865476], 1.0 + rng.uniform(-1e-3, 1e-3, 50000)])
  x = x[x != 1.0]
  w = np.concatenate([rng.randint(0, 1 << 32, 200000, dtype=np.uint64), np.arange(0, 30000, dtype=np.uint64),
                      (1 << 32) - 1 - np.arange(0, 30000, dtype=np.uint64),
                      (1 << 31) + np.arange(-3000, 3000).astype(np.int64).astype(np.uint64)])
  u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
  e = -_shim_log(shim, u)
  assert 1.16e-10 < e.min() and e.max() < 22.9
  worst = {}
  for name, arg in (('range', x), ('u grid', u), ('inner', e[e != 1.0])):
    got = _shim_log(shim, arg)
    ref = np.array([math.log(v) for v in arg])
    worst[name] = float(np.max(np.abs(got - ref) / np.spacing(np.abs(ref))))
    np.testing.assert_array_equal(_bits(got), _bits(_np_log(arg)))                             # and the restatement, bit for bit
  print('bsx_log against math.log, worst error in ulp:', worst)
  assert all(v <= 4.0 for v in worst.values()), worst
  assert _shim_log(shim, np.array([1.0]))[0] == 0.0


# ------------------------------------------------------------------------------------------ the distribution
@pytest.mark.parametrize('step', [0, (1 << 34) + 3])
@pytest.mark.parametrize('beta', [0.5, 1.0, 2.0])
@pytest.mark.parametrize('seed', [0, 1, 2, (1 << 63) + 5])
def test_action_frequencies_follow_the_softmax(shim, seed, beta, step):
  """Logits (0, ln 2, ln 4) in float32, 65536 lanes from lane 2^32 - 17 on, one step: every action's frequency within 4 sigma
  of softmax(beta * logits), sigma = sqrt(p (1 - p) / N).  The words are the header's (bsx_gumbel_draws), held against
  oracle/stream.py's stream 3."""
  N, lane0 = 65536, (1 << 32) - 17
  words = np.zeros((N, 4), np.uint32)
  shim.shim_draws(seed, lane0, N, step, _ptr(words))
  ref = stream.words(seed, np.uint64(lane0) + np.arange(N, dtype=np.uint64), step, STREAM_SAMPLE, 4)
  np.testing.assert_array_equal(words, ref)
  l = np.array([0.0, np.log(2.0), np.log(4.0)]).astype(np.float32)
  logits = np.ascontiguousarray(np.broadcast_to(l, (N, 3)))
  _, action = _shim_select(shim, logits, np.ascontiguousarray(words[:, :3]), beta)
  np.testing.assert_array_equal(action, _np_select(logits, words[:, :3], np.full(N, beta)))
  p = np.exp(beta * l.astype(np.float64))
  p = p / p.sum()
  freq = np.bincount(action, minlength=3) / N
  sigma = np.sqrt(p * (1 - p) / N)
  print('seed', seed, 'beta', beta, 'step', step, 'frequencies', freq, 'in sigma', (freq - p) / sigma)
  assert (np.abs(freq - p) <= 4 * sigma).all(), (freq, p, (freq - p) / sigma)


def test_the_sample_stream_shares_no_word_with_the_exploration_stream():
  lanes = np.uint64((1 << 32) - 17) + np.arange(64, dtype=np.uint64)
  a, b = stream.words(9, lanes, 5, STREAM_SAMPLE, 4), stream.words(9, lanes, 5, 2, 4)
  assert not (a == b).any()


# ------------------------------------------------------------------------------------------ the Python entry points
def _envs():
  return [cartpole.Cartpole(seed=0, batch=4), cartpole.CartpoleSwingup(seed=0, batch=4), mountain_car.MountainCar(seed=0, batch=4)]


def _dim(env):
  return int(np.prod(env.observation_spec().shape))


def _refused(env, kind, exc=ValueError, match=None, **kw):
  """env.sample_<kind>(...) raises, its message names the caller, and nothing was allocated."""
  raw = env.raw_env if hasattr(env, 'raw_env') else env
  name = f'sample_{kind}'
  obs = kw.pop('observation') if 'observation' in kw else torch.zeros((4, 3), dtype=torch.float32)
  if kind == 'linear':
    pol = (kw.pop('weights') if 'weights' in kw else torch.zeros((3, 4), dtype=torch.float32),)      # (None is one of the bad values)
  else:
    pol = (kw.pop('w1') if 'w1' in kw else torch.zeros((5, 4), dtype=torch.float32),
           kw.pop('w2') if 'w2' in kw else torch.zeros((3, 6), dtype=torch.float32))
  with pytest.raises(exc, match=match or name) as info:
    getattr(env, name)(*pol, obs, kw.pop('num_steps', 4), **kw)
  assert name in str(info.value)
  assert not raw._allocated and not raw._policy_rollout_out                # pylint: disable=protected-access


def test_signatures_docstrings_and_families():
  want = dict(linear=['self', 'weights', 'observation', 'num_steps', 'policy_index', 'temperature', 'sample_seed'],
              mlp=['self', 'w1', 'w2', 'observation', 'num_steps', 'policy_index', 'temperature', 'sample_seed'])
  for kind in KINDS:
    fn = getattr(base.Environment, f'sample_{kind}')
    p = inspect.signature(fn).parameters
    assert list(p) == want[kind]
    assert [p[k].kind for k in ('policy_index', 'temperature', 'sample_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
    assert p['policy_index'].default is None and p['temperature'].default == 1.0 and p['sample_seed'].default == 0
    assert 'epsilon' not in p and 'explore_seed' not in p
    rollout = inspect.signature(getattr(base.Environment, f'rollout_{kind}')).parameters
    assert list(p)[:-2] == list(rollout)[:-2]                              # rollout_*'s, but for the two exploration arguments
    for word in ('actions', 'ts[t] = step(a); actions[t] = a', f'rollout_{kind}', f'{kind}_logits', 'gumbel_select', 'rollout(actions)',
                 'policy_index', 'cached per T', 'temperature', 'sample_seed', 'stream 3' if kind == 'linear' else 'sample_linear'):
      assert word in fn.__doc__, (kind, word)
    abi = lambda cls: cls._closed_loop_abi(object.__new__(cls), f'sample_{kind}')       # pylint: disable=protected-access,cell-var-from-loop
    assert abi(cartpole.Cartpole) == abi(cartpole.CartpoleSwingup) == ENTRY['cartpole', kind]
    assert abi(mountain_car.MountainCar) == ENTRY['mountain_car', kind] and ENTRY['cartpole', kind] in _native.EXPORTED
    assert abi(base.Environment) is None and abi(catch.Catch) is None and ENTRY['mountain_car', kind] in _native.EXPORTED
    # the refusals are the recording call's, then the two of its own, then the slab — two faults at a time, the earlier one's
    # message — all before the allocation
    for env in _envs():
      D, first = _dim(env), 'weights' if kind == 'linear' else 'w1'
      shapes = dict(weights=(3, D + 1)) if kind == 'linear' else dict(w1=(5, D + 1), w2=(3, 6))
      env._device = torch.device('cpu')
      good = dict({k: torch.zeros(v) for k, v in shapes.items()}, observation=torch.zeros((4, D)))
      _refused(env, kind, match=f'{first} must be', temperature=0.0, **dict(good, **{first: None}))
      _refused(env, kind, match='temperature must be', temperature=0.0, sample_seed=-1, **good)
      env._device = torch.device('meta')                                   # tensors without storage: a slab of 4 GiB passes the
      env._batch = -(-(1 << 32) // (4 * D))                                # arguments' checks
      big = dict({k: torch.zeros(v, device='meta') for k, v in shapes.items()}, observation=torch.zeros((env._batch, D), device='meta'))
      _refused(env, kind, match='sample_seed must be', sample_seed=-1, **big)
      _refused(env, kind, match='4 GiB', **big)
  for name in ('linear_logits', 'mlp_logits', 'gumbel_select'):
    src = inspect.getsource(getattr(observations, name))
    code = re.sub(r'""".*?"""', '', src, flags=re.S)
    for word in ('addcmul', 'matmul', 'torch.log', '@', 'einsum'):
      assert word not in code, (name, word)
  assert 'torch.log' not in re.sub(r'""".*?"""', '', inspect.getsource(observations._stream_log), flags=re.S)     # pylint: disable=protected-access


def test_views_families_and_modes_are_refused():
  for kind in KINDS:
    for env in (cartpole.Cartpole(seed=0), cartpole.CartpoleSwingup(seed=0), mountain_car.MountainCar(seed=0)):
      _refused(env, kind, match='batched view')
    for bsuite_id in ('bandit/0', 'deep_sea/0', 'catch/0', 'memory_len/0', 'umbrella_length/0', 'discounting_chain/0'):
      _refused(bsuite_amd.load_from_id(bsuite_id, batch=4), kind, match='mountain_car only')
    _refused(catch.Catch(seed=0, batch=4, observation_mode='index'), kind, match='mountain_car only')
    for cls in (cartpole.Cartpole, cartpole.CartpoleSwingup, mountain_car.MountainCar):
      _refused(cls(seed=0, batch=4, rng='mt19937'), kind, match='philox')
    for env in _envs():
      env._logging = dict(steps=None)           # what enable_logging() leaves behind (it allocates: not without a GPU)
      _refused(env, kind, match='Logging')
    for env in _envs():
      env._grouped_by = object()                # what SweepBatch sets while its prepared groups hold the column pointers
      _refused(env, kind, exc=RuntimeError, match='release_groups')
    # a step of 4 GiB or more: the kernel's 32-bit lane offsets could not span it
    for env in _envs():
      env._batch = -(-(1 << 32) // (4 * _dim(env)))
      with pytest.raises(ValueError, match=f'sample_{kind}: .* 4 GiB'):
        env._check_trajectory_slab(f'sample_{kind}')                       # pylint: disable=protected-access
      assert not env._allocated                                            # pylint: disable=protected-access


def test_the_wrappers_refuse_instead_of_delegating():
  for kind in KINDS:
    name = f'sample_{kind}'
    for make in (lambda e: wrappers.RewardNoise(e, noise_scale=0.5, seed=1), lambda e: wrappers.RewardScale(e, reward_scale=2.0)):
      for raw in _envs():
        _refused(make(raw), kind, match='not available through')
        _refused(raw, kind, match='reward wrapper')                       # ... and the raw environment knows it is wrapped
    for bsuite_id in ('cartpole_noise/2', 'cartpole_scale/4', 'mountain_car_noise/3', 'mountain_car_scale/1'):
      env = bsuite_amd.load_from_id(bsuite_id, batch=4)
      assert hasattr(env, 'raw_env'), bsuite_id
      _refused(env, kind, match='not available through')
    # every wrapper class carries its own method (attribute delegation would reach the raw environment's)
    for cls in (wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
      fn = getattr(cls, name)
      assert fn is not getattr(base.Environment, name) and any(name in vars(c) for c in cls.__mro__[:-1]), cls
      args = (torch.zeros((3, 4)),) if kind == 'linear' else (torch.zeros((5, 4)), torch.zeros((3, 6)))
      with pytest.raises(ValueError, match=name):
        fn(object.__new__(cls), *args, torch.zeros((4, 3)), 4, temperature=2.0, sample_seed=1)
    image = wrappers.ImageObservation(mountain_car.MountainCar(seed=0, batch=4), (84, 84, 1))
    _refused(image, kind, match='not available through ImageObservation')


def test_arguments_are_checked_before_any_gpu_use():
  for env in _envs():
    env._device = torch.device('cpu')       # the checks themselves, on host tensors: dtype, shape, contiguity
    D, H = _dim(env), 5
    w, pw = torch.zeros((3, D + 1)), torch.zeros((4, 3, D + 1))
    w1, w2, p1, p2 = torch.zeros((H, D + 1)), torch.zeros((3, H + 1)), torch.zeros((4, H, D + 1)), torch.zeros((4, 3, H + 1))
    obs = torch.zeros((4, 1, D), dtype=torch.float32)
    idx = torch.zeros(4, dtype=torch.int32)
    for kind, ok, pop in (('linear', dict(weights=w), dict(weights=pw)), ('mlp', dict(w1=w1, w2=w2), dict(w1=p1, w2=p2))):
      name = f'sample_{kind}'
      for t in (0.0, -1.0, -0.0, float('nan'), float('inf'), float('-inf'), 5e-324, 1e-310, '1.0', None, True, [1.0]):
        _refused(env, kind, temperature=t, observation=obs, match=f'{name}: temperature', **ok)
      for n in (0, -1, 2.0, None, '4', True):
        _refused(env, kind, num_steps=n, observation=obs, match=f'{name}: num_steps', **ok)
      for seed in (-1, 1 << 64, 0.5, None, True, '3'):
        _refused(env, kind, sample_seed=seed, observation=obs, match=f'{name}: sample_seed', **ok)
      for word in ('epsilon', 'explore_seed'):                             # there is no epsilon: the softmax explores
        with pytest.raises(TypeError, match=word):
          getattr(env, name)(*ok.values(), obs, 4, **{word: 0})
      for bad in (obs.to(torch.float64), obs.numpy(), torch.zeros((4, D + 1)), torch.zeros((3, 1, D)), torch.zeros(4 * D),
                  torch.zeros((4, 2 * D))[:, ::2], None):
        _refused(env, kind, observation=bad, match=f'{name}: observation must be', **ok)
      _refused(env, kind, observation=torch.zeros((4, D)), policy_index=idx, match='must be None', **ok)
      for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)[::2]):
        _refused(env, kind, observation=obs, policy_index=bad, match='policy_index', **pop)
    for bad in (w.to(torch.float64), w.numpy(), torch.zeros((3, D)), torch.zeros((2, D + 1)), torch.zeros((0, 3, D + 1)),
                torch.zeros((3, 2 * (D + 1)))[:, ::2], None):
      _refused(env, 'linear', weights=bad, observation=obs, match='sample_linear: weights must be')
    for bad in (w1.to(torch.float64), torch.zeros((H, D)), torch.zeros((0, D + 1)), torch.zeros((65, D + 1)), None):
      _refused(env, 'mlp', w1=bad, w2=w2, observation=obs, match='sample_mlp: w1 must be')
    for bad in (w2.to(torch.float64), torch.zeros((3, H)), torch.zeros((2, H + 1)), torch.zeros((1, 3, H + 1)), None):
      _refused(env, 'mlp', w1=w1, w2=bad, observation=obs, match='sample_mlp: w2 must be')
    assert not env._allocated                                                       # pylint: disable=protected-access
  # beta is computed in float64 on the host: the smallest and the largest temperature that have a finite inverse
  check = base.Environment._check_sample                                             # pylint: disable=protected-access
  assert check('x', 4.0, 0) == 0.25 and check('x', np.float32(0.5), (1 << 64) - 1) == 2.0 and check('x', 2, np.int64(5)) == 0.5
  assert check('x', 1e308, 0) == 1e-308 and math.isfinite(check('x', 1e-308, 0))
  # host tensors for an environment on the GPU
  env = mountain_car.MountainCar(seed=0, batch=4)
  _refused(env, 'linear', weights=torch.zeros((3, 4)), observation=torch.zeros((4, 1, 3)), match='weights must be')
  _refused(env, 'mlp', observation=torch.zeros((4, 1, 3)), match='w1 must be')


# ------------------------------------------------------------------------------------------ the C ABI
def test_header_binding_and_export_agree_and_the_abi_stays_v12():
  header = open(HEADER).read()
  assert re.search(r'#define BSX_ABI_VERSION 12\b', header)
  assert _native.ABI_VERSION == 12 and _native.lib.bsx_abi_version() == 12
  plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  out = subprocess.check_output(['nm', '-D', '--defined-only', _native.SO_PATH], text=True)
  P = ctypes.c_void_p
  text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  for (fam, kind), name in ENTRY.items():
    decl = re.search(r'int ' + name + r'\(([^;]*)\);', plain)
    assert decl, f'include/bsuite_amd.h does not declare {name}'
    types = [re.sub(r'\s*\w+$', '', a.strip()) for a in ' '.join(decl.group(1).split()).split(',')]
    assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', f'const bsx_{kind}_t*', 'double', 'float*', 'int32_t*', 'bsx_timestep_t',
                     'int32_t*', 'double*']
    # the matching *_rollout with one double after the policy struct
    roll = re.search(r'int ' + name.replace('_sample', '_rollout') + r'\(([^;]*)\);', plain)
    rtypes = [re.sub(r'\s*\w+$', '', a.strip()) for a in ' '.join(roll.group(1).split()).split(',')]
    assert types[:3] + types[4:] == rtypes
    assert name in _native.EXPORTED
    fn = getattr(_native.lib, name)
    cfg = dict(cartpole=_native.CartpoleCfg, mountain_car=_native.MountainCarCfg)[fam]
    policy = dict(linear=_native.Linear, mlp=_native.Mlp)[kind]
    assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(policy), ctypes.c_double, P, P,
                           _native.TimeStepPtrs, P, P]
    assert fn.restype is ctypes.c_int
    assert any(l.split()[-1] == name and ' T ' in l for l in out.splitlines())
    assert name in text, f'INTEGRATION.md does not describe {name}'
    assert 'extern "C" int ' + name + '(' in open(os.path.join(CSRC, fam + '.hip')).read()
  # no new struct and no new field: the policies and the TimeStep are the existing ones
  assert ctypes.sizeof(_native.Linear) == 48 and ctypes.sizeof(_native.Mlp) == 56 and ctypes.sizeof(_native.TimeStepPtrs) == 32
  assert [f[0] for f in _native.Linear._fields_] == ['weights', 'n_policies', 'policy_index', 'epsilon', 'explore_seed', 'observation_in']     # pylint: disable=protected-access
  note = header[header.index('fused sampled trajectories'):header.index('int bsx_cartpole_linear_sample(')]
  for word in ('BSX_STREAM_SAMPLE', 'SAMPLE SEED', 'BSX_ERANGE', 'inv_temperature', 'epsilon is not 0.0'):
    assert word in note, word


def _abi_case(fam):
  if fam == 'mountain_car':
    return _native.MountainCarCfg(1000, 0), _native.MountainCarCfg(0, 0)
  good = dict(swingup=0, last_step=1001, height_threshold=0.8, x_threshold=3.0, theta_dot_threshold=1.0, x_reward_threshold=1.0,
              timescale=0.01, mass_cart=1.0, mass_pole=0.1, length=0.5, force_mag=10.0, gravity=9.8, move_cost=0.0, init_range=0.05,
              theta_offset=0.0, time_frac=0xDEAD0008)
  return _native.CartpoleCfg(**good), _native.CartpoleCfg(**dict(good, last_step=0))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fam', ['cartpole', 'mountain_car'])
def test_argument_checks_of_the_entry_points(fam, kind):
  """Every refusal comes before any device work: garbage stands in for device pointers, none is dereferenced.  The codes and
  their order are those of bsx_<family>_<kind>_rollout; a non-zero epsilon and a bad inv_temperature are BSX_ERANGE where an
  epsilon outside [0, 1] is there: after the modes and the scalars, before an empty call returns, before the pointers."""
  fn = getattr(_native.lib, ENTRY[fam, kind])
  cfg, bad_cfg = _abi_case(fam)
  junk = 0xDEAD0010                                                # never mapped: a dereference would fault (16-byte aligned)
  E = _native
  D = 3 if fam == 'mountain_car' else 6
  nan, inf = float('nan'), float('inf')

  def call(**kw):
    c = _native.Call(n_lanes=kw.pop('n_lanes', 4), n_steps=kw.pop('n_steps', 4), flags=kw.pop('flags', 0))
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def policy(**kw):
    if kind == 'linear':
      kw.pop('hidden', None)
      d = dict(weights=junk, n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0, observation_in=junk)
      d.update(kw)
      return _native.Linear(**d)
    d = dict(w1=junk, w2=junk, hidden=5, n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0, observation_in=junk)
    d.update(kw)
    return _native.Mlp(**d)

  def run(c, q, beta=1.0, state=junk, steps=junk, out=None, actions=junk, info=junk, cfg_=cfg):
    out = _native.TimeStepPtrs(junk, junk, junk, junk) if out is None else out
    return fn(ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(c) if c is not None else None,
              ctypes.byref(q) if q is not None else None, beta, state, steps, out, actions, info)

  bad_betas = (0.0, -0.0, -1.0, nan, inf, -inf)
  # null structs
  assert run(call(), policy(), cfg_=None) == E.BSX_ENULL
  assert run(None, policy()) == E.BSX_ENULL
  assert run(call(), None) == E.BSX_ENULL
  # BSX_EMODE: before the scalars — and before a bad temperature
  for flags in (E.CALL_OBS_INDEX, E.CALL_OBS_U8, E.CALL_OBS_F16, E.CALL_OBS_BF16, E.CALL_OBS_INDEX | E.CALL_OBS_U8):
    assert run(call(flags=flags), policy(n_policies=-1, hidden=0)) == E.BSX_EMODE, flags
    assert run(call(flags=flags), policy(), beta=nan) == E.BSX_EMODE, flags
  lg = _native.Logging()
  assert run(call(logging=ctypes.pointer(lg)), policy(hidden=99)) == E.BSX_EMODE
  for wrap in (E.WRAP_SCALE, E.WRAP_NOISE, E.WRAP_SCALE_NOISE, E.WRAP_NOISE_SCALE):
    c = call()
    c.wrap.kind = wrap
    assert run(c, policy()) == E.BSX_EMODE, wrap
  c = call()
  c.stream.mt_state, c.stream.mt_pos = junk, junk
  assert run(c, policy()) == E.BSX_EMODE
  for member in ('reward_f64', 'obs_paint', 'state_alt'):
    assert run(call(**{member: junk}), policy()) == E.BSX_EMODE, member
  assert run(call(force_reset=1), policy(), beta=0.0) == E.BSX_EMODE
  assert run(call(action_ring=4), policy(epsilon=0.5)) == E.BSX_EMODE
  # BSX_EINVAL: the scalars, before the temperature
  for n in (0, -1):
    assert run(call(n_steps=n), policy()) == E.BSX_EINVAL
    assert run(call(n_steps=n), policy(), beta=-1.0) == E.BSX_EINVAL
  assert run(call(n_lanes=-1), policy(), beta=inf) == E.BSX_EINVAL
  if kind == 'mlp':
    for h in (0, -1, 65, 1 << 20):
      assert run(call(), policy(hidden=h)) == E.BSX_EINVAL, h
      assert run(call(), policy(hidden=h), beta=nan) == E.BSX_EINVAL, h               # where n_policies < 1 is: before the temperature
      assert run(call(n_lanes=0), policy(hidden=h)) == E.BSX_EINVAL, h
    for h in (1, 64):
      assert run(call(n_lanes=0), policy(hidden=h)) == 0
  for n in (0, -3):
    assert run(call(), policy(n_policies=n)) == E.BSX_EINVAL
    assert run(call(), policy(n_policies=n, epsilon=0.5), beta=0.0) == E.BSX_EINVAL
  # BSX_ERANGE: epsilon must be 0.0 — also one that an epsilon-greedy call accepts — and inv_temperature finite and > 0
  for eps in (0.3, 1.0, 5e-324, -1e-9, 1.0000001, nan, inf):
    assert run(call(), policy(epsilon=eps)) == E.BSX_ERANGE, eps
  assert run(call(n_lanes=0), policy(epsilon=-0.0)) == 0                                    # (-0.0 == 0.0)
  for b in bad_betas:
    assert run(call(), policy(), beta=b) == E.BSX_ERANGE, b
    assert run(call(n_lanes=0), policy(), beta=b) == E.BSX_ERANGE, b                        # an empty call still checks its scalars
    none_ = {k: None for k in (('weights',) if kind == 'linear' else ('w1', 'w2')) + ('observation_in',)}
    assert run(call(), policy(**none_), beta=b, state=None) == E.BSX_ERANGE, b              # ... before any pointer is looked at
  assert run(call(), policy(), cfg_=bad_cfg) == E.BSX_ERANGE
  assert run(call(flags=E.CALL_OBS_INDEX), policy(), cfg_=bad_cfg) == E.BSX_ERANGE          # (the cfg comes first)
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at; the extreme temperatures are accepted
  none = {k: None for k in (('weights',) if kind == 'linear' else ('w1', 'w2')) + ('observation_in',)}
  for b in (1.0, 5e-324, 1.7976931348623157e308):
    assert run(call(n_lanes=0), policy(**none), beta=b, state=None, steps=None, out=_native.TimeStepPtrs(0, 0, 0, 0), actions=None,
               info=None) == 0, b
  assert run(call(n_lanes=0), policy(epsilon=0.3)) == E.BSX_ERANGE
  # BSX_ENULL: every pointer — the other ones garbage
  for missing in none:
    assert run(call(), policy(**{missing: None})) == E.BSX_ENULL, missing
  for missing in ('state', 'steps', 'info'):
    assert run(call(), policy(), **{missing: None}) == E.BSX_ENULL, missing
  for k in range(4):                                                                        # every pointer of the TimeStep
    ptrs = [junk] * 4
    ptrs[k] = 0
    assert run(call(), policy(), out=_native.TimeStepPtrs(*ptrs)) == E.BSX_ENULL, k
  assert run(call(), policy(), actions=None) == E.BSX_ENULL                                 # ... and the action column
  assert run(call(), policy(n_policies=2)) == E.BSX_ENULL                                   # a population without policy_index
  if fam == 'cartpole':
    no_table = _abi_case(fam)[0]
    no_table.time_frac = None
    assert run(call(), policy(), cfg_=no_table) == E.BSX_ENULL
  assert run(call(n_lanes=1 << 40), policy()) == E.BSX_EINVAL                               # more workgroups than a grid holds
  assert run(call(action_ring=-2), policy()) == E.BSX_EINVAL
  # what only a call that writes [T,B] slabs refuses: a slab the 32-bit lane offsets cannot span
  assert run(call(n_lanes=-(-(1 << 32) // (4 * D))), policy()) == E.BSX_EINVAL
  assert run(call(n_lanes=1 << 31), policy()) == E.BSX_EINVAL


# ------------------------------------------------------------------------------------------ the source text
def test_the_kernel_body_uses_the_headers():
  dev = open(os.path.join(CSRC, 'bsx_gumbel_device.h')).read()
  body = dev[dev.index('void bsx_gumbel_body('):]
  body = body[:body.index('\n}\n')]
  walk = dev[dev.index('void bsx_gumbel_hidden_logits('):]
  walk = walk[:walk.index('\n}\n')]
  for call_ in ('bsx_linear_logits(w, o, D, l)', 'bsx_gumbel_hidden_logits<D>(', 'bsx_gumbel_draws(p.explore_seed, lane, step)',
                'bsx_gumbel_select(l, gt.beta, u.v[0], u.v[1], u.v[2])', 'bsx_policy_clamp(k0.p.policy_index[i], k0.p.n_policies)',
                'Env::reset_pending(rg)', 'bsx_pool_counts(', 'Env::template core<0, 0, true, false, false, V, true>(',
                'Env::template load_info<V>(', 'Env::template store_info<V>(', 'bsx_fresh(0u)', 'bsx_gumbel_view(ka)',
                'bsx_emit_values<0, 0, false, 0>(', 'small_obs_store_row<true>(bsx_at_off(kt.out.observation',
                'small_rollout_nt_scalars<Env>::value', 'bsx_st<BSX_OUT_SCALARS.rollout>(bsx_at_off(kt.actions_out'):
    assert call_ in body, call_
  for piece in ('bsx_mlp_hidden(', 'bsx_mlp_accumulate('):              # the hidden-layer logits in the kernel's pieces
    assert piece in walk, piece
  loop = body[body.index('for (int t = 0; t < n_steps; ++t) {'):]
  loop = loop[:loop.index('\n    }\n')]
  assert 'core<' in loop and 'bsx_gumbel_select(' in loop and loop.count('bsx_gumbel_hidden_logits<D>(') == 2
  assert loop.count('bsx_st<') == 4 and loop.count('small_obs_store_row<true>(') == 1
  assert 'if (!resets) {' in loop and loop.index('if (!resets) {') < loop.index('bsx_gumbel_draws(')       # nothing drawn on a reset
  for word in ('__syncthreads', 'atomic', 's_w[', 'Env::store', 'store_info', 'observation_in', 'bsx_pool_counts', 'epsilon'):
    assert word not in loop, word
  for word in ('__syncthreads', 'atomic', 'bsx_st<', 's_w['):
    assert word not in walk, word
  # three views: before the loop, per step, after the loop (+ the pooled counts)
  assert body.count('bsx_gumbel_view(ka)') == 4 and loop.count('bsx_gumbel_view(ka)') == 1
  # no second statement of either rule: no comparison of logits or scores, no logarithm, no ReLU outside the headers
  for f in ('bsx_gumbel_device.h', 'gumbel.hip'):
    text = re.sub(r'//.*', '', open(os.path.join(CSRC, f)).read())
    for word in ('l_best', 'z_best', '> 0.0f', 'bsx_log(', '0x1p-32', 'bsx_mlp_argmax', 'bsx_linear_select'):
      assert word not in text, (f, word)
  hip = open(os.path.join(CSRC, 'gumbel.hip')).read()
  assert hip.count('__global__') == 1
  assert '__global__ void __launch_bounds__(BSX_BLOCK) bsx_gumbel_kernel(const bsx_gumbel_args a)' in hip
  for inst in ('<Fam, V, true, true>', '<Fam, V, false, true>', '<Fam, V, true, false>', '<Fam, V, false, false>'):
    assert 'bsx_gumbel_body' + inst in hip, inst
  for inst in ('<bsx_trajectory_mountain_car, 0>', '<bsx_trajectory_cartpole, 1>', '<bsx_trajectory_cartpole, 0>'):
    assert 'bsx_gumbel_switch' + inst in hip, inst
  assert re.search(r'struct bsx_gumbel_args \{\s*bsx_trajectory_args t;\s*double beta;', dev)
  # what paid for the kernel: one tagged kernel for the two launches of an mnist group, the bodies those of the stand-alone kernels
  mnist = open(os.path.join(CSRC, 'mnist.hip')).read()
  assert '__global__ void __launch_bounds__(BSX_BLOCK) mnist_group_kernel(const mnist_group_args a)' in mnist
  assert 'mnist_advance_group_kernel' not in mnist and 'mnist_observe_group_kernel' not in mnist
  assert mnist.count('__global__') == 3 and 'a.phase == MNIST_GROUP_ADVANCE' in mnist
  assert 'mnist_advance_body(a.table.advance[w.seg], w.block, s_cnt)' in mnist and 'mnist_observe_body<K>(a.table.observe[w.seg], w.block, s_lut)' in mnist


def test_the_shim_runs_stand_alone_under_the_sanitizers(tmp_path):
  """bsx_gumbel.h with its own main under AddressSanitizer and UBSan, on the CPU (nothing loaded into python)."""
  exe = str(tmp_path / 'gumbel_shim_main')
  cmd = ['gcc', '-O1', '-g', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-DGUMBEL_SHIM_MAIN', SHIM, '-o', exe]
  if subprocess.run(cmd, capture_output=True).returncode != 0:
    pytest.skip('this gcc has no sanitizer runtime')
  out = subprocess.run([exe], capture_output=True, text=True)
  assert out.returncode == 0, out
  seen = [int(x) for x in out.stdout.split()]
  assert len(seen) == 3 and sum(seen) == 64, out


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
NEW = 'bsx_gumbel_kernel'


@needs_llvm
def test_product_library_has_the_one_new_kernel_inside_the_kernel_budget():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  assert [n for n in ks if 'gumbel' in n] == [NEW]                       # ONE kernel for the twelve cases
  assert not any(w in NEW for w in ('trajectory', 'eval', 'linear', 'mlp', 'policy', 'score', 'index', 'hot_cells', 'calib_'))
  # what paid for it: the two launches of an mnist group are one kernel; the stand-alone pair is as it was
  assert 'mnist_group_kernel<4>' in ks and 'mnist_advance_group_kernel' not in ks and 'mnist_observe_group_kernel<4>' not in ks
  assert sorted(n for n in ks if n.startswith('mnist_')) == ['mnist_advance_kernel', 'mnist_group_kernel<4>', 'mnist_observe_kernel<4>']
  g = ks['mnist_group_kernel<4>']
  assert g['private_segment_fixed_size'] == 0 and g['vgpr_spill_count'] == 0 and g['sgpr_spill_count'] == 0 and g['vgpr_count'] <= 64, g
  k = ks[NEW]
  assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
  assert k['agpr_count'] == 0, k
  assert k['vgpr_count'] <= 128, k
  assert k['group_segment_fixed_size'] <= 4096, k
  # the neighbours it was modelled on are untouched
  assert 'bsx_trajectory_kernel' in ks and 'bsx_linear_score_kernel' in ks and 'bsx_mlp_returns_kernel' in ks


@needs_llvm
def test_stores_inside_the_loops_of_the_new_kernel_and_nothing_that_waits():
  """Inside ANY loop of the kernel (the compiler marks a loop's blocks in its block comments): the per-step stores are there,
  every one addressed as {scalar base} + {32-bit lane offset}; no flat, scratch or buffer access, no barrier, no LDS write, no
  atomic, no spill reload.  The rows follow small_obs_store_row<true>: three floats as one non-temporal 12-byte store, six and
  eight in plain 16- and 8-byte pieces.  The action column is non-temporal, and so are cartpole's scalar columns; mountain_car's
  are plain (small_rollout_nt_scalars<mountain_car_env>)."""
  _, text = ki.kernel_text(os.path.join(CSRC, 'gumbel.hip'), NEW)
  in_loop, inside, headers = False, [], 0
  for l in text:
    if re.match(r'^\.LBB\d+_\d+:', l) or l.startswith('; %bb.'):
      in_loop = 'Loop' in l
      headers += 'Loop Header' in l and 'Depth=1' in l
      continue
    s = l.strip()
    if in_loop and s and not s.startswith(';') and not s.startswith('.'):
      inside.append(s)
  assert headers >= 12, headers
  stores = [s for s in inside if s.startswith('global_store')]
  assert len(stores) >= 12 * 5, len(stores)
  form = r', s\[\d+:\d+\]( offset:\d+)?( nt)?$'
  assert all(re.search(form, s) for s in stores), [s for s in stores if not re.search(form, s)]
  rows = [s for s in stores if re.match(r'global_store_dwordx[234] ', s)]
  assert len(rows) >= 12, rows
  assert sum(s.startswith('global_store_dwordx3 ') and s.endswith(' nt') for s in rows) == 4          # mountain_car's rows
  assert all(not s.endswith(' nt') for s in rows if not s.startswith('global_store_dwordx3 '))        # cartpole's: partial lines
  # 12 branches x the action column, + 8 cartpole branches x (reward, discount): dword stores, non-temporal
  assert sum(s.startswith('global_store_dword ') and s.endswith(' nt') for s in stores) == 12 + 16
  scalars = [s.split()[0] for s in stores if not s.endswith(' nt') and not re.match(r'global_store_dwordx[234] ', s)]
  assert sorted(scalars) == ['global_store_byte'] * 4 + ['global_store_dword'] * 8, scalars          # mountain_car's scalar columns
  assert sum(s.startswith('ds_read') for s in inside) >= 6, 'the shared policy is read inside the loops'
  assert any('f64' in s for s in inside), 'the Gumbel scores are computed inside the loops'
  bad = [s for s in inside if re.match(r'flat_|scratch_|buffer_|(global|ds)_atomic|ds_write|ds_add|ds_\w*rtn|s_barrier', s)]
  assert not bad, bad
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
