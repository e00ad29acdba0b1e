"""CPU: the hint word of the one-launch deep_sea step (bsuite_amd/csrc/deep_sea_hint.h), through gcc, against the C
oracle — for every cell of a board, both reset states and actions inside and outside the action_spec, the hot cell the
stream selects from the hint is the hot cell of the board the oracle shows after that call; and the three fields of
the word cannot run into each other at the largest board."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import coracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTIONS = (-1, 0, 1, 2)


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('hint') / 'deep_sea_hint_shim.so')
  subprocess.check_call(['gcc', '-O2', '-std=gnu99', '-Wall', '-Werror', '-shared', '-fPIC',
                         os.path.join(ROOT, 'tests', 'csrc', 'deep_sea_hint_shim.c'), '-o', so])
  return ctypes.CDLL(so)


def _ptr(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def _mapping_bits(mapping):
  bits = np.zeros(64 * 64 // 32, np.uint32)
  for idx in np.nonzero(mapping.reshape(-1) == 1)[0]:
    bits[idx >> 5] |= np.uint32(1 << (int(idx) & 31))
  return bits


def _hints(shim, N, bits, row, col, reset, action):
  n = row.shape[0]
  hint, hot = np.zeros(n, np.uint32), np.zeros(n, np.int32)
  shim.shim_hint_hot(n, N, _ptr(bits), _ptr(row), _ptr(col), _ptr(reset), _ptr(action), _ptr(hint), _ptr(hot))
  return hint, hot


@pytest.mark.parametrize('size', [2, 4, 30, 64])
def test_hint_selects_the_oracles_next_board(shim, size):
  kw = dict(size=size, mapping_seed=size + 1)
  rows, cols, resets = (x.reshape(-1).astype(np.int32) for x in np.meshgrid(np.arange(size), np.arange(size), [0, 1], indexing='ij'))
  B = rows.shape[0]
  orc = coracle.OracleEnv('deep_sea', kw, np.arange(B, dtype=np.uint64), seed=1)
  bits = _mapping_bits(orc.mapping)
  for act in ACTIONS:
    orc.s['row'][:], orc.s['col'][:], orc.s['bad'][:], orc.reset_next[:] = rows, cols, 0, resets
    action = np.full(B, act, np.int32)
    _, _, _, obs = orc.call(action, 5)
    flat = obs.reshape(B, -1)
    assert ((flat == 0) | (flat == 1)).all() and (flat.sum(axis=1) <= 1).all()
    want = np.where(flat.any(axis=1), flat.argmax(axis=1), -1).astype(np.int32)
    _, hot = _hints(shim, size, bits, rows, cols, resets, action)
    np.testing.assert_array_equal(hot, want, err_msg=f'N={size} action={act}')
  # both outcomes occur, and so does the all-zero board (the last row) and the reset board
  assert (want == -1).any() and (want == 0).any() and (want > 0).any()


def test_fields_cannot_overflow_at_the_largest_board(shim):
  N = shim.shim_max_size()
  fb, ls, ms = shim.shim_hint_field_bits(), shim.shim_hint_l_shift(), shim.shim_hint_m_shift()
  assert N == 64
  assert (1 << fb) >= N * N + 1                                    # hot cell + 1, and 0 for the all-zero board
  assert ls >= fb and ms >= ls + fb and ms + 1 <= 32                # R | L | M: disjoint, inside 32 bits
  rows, cols, resets = (x.reshape(-1).astype(np.int32) for x in np.meshgrid(np.arange(N), np.arange(N), [0, 1], indexing='ij'))
  mask = (1 << fb) - 1
  for fill in (0, 0xFFFFFFFF):                                      # the mapping bit clear / set in every cell
    bits = np.full(64 * 64 // 32, fill, np.uint32)
    hint, _ = _hints(shim, N, bits, rows, cols, resets, np.zeros(rows.shape[0], np.int32))
    r, l, m = hint & mask, (hint >> ls) & mask, hint >> ms
    assert int(r.max()) == N * N and int(l.max()) == N * N - 1      # the last cell of the board + 1; its left neighbour + 1
    np.testing.assert_array_equal(r | (l << ls) | (m << ms), hint)  # nothing outside the three fields
    assert set(np.unique(m[resets == 0])) == {1 if fill else 0} and (m <= 1).all()
    # the fields decoded on their own are the cells of the move right / left: nothing carried from one into another
    live = (resets == 0) & (rows + 1 < N)
    np.testing.assert_array_equal(r[live], ((rows + 1) * N + np.minimum(cols + 1, N - 1) + 1)[live])
    np.testing.assert_array_equal(l[live], ((rows + 1) * N + np.maximum(cols - 1, 0) + 1)[live])
    assert (r[(resets == 0) & (rows + 1 == N)] == 0).all() and (l[(resets == 0) & (rows + 1 == N)] == 0).all()
    assert (r[resets == 1] == 1).all() and (l[resets == 1] == 1).all()
