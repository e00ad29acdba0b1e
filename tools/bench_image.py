"""Times bsx_image_observation_typed (ImageObservation adapter) as a store stream: achieved HBM GB/s =
image bytes written / kernel time (HIP events on the launch stream).  Run on the GPU box.

  python tools/bench_image.py                      # float32 images, the six shapes
  python tools/bench_image.py --dtype f32,bf16,f16,u8

f32 / bf16 / f16 images are converted from observations of the same dtype, u8 images from 0/1 uint8 boards (the
reference's integer path); every dtype is timed in the same process."""
import argparse
import json
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsuite_amd.utils import wrappers  # noqa: E402

DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16, 'u8': torch.uint8}
SHAPES = [((10, 5), (84, 84, 4), 4096), ((30, 30), (84, 84, 4), 4096), ((1, 6), (84, 84, 4), 4096),
          ((1, 3), (84, 84, 4), 4096), ((10, 5), (84, 84), 16384), ((28, 28), (84, 84, 3), 4096)]


def run(obs_shape, shape, lanes, dtype=torch.float32, reps=30):
  if dtype == torch.uint8:
    obs = (torch.rand((lanes,) + obs_shape, device='cuda') < 0.3).to(torch.uint8)
  else:
    obs = torch.rand((lanes,) + obs_shape, device='cuda').to(dtype)
  out = torch.empty((lanes,) + shape, device='cuda', dtype=dtype)
  for _ in range(5):
    wrappers.to_image(shape, obs, out=out)
  ms = float('inf')
  for _ in range(3):                               # best of 3 rounds (first-touch / clock ramp noise)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
      wrappers.to_image(shape, obs, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = min(ms, e0.elapsed_time(e1) / reps)
  gb = out.numel() * out.element_size() / 1e9
  return dict(dtype=str(dtype).replace('torch.', ''), obs_shape=list(obs_shape), shape=list(shape), lanes=lanes,
              ms=round(ms, 4), GBps=round(gb / (ms / 1e3), 1), frac_of_8TBps=round(gb / (ms / 1e3) / 8000, 3),
              images_per_s=round(lanes / (ms / 1e3)))


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--dtype', default='f32', help='comma-separated image dtypes: ' + ','.join(DTYPES))
  ap.add_argument('--k', default='', help='comma-separated run lengths (BSX_IMAGE_K: 4, 8, 16 chunks per thread) to '
                  'sweep; read by the tuning build only (BSX_NATIVE_LIB=bsuite_amd/_lib/libbsuite_amd_tuning.so)')
  args = ap.parse_args()
  for k in args.k.split(',') if args.k else ['']:
    if k:
      os.environ['BSX_IMAGE_K'] = k
    for name in args.dtype.split(','):
      for obs_shape, shape, lanes in SHAPES:
        print(json.dumps(dict(run(obs_shape, shape, lanes, DTYPES[name]), **({'K': int(k)} if k else {}))), flush=True)
