"""Time of the device part of munit_amd.utils.write_2images (GPU box): the two ops.image_grid calls for a 12-tensor
sample() tuple at 256 x 256, display_size 8, against the reference's sequence of torch ops on the same tensors
(torchvision's make_grid(normalize=True) + save_image up to the uint8 grid, two host synchronisations per grid for the
minimum and the maximum).  python tools/time_grid.py [size] [display_size] [rounds]

Both are timed as a host clock around a batch of calls that ends in a device synchronise, the two alternating round by
round; the figure is the median round.  The outputs are compared first: faster and different would not be faster."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from munit_amd import ops  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else 256
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
dev = torch.device("cuda", 0)


def torch_grid(tensors, nrow):
    img = torch.cat([t[:nrow].expand(-1, 3, -1, -1) for t in tensors], 0).clone()
    lo, hi = float(img.min()), float(img.max())
    img.clamp_(lo, hi)
    img.sub_(lo).div_(max(hi - lo, 1e-5))
    nmaps, _, h, w = img.shape
    xmaps = min(nrow, nmaps)
    ymaps = (nmaps + xmaps - 1) // xmaps
    grid = img.new_zeros((3, ymaps * h, xmaps * w))
    for m in range(nmaps):
        cy, cx = divmod(m, xmaps)
        grid[:, cy * h:(cy + 1) * h, cx * w:(cx + 1) * w].copy_(img[m])
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


# the tuple sample() returns with semantic_w on: inputs (planar), decoder outputs (channels_last, tanh range) and
# colour-coded label maps in [0, 1] (channels_last), six per direction
g = torch.Generator().manual_seed(0)
outs = []
for k in range(12):
    x = torch.tanh(torch.randn(n, 3, size, size, generator=g)).to(dev)
    if k % 6 in (2, 4):
        x = ((x + 1) / 2).contiguous(memory_format=torch.channels_last)
    elif k % 6:
        x = x.contiguous(memory_format=torch.channels_last)
    outs.append(x)
halves = (outs[:6], outs[6:])


def ours():
    return [ops.image_grid(h, n) for h in halves]


def theirs():
    return [torch_grid(h, n) for h in halves]


a, b = ours(), theirs()
torch.cuda.synchronize()
diff = sum(int((x != y).sum()) for x, y in zip(a, b))
print("grids %s, bytes that differ between the kernel and the torch sequence: %d" % (tuple(a[0].shape), diff))


def batch(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


for fn, reps in ((ours, 50), (theirs, 10)):      # warm-up: code objects, allocator
    batch(fn, reps)
t_ours, t_theirs = [], []
for _ in range(rounds):
    t_ours.append(batch(ours, 2000))
    t_theirs.append(batch(theirs, 100))
mo, mt = statistics.median(t_ours), statistics.median(t_theirs)
# bytes the two passes need: every input element read twice (range, pack), every output byte written once
nbytes = sum(2 * t[:n].numel() * 4 for t in outs) + sum(x.numel() for x in a)
print("write_2images device part, 12 x (%d, 3, %d, %d): kernel %.1f us (rounds %.1f .. %.1f), torch sequence %.1f us "
      "(rounds %.1f .. %.1f), ratio %.1f; kernel traffic %.1f MB -> %.0f GB/s"
      % (n, size, size, 1e6 * mo, 1e6 * min(t_ours), 1e6 * max(t_ours), 1e6 * mt, 1e6 * min(t_theirs), 1e6 * max(t_theirs),
         mt / mo, nbytes / 1e6, nbytes / mo / 1e9))
