"""Dev tool (CPU, pure torch): how many planes are live in the tile steps the decode kernels execute.

A tile step executes when some sample of its 32 has an in-bounds texel in some plane; plane p is live in it when some
sample has one in plane p.  A sample that has left the cube along exactly one axis is still inside the one plane that does
not use that axis, so rays entering and leaving the cube produce tile steps with ONE live plane: the single-plane path of
the decode kernels (tt_device.h, "plane mask of a tile step").  This re-derives the table of that
section -- and the live-tile / in-bounds-pair fractions bench.py reports from the device counters -- without a GPU.

usage: python tools/plane_liveness.py [--tile-sb 2] [--res 256] [--samples 128] [--plane 256] [--near 0.1] [--far 4.0]
(defaults: the headline scene of bench.py --config 1)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cpu_ref as O  # noqa: E402

BW = {1: 8, 2: 4, 4: 4, 8: 2, 16: 2, 32: 1}  # pixel block of a tile, tt_make_geom
BH = {1: 4, 2: 4, 4: 2, 8: 2, 16: 1, 32: 1}
PLANE_AXES = ((0, 1), (0, 2), (2, 1))  # plane p samples at (u, v) = these world axes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile-sb", type=int, default=2, choices=sorted(BW))
    ap.add_argument("--res", type=int, default=256, help="image height = width")
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--plane", type=int, default=256, help="plane height = width (texels)")
    ap.add_argument("--near", type=float, default=0.1)
    ap.add_argument("--far", type=float, default=4.0)
    ap.add_argument("--radius", type=float, default=1.0)
    a = ap.parse_args()
    H = W = a.res
    S, sb, bw, bh = a.samples, a.tile_sb, BW[a.tile_sb], BH[a.tile_sb]
    if H % bh or W % bw or S % sb:
        sys.exit("image and sample count must be multiples of the tile shape for this model")
    ro, rd, _, _ = O.make_cameras(1, H, W)
    ts, te = O.uniform_intervals(1, S, a.near, a.far)
    tm = ((ts + te) / 2.0).reshape(1, 1, S, 1)
    pos = (ro[0].reshape(H, W, 1, 3) + rd[0].reshape(H, W, 1, 3) * tm) / a.radius  # plane coordinates in [-1, 1]
    # some bilinear corner in bounds (zeros padding, align_corners=False): floor(ix) in [-1, W - 1], ix = ((g + 1) W - 1) / 2
    ix = ((pos + 1.0) * a.plane - 1.0) / 2.0
    inb_axis = (torch.floor(ix) >= -1) & (torch.floor(ix) <= a.plane - 1)  # (H, W, S, 3)
    inb = torch.stack([inb_axis[..., u] & inb_axis[..., v] for u, v in PLANE_AXES], -1)  # (H, W, S, plane)
    tiles = inb.reshape(H // bh, bh, W // bw, bw, S // sb, sb, 3).permute(0, 2, 4, 1, 3, 5, 6).reshape(-1, 32, 3)
    live_planes = tiles.any(dim=1)  # (tile steps, plane)
    n_live = live_planes.sum(dim=1)
    executed = n_live > 0
    n_exec = int(executed.sum())
    print(f"tile: {bw}x{bh} pixels x {sb} samples; {tiles.shape[0]} tile steps, {n_exec} executed "
          f"(live tile fraction {n_exec / tiles.shape[0]:.4f})")
    pairs = tiles[executed].sum().item()
    print(f"in-bounds (plane, sample) pairs: {pairs / (3 * 32 * n_exec):.4f} of the executed tile steps, "
          f"{pairs / (3 * 32 * tiles.shape[0]):.4f} of all")
    print("| live planes in the tile step | tile steps | share |")
    print("|---|---|---|")
    for k in (3, 2, 1):
        n = int((n_live == k).sum())
        print(f"| {k} | {n} | {100.0 * n / n_exec:.3f} % |")
    one = live_planes[n_live == 1]
    print("single-plane tile steps by plane (0, 1, 2):", [int(one[:, p].sum()) for p in range(3)])


if __name__ == "__main__":
    main()
