"""The depth-ranked sample tiles of the coarse-level backward (grid_encode_merge.hip: k_merge_tile_order), through their
torch restatement tools/merge_tiles.py — the rule `tools/headline_bwd_routes.py --count` counts with.  Whatever the inputs,
the tiling must be a permutation of the samples (a sample dropped or taken twice is a wrong gradient); on neighbouring
parallel rays it must merge clearly better than consecutive blocks, and on a stream without ray structure no worse.
Runs without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import merge_tiles as mt  # noqa: E402


def _rays(n_rays, n_samples, seed=0, step=1 / 300, spacing=1 / 800):
    """Neighbouring parallel rays of one scanline: origins `spacing` apart, samples `step` apart (the bench frame's
    middle: ~300 samples per ray across the cube, 800 pixels across it)."""
    rng = np.random.default_rng(seed)
    d = np.array([0.62, 0.33, 0.71])
    d /= np.linalg.norm(d)
    side = np.cross(d, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    o = np.array([0.07, 0.31, 0.05]) + side[None, :] * spacing * np.arange(n_rays)[:, None]
    t = step * (np.arange(n_samples)[None, :] + rng.uniform(0, 1, size=(n_rays, 1)))
    return torch.as_tensor((o[:, None, :] + d[None, None, :] * t[:, :, None]).reshape(-1, 3), dtype=torch.float32)


def _degenerate(name, N):
    x = _rays(-(-N // 200), 200)[:N].clone()
    if name == "one_position":
        x[:] = torch.tensor([0.3, 0.4, 0.5])
    elif name == "plane_across_axis":      # every sample at depth 0 along the step direction of the first samples
        x = torch.rand((N, 3), generator=torch.Generator().manual_seed(1))
        x[:, 0] = 0.5
        x[:4] = torch.tensor([[0.1, 0.5, 0.5], [0.2, 0.5, 0.5], [0.3, 0.5, 0.5], [0.4, 0.5, 0.5]])[: min(N, 4)]
    elif name == "zero_axis":
        x[:32] = x[0]
    elif name == "outside_and_nan":
        x[4::7] += 2.0
        x[12::64, 1] = float("nan")
        x[min(1, N - 1), 0] = float("nan")  # an axis candidate
    elif name == "shuffled":
        x = x[torch.randperm(N, generator=torch.Generator().manual_seed(2))]
    return x


@pytest.mark.parametrize("W,S", [(8192, 8), (4096, 4), (2048, 16), (16384, 16)])
@pytest.mark.parametrize("N", [1, 7, 1023, 8191, 8192, 8193, 70001])
@pytest.mark.parametrize("name", ["rays", "one_position", "plane_across_axis", "zero_axis", "outside_and_nan", "shuffled"])
def test_tiling_is_a_permutation_of_the_samples(name, N, W, S):
    x = _degenerate(name, N)
    blocks = mt.block_samples(x, W, S)
    assert blocks.shape == (-(-N // 1024), 1024)
    taken = blocks[blocks < N]
    assert taken.numel() == N and torch.equal(torch.sort(taken).values, torch.arange(N))
    assert int(blocks.max()) <= N
    # a block that exists holds at least one sample (the kernel launches ceil(N / 1024) blocks per level)
    assert bool((blocks < N).any(dim=1).all())
    # every window is a permutation of its own samples
    for w in range(-(-N // W)):
        order, n_sub = mt.window_order(x, w * W, N, W, S)
        assert torch.equal(torch.sort(order).values, torch.arange(W // S))
        assert n_sub in (1, 2, 4, 8, 16) and n_sub <= W // 1024


def _cells(x, blocks, resolutions):
    total = 0
    for R in resolutions:
        c = torch.floor(x * (R - 2) + 0.5).to(torch.int64)
        total += mt.cells_per_block(c[:, 0] | c[:, 1] << 16 | c[:, 2] << 32, blocks)
    return total


RES = [16, 26, 42, 68, 110]


def test_neighbouring_rays_merge_better_and_a_shuffled_stream_no_worse():
    """64 rays of 256 samples (two windows of 32 rays): a consecutive block is the full depth of 4 rays, a ranked tile a
    32-sample slab of 32 rays.  The count on the bench frame says 0.57 of the cells; a quarter fewer is asked here, half of
    what the slab shape promises.  Shuffled, the depths fall at every other segment, the window splits itself into its
    1,024-sample blocks and the count is the consecutive one (the frame-sized count saw -0.9 %; within 2 % is asked)."""
    x = _rays(64, 256, seed=3)
    cons, tiles = _cells(x, mt.block_samples(x, 0), RES), _cells(x, mt.block_samples(x), RES)
    assert mt.window_order(x, 0, x.shape[0])[1] == 1
    assert tiles <= 0.75 * cons, (tiles, cons)
    xs = x[torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(4))]
    cons_s, tiles_s = _cells(xs, mt.block_samples(xs, 0), RES), _cells(xs, mt.block_samples(xs), RES)
    assert abs(tiles_s - cons_s) <= 0.02 * cons_s, (tiles_s, cons_s)
    assert cons_s > 2 * cons           # the shuffled stream really has no structure left


def test_short_rays_fall_back_to_the_consecutive_blocks():
    """Rays far shorter than a 32nd of the window: eight sub-windows, every block holds the samples it held before."""
    x = _rays(512, 24, seed=5)
    order, n_sub = mt.window_order(x, 0, x.shape[0])
    assert n_sub == 8
    blocks = mt.block_samples(x)
    cons = mt.block_samples(x, 0)
    assert torch.equal(torch.sort(blocks, dim=1).values, torch.sort(cons, dim=1).values)
