"""The depth-ranked sample tiles of k_grid_encode_bwd_merge (grid_encode_merge.hip, k_merge_tile_order), restated in torch:
which samples each 1,024-sample block of the coarse-level backward holds.  Same window, segments, axis, 22-bit depth key,
ray count and sub-window split as the kernel, in the same fp32 operations, so that `tools/headline_bwd_routes.py --count`
counts the cells the kernel really sends and tests/test_merge_tile_ranking.py can check the rule without a GPU."""
import torch

PAST_END, UNUSABLE = 0x3FFFFF, 0x3FFFFE
MIN_RES = 52          # kMergeTileMinRes: levels of a lower resolution keep the consecutive tiling


def window_order(x, base, N, W=8192, S=8, MB=1024):
    """Segments of the window that starts at sample `base`, in the order the window's tiles take them: int64 [W // S]
    (entries >= the window's segment count: no segment), and the number of sub-windows the window split itself into."""
    segs, tiles = W // S, W // MB
    assert segs <= MB and segs * S == W and tiles * MB == W and 1 <= S <= 16
    n_in = min(N - base, W)
    n_seg = -(-n_in // S)
    ax = torch.zeros(3, dtype=torch.float32)
    if n_in >= 2:
        a = torch.tensor([base + min(k * 11, n_in - 2) for k in range(3)])
        cand = x[a + 1] - x[a]
        sq = cand * cand
        l0, l1, l2 = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]).tolist()
        m0 = (l1 > l2 and l0 > l2) if l0 <= l1 else l0 <= l2
        m2 = (l1 > l2 and l0 <= l2) if l0 <= l1 else (l0 > l2 and l1 <= l2)
        ax = cand[0] if m0 else cand[2] if m2 else cand[1]
    q = torch.full((MB,), PAST_END, dtype=torch.int64)
    mid = base + torch.clamp(torch.arange(n_seg) * S + S // 2, max=n_in - 1)
    xm = x[mid]
    dep = (xm[:, 0] * ax[0] + xm[:, 1] * ax[1]) + xm[:, 2] * ax[2]
    usable = ((xm >= 0) & (xm <= 1)).all(dim=1) & (dep == dep)
    u = dep.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = u ^ torch.where(u >> 31 != 0, torch.tensor(0xFFFFFFFF), torch.tensor(0x80000000))
    q[:n_seg] = torch.where(usable, torch.clamp(u >> 10, max=UNUSABLE - 1), torch.tensor(UNUSABLE))
    i = torch.arange(1, MB)
    n_rays = 1 + int(((i % 64 != 0) & (q[1:] < q[:-1]) & (q[:-1] < UNUSABLE)).sum())
    have, want = n_rays * segs * 5, n_seg * 32 * 7
    n_sub = 1 if have < want else 2 if have < 2 * want else 4 if have < 4 * want else 8 if have < 8 * want else 16
    n_sub = min(n_sub, tiles)
    key = (q << 10 | torch.arange(MB))[:segs].reshape(n_sub, segs // n_sub)
    return (torch.sort(key, dim=1).values & (MB - 1)).reshape(-1), n_sub


def block_samples(x, W=8192, S=8, MB=1024):
    """Sample index of every (block, thread) of the ranked tiling of the points x [N, 3]: int64 [ceil(N / MB), MB], N = none.
    W = 0: the consecutive tiling."""
    N = x.shape[0]
    n_blocks = -(-N // MB)
    if W == 0:
        b = torch.arange(n_blocks * MB).reshape(n_blocks, MB)
        return torch.where(b < N, b, torch.tensor(N))
    x = x.detach().to("cpu", torch.float32)
    tiles = W // MB
    out = torch.full((-(-N // W) * tiles, MB), N, dtype=torch.int64)
    for w in range(-(-N // W)):
        order, _ = window_order(x, w * W, N, W, S, MB)
        b = w * W + (order[:, None] * S + torch.arange(S)[None, :]).reshape(tiles, MB)
        out[w * tiles:(w + 1) * tiles] = torch.where(b < N, b, torch.tensor(N))
    return out[:n_blocks]


def cells_per_block(keys, blocks):
    """Distinct cell keys per block, summed: what the merge kernel sends atomics for.  keys: int64 [N] (>= 0), blocks: from
    block_samples."""
    N = keys.shape[0]
    k = torch.cat([keys, torch.tensor([-1])])[blocks]              # -1: the empty slots
    k = torch.sort(k, dim=1).values
    first = torch.ones_like(k, dtype=torch.bool)
    first[:, 1:] = k[:, 1:] != k[:, :-1]
    return int((first & (k >= 0)).sum())
