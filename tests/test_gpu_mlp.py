"""Fused MFMA MLP forward vs torch fp32 (nn.Sequential on hipBLASLt): the MFMA result is a k-ordered
fp32 fmaf chain, so agreement is at fp32 round-off."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


REL = 2e-5         # of max(1, |want|_max): fp32 round-off of a k-ordered fmaf chain


def make_seq(dims, dev):
    """Linear-ReLU-Linear[-ReLU-Linear] of the given widths on `dev`, with asymmetric, non-trivial weights."""
    from cnc_amd.mlp import Linear
    layers = []
    for i in range(len(dims) - 1):
        layers.append(Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(nn.ReLU(inplace=True))
    seq = nn.Sequential(*layers).to(dev)
    for l in seq:
        if isinstance(l, nn.Linear):   # asymmetric, non-trivial weights
            with torch.no_grad():
                l.weight.copy_(torch.randn_like(l.weight) / dims[0] ** 0.5 + torch.arange(l.weight.shape[1], device=dev) * 1e-3)
                l.bias.copy_(torch.randn_like(l.bias))
    return seq


def chain64(seq, x):
    """The network in double precision."""
    ref = x.double()
    for l in seq:
        ref = torch.relu(ref) if isinstance(l, nn.ReLU) else ref @ l.weight.double().t() + l.bias.double()
    return ref


@pytest.mark.parametrize("dims", [(255, 160, 80), (95, 160, 160, 3), (25, 32, 32, 8), (64, 16, 16), (7, 48, 33)])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 4099, 1 << 16])
def test_fused_mlp_forward_matches_torch(cuda, dims, N):
    from cnc_amd.mlp import FusedMLPForward
    torch.manual_seed(len(dims) * 1000 + N)
    seq = make_seq(dims, cuda)
    fused = FusedMLPForward(seq)
    x = torch.randn(N, dims[0], device=cuda)
    with torch.no_grad():
        want = seq(x)
    got = fused(x)
    assert got.shape == want.shape
    scale = want.abs().max().clamp_min(1.0)
    assert (got - want).abs().max() <= REL * scale
    # a double-precision check pins both to the true value
    ref = chain64(seq, x)
    assert (got.double() - ref).abs().max() <= REL * scale
    # strided input view (columns of a wider matrix) and weight update tracking.  (At N = 2^16 and 16 columns `wide` is
    # exactly 4 MiB: in a fresh segment the window's last row ends with the allocation, and a kernel that read the padded K
    # of THAT row faulted whenever nothing was mapped behind it — behind tests/test_gpu_march.py on some boxes; round 6 took
    # that read out of both kernels.  The fresh segment makes the case likelier, it cannot force the mapping.)
    torch.cuda.empty_cache()
    wide = torch.randn(N, dims[0] + 9, device=cuda)
    assert torch.allclose(fused(wide[:, 4:4 + dims[0]]), seq(wide[:, 4:4 + dims[0]]), rtol=0, atol=2e-5 * float(scale) + 1e-4)
    with torch.no_grad():
        seq[0].weight.mul_(0.5)
    assert (fused(x) - seq(x)).abs().max() <= 2e-5 * scale


@pytest.mark.parametrize("dims", [(255, 160, 80), (95, 160, 160, 3), (64, 160, 96)])
@pytest.mark.parametrize("N", [1, 31, 33, 5000])
@pytest.mark.parametrize("aligned", [True, False])
def test_fused_mlp_32_row_kernel(cuda, dims, N, aligned):
    """v_mfma_f32_32x32x2 kernel (32 rows per wave, cnc_mlp_forward32) vs torch: fp32 round-off only;
    ragged row counts, 16-byte aligned and unaligned input rows."""
    import torch.nn as nn
    from cnc_amd.mlp import FusedMLPForward
    torch.manual_seed(N + len(dims))
    layers = []
    for i in range(len(dims) - 1):
        layers.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(nn.ReLU())
    seq = nn.Sequential(*layers).to(cuda)
    fused = FusedMLPForward(seq, rows_per_wave=32)
    if aligned:
        x = torch.randn(N, (dims[0] + 3) // 4 * 4, device=cuda)[:, :dims[0]]
    else:
        x = torch.randn(N, dims[0] + 1, device=cuda)[:, 1:].contiguous() if dims[0] % 4 else \
            torch.randn(N, dims[0] + 1, device=cuda)[:, :dims[0]]
    with torch.no_grad():
        want = seq(x)
        got = fused(x)
    assert got.shape == want.shape
    assert (got - want).abs().max() <= 2e-5 * (1 + want.abs().max())


def _chain64_in_chunks(seq, x, rows=1 << 15):
    """`chain64` over row chunks (the float64 activations of half a million rows at once would be ~0.7 GB a layer)."""
    return torch.cat([chain64(seq, x[r:r + rows]) for r in range(0, x.shape[0], rows)])


# Both kernels cap their grid at 256 * 32 = 8192 one-wave blocks (csrc/mlp.hip, `blocks` / `bw`); a block then walks
# `tile += gridDim.x`.  (rows per wave, rows per tile, dims, N):
GRID_CAP = 256 * 32
BEHIND_THE_CAP = [
    # k_mlp_forward, 16-row tiles: 16 * 8192 + 17 rows = 8194 tiles, blocks 0 and 1 take a second tile, the last tile
    # holds one row.  Run-time widths, then the two compile-time instances <10, 10, 1> and <10, 5, 0>.
    (16, 16, (25, 32, 32, 8), 16 * GRID_CAP + 17),
    (16, 16, (95, 160, 160, 3), 16 * GRID_CAP + 17),
    (16, 16, (255, 160, 80), 16 * GRID_CAP + 17),
    # k_mlp_forward64, 64-row tiles.  2^17 rows: the size from which cnc_amd/field.py calls this kernel (2048 full
    # tiles, one trip).  64 * 8192 + 65 rows = 8194 tiles: blocks 0 and 1 take a second tile, the last tile has one
    # live row and an empty second 32-row half.
    (32, 64, (95, 160, 160, 3), 1 << 17),
    (32, 64, (64, 160, 96), 1 << 17),
    (32, 64, (95, 160, 160, 3), 64 * GRID_CAP + 65),
    (32, 64, (64, 160, 96), 64 * GRID_CAP + 65),
]


@pytest.mark.parametrize("rows_per_wave,tile_rows,dims,N", BEHIND_THE_CAP)
def test_tile_loop_behind_the_grid_cap(cuda, rows_per_wave, tile_rows, dims, N):
    """The blocks' second trip through `for (tile = blockIdx.x; tile < tiles; tile += gridDim.x)`.

    (a) every output against the float64 chain within the file's REL of max(1, |want|_max);
    (b) the rows of the second trip and the 64 rows on either side of the first trip's end equal, bit for bit, the same
        rows evaluated alone in a call that stays inside the first trip: an output element is one k-ordered fmaf chain
        whose order does not depend on the tile the row sits in.

    Measured on the MI355X, the largest |got - float64| / (REL scale): 16-row kernel 0.0192 ((255, 160, 80)), of that
    0.0092 on the rows behind the cap; 64-row kernel 0.0204 ((64, 160, 96) at N = 2^17), 0.0119 behind the cap
    ((64, 160, 96) at N = 524353).  (b) held in all five cases that have a second trip."""
    from cnc_amd.mlp import FusedMLPForward
    torch.manual_seed(len(dims) * 1000 + N % 9973 + rows_per_wave)
    seq = make_seq(dims, cuda)
    fused = FusedMLPForward(seq, rows_per_wave=rows_per_wave)
    x = torch.randn(N, dims[0], device=cuda)
    got = fused(x)
    assert got.shape == (N, dims[-1])
    ref = _chain64_in_chunks(seq, x)
    scale = ref.abs().max().clamp_min(1.0)
    err = torch.cat([(got[r:r + (1 << 16)].double() - ref[r:r + (1 << 16)]).abs().amax(dim=1)
                     for r in range(0, N, 1 << 16)])
    first_trip = tile_rows * GRID_CAP
    print(f"MLP {rows_per_wave}-row kernel dims={dims} N={N}: |got - float64| / (REL scale) {float(err.max() / (REL * scale)):.3g}"
          + (f", behind the cap {float(err[first_trip:].max() / (REL * scale)):.3g}" if N > first_trip else ""))
    assert err.max() <= REL * scale
    if N > first_trip:
        lo = first_trip - 64
        alone = fused(x[lo:].clone())
        assert alone.shape[0] == N - lo <= first_trip
        assert torch.equal(alone.view(torch.int32), got[lo:].view(torch.int32)), \
            f"rows {lo}..{N - 1} differ from the same rows in a call of their own"
        assert float(got[first_trip:].abs().max()) > 0


def test_field_glue_kernels_equal_the_op_chain(cuda):
    """normalise + selector, density activation, SH-4 encoding and the head-input concat as single kernels
    (cnc_amd/csrc/field_glue.hip) vs the reference's op chain (ngp.py:516-547): same rgb / density and the
    same parameter gradients, with and without gradients enabled, for points inside and outside the box."""
    from cnc_amd.field import NGPRadianceField_mygrid_2D3D
    torch.manual_seed(0)
    f = NGPRadianceField_mygrid_2D3D(aabb=[-1.5] * 3 + [1.5] * 3, n_features_per_level=8, n_neurons=160,
                                     resolutions_list=(18, 24, 33, 44), log2_hashmap_size=12,
                                     resolutions_list_2D=(130, 258), log2_hashmap_size_2D=10).to(cuda)
    with torch.no_grad():
        for p in f.parameters():
            if p.dim() == 2 and p.shape[1] != 8:
                p.mul_(3.0)                  # livelier MLPs than the default init
    g = torch.Generator(device="cpu").manual_seed(1)
    N = 5000
    pos = ((torch.rand(N, 3, generator=g) * 3.4 - 1.7)).to(cuda)          # ~20 % outside the box
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).to(cuda)
    go_rgb, go_den = torch.randn(N, 3, generator=g).to(cuda), torch.randn(N, 1, generator=g).to(cuda)
    res = {}
    for fused in (False, True):
        f.fused_glue = fused
        for p in f.parameters():
            p.grad = None
        rgb, den = f(pos, d)
        ((rgb * go_rgb).sum() + (den * go_den).sum()).backward()
        with torch.no_grad():
            den_only = f.query_density(pos)
            den2, feat = f.query_density(pos, return_feat=True)
        res[fused] = (rgb.detach(), den.detach(), den_only, feat, [p.grad.clone() for p in f.parameters()])
    a, b = res[False], res[True]
    assert (b[1] == 0).float().mean() > 0.1 and (b[1] > 0).float().mean() > 0.5          # selector at work
    assert torch.allclose(a[0], b[0], rtol=1e-5, atol=1e-6) and torch.allclose(a[1], b[1], rtol=1e-5, atol=1e-7)
    assert torch.allclose(a[2], b[2], rtol=1e-5, atol=1e-7) and torch.allclose(a[3], b[3], rtol=1e-5, atol=1e-6)
    for ga, gb in zip(a[4], b[4]):
        assert float((ga - gb).abs().max()) <= 2e-4 * max(float(ga.abs().max()), 1e-12)


@pytest.mark.parametrize("N,C", [(1, 4), (777, 80), (100003, 160), (5000, 256)])
def test_relu_backward_with_bias_sums(cuda, N, C):
    """cnc_relu_backward_bias through `_LinearReLUSplitK`: the masked gradient equals aten::threshold_backward bit for
    bit; the bias gradient equals the column sums within float32 summation error; dX / dW as the op chain."""
    from cnc_amd.mlp import _LinearReLUSplitK
    g = torch.Generator(device="cpu").manual_seed(N + C)
    x = torch.randn(N, 24, generator=g).to(cuda).requires_grad_()
    w = (torch.randn(C, 24, generator=g) * 0.3).to(cuda).requires_grad_()
    b = torch.randn(C, generator=g).to(cuda).requires_grad_()
    go = torch.randn(N, C, generator=g).to(cuda)
    y = _LinearReLUSplitK.apply(x, w, b)
    y.backward(go)
    x2, w2, b2 = (t.detach().clone().requires_grad_() for t in (x, w, b))
    y2 = torch.relu(torch.nn.functional.linear(x2, w2, b2))
    y2.backward(go)
    mask = torch.ops.aten.threshold_backward(go, y.detach(), 0.0)
    want_b = mask.double().sum(0)
    assert torch.allclose(b.grad.double(), want_b, rtol=1e-5, atol=1e-5 * float(mask.abs().sum(0).max()) + 1e-6)
    assert torch.allclose(x.grad, x2.grad, rtol=1e-4, atol=1e-4)
    assert torch.allclose(w.grad, w2.grad, rtol=1e-3, atol=1e-3 * float(w2.grad.abs().max()))
