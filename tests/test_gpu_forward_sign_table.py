"""Bit-plane forward with the sign-nibble table (unit_finish_lut: packed FMAs on +-1.0f patterns from LDS) on every
level, on the dense levels only, and without it (CNC_FWD_LUT = 1 / 2 / 0, read per launch): bit-equal to the oracle and
to the fp32 gather with the STE flag, at every feature width, at 1 to 17 levels (dense and hashed), ragged point
counts, points outside the box, point-major rows, and the bench's own marched chunk at full size."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import make_grid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _res(D, L):
    """L resolutions growing by ~1.4 per level: dense coarse levels, hashed fine ones (2^10 rows)."""
    r0 = 6 if D == 3 else 10
    return [int(r0 * 1.4 ** l) for l in range(L)]


def _points(N, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, size=(N, D)).astype(np.float32)
    x[0] = 0.0
    x[1] = 1.0
    x[2, 0] = -1e-3                           # outside the box: zeros
    x[3, D - 1] = 1.0 + 1e-3
    x[4] = np.float32(1.0) - np.float32(2 ** -24)
    x[5::97] = rng.uniform(-0.5, 1.5, size=x[5::97].shape).astype(np.float32)     # more outside (and inside) points
    return x


def _table(res, D, F, seed):
    offs, resl, emb = make_grid(res, 10, D, F, seed=seed)
    emb[::7] = 0.0                            # sign(0) = +1
    emb[3::7] = -0.0
    return offs, resl, emb


def _bits_forward(dev, x, bits, offs, resl, D, F, L, lut, monkeypatch, ld=0, col=0):
    from cnc_amd.backends import gridencoder_backend as be
    t = lambda a: torch.as_tensor(a, device=dev)
    N = x.shape[0]
    monkeypatch.setenv("CNC_FWD_LUT", str(lut))
    if ld:
        out = torch.full((N, ld), 7.0, device=dev)
        be.grid_encode_forward_bits(t(x), bits, t(offs), t(resl), out, N, D, F, L, 128, None, None, None,
                                    out_ld=ld, out_col=col)
    else:
        out = torch.full((L, N, F), 7.0, device=dev)
        be.grid_encode_forward_bits(t(x), bits, t(offs), t(resl), out, N, D, F, L, 128)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("F", [1, 2, 4, 8, 16, 32])
@pytest.mark.parametrize("L", [1, 2, 15, 16, 17])
def test_sign_table_forward_bit_exact(cuda, oracle, monkeypatch, D, F, L):
    from cnc_amd.backends import gridencoder_backend as be
    res = _res(D, L)
    offs, resl, emb = _table(res, D, F, seed=100 + 10 * L + F)
    N = 1000 + 3 * L + F                      # ragged: not a multiple of the wave or the block
    x = _points(N, D, seed=7 * L + D)
    t = lambda a: torch.as_tensor(a, device=cuda)
    want = oracle.grid_encode_forward(x, emb, offs, resl, ste_binary=True)
    bits = be.pack_sign_bits(t(emb))
    got = _bits_forward(cuda, x, bits, offs, resl, D, F, L, 1, monkeypatch)
    assert np.array_equal(got, want)
    for lut in (0, 2):
        assert np.array_equal(_bits_forward(cuda, x, bits, offs, resl, D, F, L, lut, monkeypatch), got)
    ste = torch.empty((L, N, F), device=cuda)
    be.grid_encode_forward(t(x), t(emb), t(offs), t(resl), ste, N, D, F, L, 0, 128, 0.0, None, None, None,
                           ste_binary=True)
    assert np.array_equal(ste.cpu().numpy(), got)


@pytest.mark.parametrize("N", [1, 255, 257, 4097])
@pytest.mark.parametrize("D,F,L", [(3, 8, 16), (3, 8, 17), (3, 4, 15), (2, 16, 17), (3, 32, 2)])
def test_sign_table_forward_ragged_and_point_major(cuda, oracle, monkeypatch, N, D, F, L):
    """Ragged point counts in both layouts; point-major rows (out_ld / out_col) inside a wider matrix, the neighbours'
    columns untouched."""
    from cnc_amd.backends import gridencoder_backend as be
    res = _res(D, L)
    offs, resl, emb = _table(res, D, F, seed=200 + N)
    x = _points(max(N, 8), D, seed=N)[:N]
    want = oracle.grid_encode_forward(x, emb, offs, resl, ste_binary=True)      # [L, N, F]
    bits = be.pack_sign_bits(torch.as_tensor(emb, device=cuda))
    assert np.array_equal(_bits_forward(cuda, x, bits, offs, resl, D, F, L, 1, monkeypatch), want)
    for ld, col in ((L * F, 0), (L * F + 12, 4)):
        got = _bits_forward(cuda, x, bits, offs, resl, D, F, L, 1, monkeypatch, ld=ld, col=col)
        assert np.array_equal(got[:, col:col + L * F].reshape(N, L, F).transpose(1, 0, 2), want)
        assert np.all(got[:, :col] == 7.0) and np.all(got[:, col + L * F:] == 7.0)


def test_bench_marched_chunk_full_size(cuda, oracle, monkeypatch):
    """bench.py's table (16L x 2^19 x F8) and the first 2^19 samples of its marched probe chunk: every sign-table mode
    gives the oracle's and the fp32 STE gather's answer, bit for bit."""
    sys.path.insert(0, ROOT)
    import bench
    from cnc_amd.backends import gridencoder_backend as be
    w = bench.build_workload(cuda, 0)
    box = {}
    bench.march_frame(w, box)
    x = bench.probe_chunk_of(box["ex"]["positions"])[: 1 << 19].contiguous()
    N, F, L, D = x.shape[0], bench.F, bench.L, bench.D
    assert N == 1 << 19
    be.pack_sign_bits(w["table"], w["bits"], w["clip"])
    out = torch.empty((L, N, F), device=cuda)
    got = []
    for lut in ("1", "0", "2"):
        monkeypatch.setenv("CNC_FWD_LUT", lut)
        be.grid_encode_forward_bits(x, w["bits"], w["offsets"], w["resolutions"], out, N, D, F, L, 128)
        torch.cuda.synchronize()
        got.append(out.cpu().numpy())
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    ste = torch.empty_like(out)
    be.grid_encode_forward(x, w["table"], w["offsets"], w["resolutions"], ste, N, D, F, L, 0, 128, 0.0, None, None,
                           None, ste_binary=True)
    assert np.array_equal(ste.cpu().numpy(), got[0])
    want = oracle.grid_encode_forward(x.cpu().numpy(), w["table"].cpu().numpy(), w["offsets"].cpu().numpy(),
                                      w["resolutions"].cpu().numpy(), ste_binary=True, threads=oracle.max_threads())
    assert np.array_equal(got[0], want)
