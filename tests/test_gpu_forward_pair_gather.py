"""Bit-plane forward with the paired x-neighbour gathers (unit_issue_fast<D, 8, true>: one aligned word load per corner
pair on the hashed levels; CNC_FWD_PAIR = 0 off / 1 default policy / 2 every hashed level that qualifies, read per
launch): bit-equal to the oracle and to the unpaired path on small hashed tables (down to one word per level), at every
cell residue of every level, at the other feature widths, on a misaligned plane, at ragged point counts, in point-major
rows, under the default policy and on the bench's own table."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import make_grid
from test_gpu_forward_sign_table import _points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 8 levels per table size (log2 rows): dense coarse levels (R^D rows fit), hashed ones above; R = 2 has no inner cell
RES = {3: [2, 3, 6, 11, 18, 47, 130, 300],
       4: [2, 4, 5, 9, 19, 33, 130, 257],
       6: [2, 4, 8, 9, 17, 40, 129, 300],
       10: [4, 10, 11, 32, 33, 70, 155, 520]}


def _cell_points(res, D, seed):
    """The sign-table test's edge / outside points, plus one point in every cell g = 0 .. R-3 of every level along x
    (x (R - 2) + 0.5 = g + 0.75: every residue of g mod 16, g % 8 == 7 and the last cells included), other axes random."""
    rng = np.random.default_rng(seed)
    parts = [_points(1200, D, seed)]
    for R in res:
        if R < 3:
            continue
        p = rng.uniform(0, 1, size=(R - 2, D)).astype(np.float32)
        p[:, 0] = ((np.arange(R - 2) + 0.25) / (R - 2)).astype(np.float32)
        assert np.array_equal(np.floor(p[:, 0] * np.float32(R - 2) + np.float32(0.5)), np.arange(R - 2))
        parts.append(p)
    return np.concatenate(parts)


def _table(res, log2_rows, D, F, seed):
    offs, resl, emb = make_grid(res, log2_rows, D, F, seed=seed)
    emb[::7] = 0.0                            # sign(0) = +1
    emb[3::7] = -0.0
    return offs, resl, emb


def _fwd(dev, x, bits, offs, resl, D, F, pair, lut, monkeypatch, ld=0, col=0):
    from cnc_amd.backends import gridencoder_backend as be
    t = lambda a: torch.as_tensor(a, device=dev)
    N, L = x.shape[0], len(resl)
    monkeypatch.setenv("CNC_FWD_PAIR", str(pair))
    monkeypatch.setenv("CNC_FWD_LUT", str(lut))
    out = torch.full((N, ld) if ld else (L, N, F), 7.0, device=dev)
    be.grid_encode_forward_bits(t(x), bits, t(offs), t(resl), out, N, D, F, L, 128, None, None, None,
                                out_ld=ld, out_col=col)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("log2_rows", [3, 4, 6, 10])
def test_small_hashed_tables_every_cell(cuda, oracle, monkeypatch, D, log2_rows):
    from cnc_amd.backends import gridencoder_backend as be
    res = RES[log2_rows]
    offs, resl, emb = _table(res, log2_rows, D, 8, seed=300 + log2_rows + D)
    dense = [int(R) ** D <= 2 ** log2_rows for R in res]
    assert any(dense) and not all(dense)
    x = _cell_points(res, D, seed=11 * log2_rows + D)
    want = oracle.grid_encode_forward(x, emb, offs, resl, ste_binary=True)
    bits = be.pack_sign_bits(torch.as_tensor(emb, device=cuda))
    for lut in (0, 1):
        off = _fwd(cuda, x, bits, offs, resl, D, 8, 0, lut, monkeypatch)
        got = _fwd(cuda, x, bits, offs, resl, D, 8, 2, lut, monkeypatch)
        assert np.array_equal(got, want)
        assert np.array_equal(got, off)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("F", [1, 2, 4, 16, 32])
def test_other_feature_widths_keep_the_old_path(cuda, oracle, monkeypatch, D, F):
    from cnc_amd.backends import gridencoder_backend as be
    res = RES[6]
    offs, resl, emb = _table(res, 6, D, F, seed=400 + F)
    x = _cell_points(res, D, seed=F + D)
    want = oracle.grid_encode_forward(x, emb, offs, resl, ste_binary=True)
    bits = be.pack_sign_bits(torch.as_tensor(emb, device=cuda))
    assert np.array_equal(_fwd(cuda, x, bits, offs, resl, D, F, 2, 1, monkeypatch), want)
    assert np.array_equal(_fwd(cuda, x, bits, offs, resl, D, F, 0, 1, monkeypatch), want)


@pytest.mark.parametrize("shift", [1, 3, 4])
def test_misaligned_plane(cuda, oracle, monkeypatch, shift):
    """The plane as a view `shift` bytes into a larger buffer: the aligned words are not available, the byte gathers are."""
    from cnc_amd.backends import gridencoder_backend as be
    res = RES[10]
    offs, resl, emb = _table(res, 10, 3, 8, seed=500)
    x = _cell_points(res, 3, seed=5)
    want = oracle.grid_encode_forward(x, emb, offs, resl, ste_binary=True)
    bits = be.pack_sign_bits(torch.as_tensor(emb, device=cuda))
    assert bits.data_ptr() % 16 == 0
    big = torch.full((bits.numel() + 64,), 0xA5, dtype=torch.uint8, device=cuda)
    view = big[shift:shift + bits.numel()]
    view.copy_(bits)
    assert view.data_ptr() % 8 == shift
    for lut in (0, 1):
        assert np.array_equal(_fwd(cuda, x, view, offs, resl, 3, 8, 2, lut, monkeypatch), want)
        assert np.array_equal(_fwd(cuda, x, view, offs, resl, 3, 8, 0, lut, monkeypatch), want)


@pytest.mark.parametrize("N", [1, 63, 65, 257])
@pytest.mark.parametrize("D", [2, 3])
def test_ragged_and_point_major(cuda, oracle, monkeypatch, N, D):
    """Ragged point counts in both layouts; point-major rows inside a wider matrix, the neighbours' columns untouched."""
    from cnc_amd.backends import gridencoder_backend as be
    res = RES[10]
    L, F = len(res), 8
    offs, resl, emb = _table(res, 10, D, F, seed=600 + N)
    # the last N points: cells of the finest level, g % 8 == 7 among them from N = 63 up
    x = _cell_points(res, D, seed=N)[-N:]
    want = oracle.grid_encode_forward(x, emb, offs, resl, ste_binary=True)      # [L, N, F]
    bits = be.pack_sign_bits(torch.as_tensor(emb, device=cuda))
    assert np.array_equal(_fwd(cuda, x, bits, offs, resl, D, F, 2, 1, monkeypatch), want)
    assert np.array_equal(_fwd(cuda, x, bits, offs, resl, D, F, 0, 1, monkeypatch), want)
    ld, col = L * F + 12, 4
    for pair in (2, 0):
        got = _fwd(cuda, x, bits, offs, resl, D, F, pair, 1, monkeypatch, ld=ld, col=col)
        assert np.array_equal(got[:, col:col + L * F].reshape(N, L, F).transpose(1, 0, 2), want)
        assert np.all(got[:, :col] == 7.0) and np.all(got[:, col + L * F:] == 7.0)


def test_default_policy(cuda, oracle, monkeypatch):
    """CNC_FWD_PAIR=1 (and the switch unset): hashed levels below, at both ends of and above the policy's window of
    resolutions (kFwdPairMinRes = 80 <= R < kFwdPairMaxRes = 660 in grid_encode.hip), 2^10 rows, N = 4,097."""
    from cnc_amd.backends import gridencoder_backend as be
    res = [4, 10, 11, 40, 79, 80, 200, 659, 660, 700]
    offs, resl, emb = _table(res, 10, 3, 8, seed=700)
    x = np.concatenate([_cell_points(res, 3, seed=7), _points(4097, 3, seed=8)])[:4097]
    assert x.shape[0] == 4097
    want = oracle.grid_encode_forward(x, emb, offs, resl, ste_binary=True)
    bits = be.pack_sign_bits(torch.as_tensor(emb, device=cuda))
    off = _fwd(cuda, x, bits, offs, resl, 3, 8, 0, 1, monkeypatch)
    assert np.array_equal(off, want)
    assert np.array_equal(_fwd(cuda, x, bits, offs, resl, 3, 8, 1, 1, monkeypatch), off)
    monkeypatch.delenv("CNC_FWD_PAIR")
    t = lambda a: torch.as_tensor(a, device=cuda)
    out = torch.empty((len(res), 4097, 8), device=cuda)
    be.grid_encode_forward_bits(t(x), bits, t(offs), t(resl), out, 4097, 3, 8, len(res), 128)
    assert np.array_equal(out.cpu().numpy(), off)


def test_bench_table(cuda, oracle, monkeypatch):
    """bench.py's table (16L x 2^19 x F8) and the first 2^16 samples of its marched probe chunk: every mode gives the
    oracle's and the fp32 STE gather's answer, bit for bit."""
    sys.path.insert(0, ROOT)
    import bench
    from cnc_amd.backends import gridencoder_backend as be
    w = bench.build_workload(cuda, 0)
    box = {}
    bench.march_frame(w, box)
    x = bench.probe_chunk_of(box["ex"]["positions"])[: 1 << 16].contiguous()
    N, F, L, D = x.shape[0], bench.F, bench.L, bench.D
    assert N == 1 << 16 and L == 16 and F == 8
    be.pack_sign_bits(w["table"], w["bits"], w["clip"])
    out = torch.empty((L, N, F), device=cuda)
    got = []
    for pair in ("0", "1", "2"):
        monkeypatch.setenv("CNC_FWD_PAIR", pair)
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
