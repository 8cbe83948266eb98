"""CPU-only: the coders' common call shape (cnc_amd/coders.py) on the host coder, the factory, and the names
cnc_amd.context re-exports."""
import os

import pytest
import torch


def test_host_coder_through_the_common_interface(tmp_path):
    """`make_coder("host")` on CPU tensors: encode / finish / decode_group / check give `encoder`'s bytes, their size
    in bits and the symbols back in order — a single symbol, a level coded with one frequency (an expanded scalar p)
    and a stream long enough for the range coder to renormalise many times."""
    from cnc_amd import coders
    gen = torch.Generator().manual_seed(12)
    ps = [torch.rand(1, generator=gen).clamp(1e-6, 1 - 1e-6),
          torch.tensor(0.3).reshape(1).expand(63),
          torch.rand(4097, generator=gen).clamp(1e-6, 1 - 1e-6)]
    xs = [torch.where(torch.rand(p.shape, generator=gen) < p, 1.0, -1.0) for p in ps]
    assert ps[1].stride(0) == 0 and [x.numel() for x in xs] == [1, 63, 4097]
    files = [str(tmp_path / f"s{k}.b") for k in range(3)]
    refs = [str(tmp_path / f"r{k}.b") for k in range(3)]
    pool = coders.make_coder("host")
    assert isinstance(pool, coders.CoderPool)
    for x, p, f, r in zip(xs, ps, files, refs):
        pool.encode(x, p, f)
        coders.encoder(x, p, r)
    bits = pool.finish()
    for f, r in zip(files, refs):
        assert open(f, "rb").read() == open(r, "rb").read()
    assert bits == 8 * sum(os.path.getsize(f) for f in files) > 0
    assert pool.finish() == 0                                  # nothing handed over since
    back = pool.decode_group((p, f) for p, f in zip(ps, files))          # any iterable, taken one by one
    assert len(back) == 3
    for got, x in zip(back, xs):
        assert got.dtype == torch.float32 and got.device == x.device and torch.equal(got, x)
    assert pool.check() is None
    pool.shutdown()


def test_make_coder_refuses_an_unknown_kind():
    from cnc_amd import coders
    with pytest.raises(ValueError, match="coder must be 'host' or 'device'"):
        coders.make_coder("gpu")


def test_context_re_exports_the_coders():
    from cnc_amd import coders, context
    for name in ("encoder", "decoder", "CoderPool", "DeviceCoder", "DEVICE_CODER_SYMBOLS_PER_LANE"):
        assert getattr(context, name) is getattr(coders, name), name
