"""The occupancy grid's "pyramid1" coder on the GPU (cnc_amd/csrc/occ_pyramid.hip, cnc_amd/occupancy_codec.py, DESIGN
§4.9) against its NumPy twin (tests/occ_pyramid_twin.py): every integer the kernels produce is EQUAL to the twin's, the
round trip gives the grid back bit for bit under both coders, and the payload's size is held to the twin's ideal code
length.  Kernel outputs sit inside sentinel-filled allocations (tests/guarded.py)."""
import functools
import os

import numpy as np
import pytest
import torch

import occ_pyramid_twin as twin
from guarded import Guarded

pytestmark = pytest.mark.gpu

# The proportional excess of the device coder's streams over the host range coder's for the same symbols, once the
# derivable part (6 bytes per stream, 4 + dir_width per lane) is taken off, at the default 16384 symbols per lane.  Measured
# on the two 128^3 grids below (profiles/occ_pyramid.md): -0.6 % ... -100 % on the ball's four streams, -0.2 % ... -1.5 % on
# the blobs and rods' — never positive, because a lane's 32-bit state, counted in the derivable part, carries what the
# range coder spends on its last bytes.  Twice a measured excess of nothing is nothing: the device stream may exceed the
# host stream by the derivable part alone.
RANS_EXCESS = 0.0


def _corners(res):
    g = np.zeros((1, res, res, res), np.uint8)
    for x in (0, res - 1):
        for y in (0, res - 1):
            for z in (0, res - 1):
                g[0, x, y, z] = 1
    return g


def _rand(shape, p, seed):
    return (np.random.default_rng(seed).uniform(size=shape) < p).astype(np.uint8)


def _two_grids():
    g = np.zeros((2, 32, 32, 32), np.uint8)
    g[1] = twin.ball(32, radius=0.7)[0]
    g[1, 0, 31, 5] = 1
    return g


GRIDS = {
    "16": lambda: _rand((1, 16, 16, 16), 0.1, 1),
    "18_K1": lambda: _rand((1, 18, 18, 18), 0.15, 2),
    "32x48x16": lambda: _rand((1, 32, 48, 16), 0.05, 3),
    "two_grids_one_empty": _two_grids,
    "ball128": lambda: twin.ball(128),
    "blobs_rods128": lambda: twin.blobs_and_rods(128, seed=11),
    "zeros": lambda: np.zeros((1, 32, 32, 32), np.uint8),
    "ones": lambda: np.ones((1, 32, 32, 32), np.uint8),
    "corners": lambda: _corners(32),
    "half32": lambda: _rand((1, 32, 32, 32), 0.5, 4),
    # occ_scan_kernel: one workgroup scans 1024 block counts (262144 parents) per trip and carries the total into the
    # next.  128^3 has exactly 262144 level-1 parents — one trip; five 80^3 grids have 320000 — two trips
    "five_80": lambda: _rand((5, 80, 80, 80), 0.05, 5),
}
BIG = ("ball128", "blobs_rods128")


@functools.lru_cache(maxsize=None)
def _case(name):
    g = GRIDS[name]()
    g.setflags(write=False)
    return g, twin.model(g)


def _dir_width(n, lanes):
    worst = 2 * ((n + lanes - 1) // lanes)
    return 1 if worst < 1 << 8 else 2 if worst < 1 << 16 else 3 if worst < 1 << 24 else 4


def _rans_fixed_bytes(n, S):
    """rans1's derivable part for a stream of n symbols: header, and per lane its state and directory entry."""
    lanes = (n + S - 1) // S
    return 6 + lanes * (4 + _dir_width(n, lanes))


@pytest.mark.parametrize("name", list(GRIDS))
def test_kernels_equal_the_twin(cuda, name):
    from cnc_amd.backends import occ_pyramid as B
    g, m = _case(name)
    K = m["K"]
    assert K == {"16": 4, "18_K1": 1, "32x48x16": 4}.get(name, 4)
    grid = Guarded(g, cuda)
    n_coarse = sum(lv.size for lv in m["levels"][1:])
    coarse = Guarded.empty((n_coarse,), np.uint8, cuda)
    B.reduce(grid.tensor(), K, coarse.tensor())
    got, at = coarse.get(), 0
    levels = [grid.tensor()]
    for k in range(1, K + 1):
        lv = m["levels"][k]
        assert np.array_equal(got[at:at + lv.size].reshape(lv.shape), lv), f"level {k}"
        levels.append(coarse.tensor()[at:at + lv.size].view(lv.shape))
        at += lv.size
    assert coarse.intact() and grid.intact()
    for k in range(K - 1, -1, -1):
        want = m["per"][k]
        n = want["n"]
        words = B.rank_scratch_words(levels[k + 1].numel())
        assert words == (levels[k + 1].numel() + 255) // 256 + 1
        scratch = Guarded.empty((words,), np.int32, cuda)
        B.rank(levels[k + 1], scratch.tensor())
        s = scratch.get()
        flat = m["levels"][k + 1].reshape(-1)
        per_block = np.add.reduceat(flat.astype(np.int64), np.arange(0, flat.size, 256))
        assert s[-1] * 8 == n and np.array_equal(s[:-1], np.cumsum(per_block) - per_block)
        idx, ctx = Guarded.empty((n,), np.int32, cuda), Guarded.empty((n,), np.uint8, cuda)
        sym, hist = Guarded.empty((n,), np.float32, cuda), Guarded(np.zeros((32, 2), np.int32), cuda)
        B.emit(levels[k + 1], scratch.tensor(), n, ctx.tensor(), idx=idx.tensor(), child=levels[k], sym=sym.tensor(),
               hist=hist.tensor())
        assert np.array_equal(idx.get(), want["idx"]) and np.array_equal(ctx.get(), want["ctx"])
        assert np.array_equal(sym.get(), want["sym"]) and np.array_equal(hist.get(), want["hist"])
        # the decode's form of the same call: no child, no symbols, no histogram
        idx2, ctx2 = Guarded.empty((n,), np.int32, cuda), Guarded.empty((n,), np.uint8, cuda)
        B.emit(levels[k + 1], scratch.tensor(), n, ctx2.tensor(), idx=idx2.tensor())
        assert np.array_equal(idx2.get(), want["idx"]) and np.array_equal(ctx2.get(), want["ctx"])
        table = twin.p_of_c1(want["c1"])
        p = Guarded.empty((n,), np.float32, cuda)
        B.probs(ctx.tensor(), torch.from_numpy(table).to(cuda), p.tensor())
        assert np.array_equal(p.get(), table[want["ctx"]])
        child = Guarded(np.zeros(m["levels"][k].shape, np.uint8), cuda)
        status = Guarded(np.zeros(1, np.int32), cuda)
        if n:
            B.scatter(sym.tensor(), idx.tensor(), scratch.tensor(), levels[k + 1].numel(), child.tensor(), status.tensor())
        assert np.array_equal(child.get(), m["levels"][k]) and status.get()[0] == 0
        for buf in (scratch, idx, ctx, sym, hist, idx2, ctx2, p, child, status):
            assert buf.intact()


@pytest.mark.parametrize("name", list(GRIDS))
def test_round_trip_sizes_and_cross_decode(cuda, name, tmp_path):
    from cnc_amd import occupancy_codec as oc
    from cnc_amd.context import DEVICE_CODER_SYMBOLS_PER_LANE as S, decoder
    g, m = _case(name)
    K = m["K"]
    dev_grid = torch.from_numpy(g.copy()).to(cuda).bool()
    out = {}
    for coder in ("host", "device"):
        payload, info = oc.encode_occupancy(dev_grid, coder=coder)
        again, info2 = oc.encode_occupancy(dev_grid, coder=coder)
        assert payload == again and info == info2                          # the bytes depend on the grid alone
        assert info["model"] == "pyramid1" and info["shape"] == list(g.shape) and info["levels"] == K
        assert info["n"] == [lv["n"] for lv in m["per"]]
        assert np.array_equal(np.array(info["c1"]), np.stack([lv["c1"] for lv in m["per"]]))
        assert info["coder"] == ("rans1" if coder == "device" else "range")
        back = oc.decode_occupancy(payload, info, cuda)
        assert back.dtype == torch.bool and torch.equal(back, dev_grid)
        header = {k: v for k, v in info.items() if k != "c1"}              # what the container keeps: the payload has the tables
        assert torch.equal(oc.decode_occupancy(payload, header, cuda, coder=coder), dev_grid)
        out[coder] = (payload, info)
    payload, info = out["host"]
    # cross decode: the GPU path's host-coder payload through the twin and the host decoder
    top, c1, streams = twin.split_payload(payload, g.shape, info["n"], info["stream_sizes"])
    assert payload[:len(m["raw"])] == m["raw"]

    def decode_stream(k, p):
        f = str(tmp_path / f"x{k}.b")
        with open(f, "wb") as fo:
            fo.write(streams[k])
        return decoder(torch.from_numpy(p), f).numpy()
    assert np.array_equal(twin.decode(top, c1, info["n"], decode_stream), g)
    # size, host coder: raw + tables + per stream 1.002 x ideal + 64 bits (the range coder's bound)
    fixed = len(m["raw"]) + K * 64
    bound = fixed + sum((lv["ideal_bits"] * 1.002 + 64) / 8 for lv in m["per"] if lv["n"])
    print(f"{name}: host payload {len(payload)} B, bound {bound:.1f} B, ideal {sum(lv['ideal_bits'] for lv in m['per']) / 8:.1f} B")
    assert len(payload) <= bound
    assert sum(info["stream_sizes"]) == len(payload) - fixed
    # size, device coder: against the host coder's bytes for the same streams
    dpayload, dinfo = out["device"]
    for k in range(K):
        n, hs, ds = info["n"][k], info["stream_sizes"][k], dinfo["stream_sizes"][k]
        if n == 0:
            assert hs == ds == 0
            continue
        derivable = _rans_fixed_bytes(n, S)
        print(f"{name} level {k}: n {n}, host {hs} B, device {ds} B, derivable {derivable} B, "
              f"excess {(ds - derivable - hs) / hs:+.5f}")
        assert ds <= hs + derivable + 2 * RANS_EXCESS * hs, (k, n, hs, ds)


@pytest.mark.parametrize("name", BIG)
def test_a_fifth_of_todays_section(cuda, name, tmp_path):
    """Against the section write_container produces today (one Bernoulli frequency), same grid, same test."""
    from cnc_amd import occupancy_codec as oc
    from cnc_amd.container import section_sizes, write_container
    g, _ = _case(name)
    dev_grid = torch.from_numpy(g.copy()).to(cuda).bool()
    f = str(tmp_path / "iid.cnc")
    write_container(f, meta={}, table_streams={}, binaries=dev_grid, field_mlp={}, context_state={})
    iid = section_sizes(f)["occupancy"]
    for coder in ("host", "device"):
        payload, _ = oc.encode_occupancy(dev_grid, coder=coder)
        print(f"{name}: iid {iid} B, pyramid ({coder}) {len(payload)} B")
        assert 5 * len(payload) <= iid


@pytest.mark.parametrize("coder", ["host", "device"])
def test_damaged_header_and_stream(cuda, coder):
    """A header whose n_k is off by 8 in either direction raises; so does a payload shorter than the header says, and with
    the device coder a stream cut short with the header adjusted to it (cnc_rans_check, as for the tables' streams)."""
    from cnc_amd import occupancy_codec as oc
    g, m = _case("blobs_rods128")
    dev_grid = torch.from_numpy(g.copy()).to(cuda).bool()
    payload, info = oc.encode_occupancy(dev_grid, coder=coder)
    for k in (0, 2):
        for d in (8, -8):
            bad = dict(info, n=[v + (d if j == k else 0) for j, v in enumerate(info["n"])])
            with pytest.raises(RuntimeError):
                oc.decode_occupancy(payload, bad, cuda)
    with pytest.raises(RuntimeError):
        oc.decode_occupancy(payload[:-3], info, cuda)
    if coder == "device":
        cut = dict(info, stream_sizes=[info["stream_sizes"][0] - 3] + info["stream_sizes"][1:])
        with pytest.raises(RuntimeError):
            oc.decode_occupancy(payload[:-3], cut, cuda)
    assert torch.equal(oc.decode_occupancy(payload, info, cuda), dev_grid)          # and the device is as it was


@pytest.mark.parametrize("delta", [8, -8])
def test_wrong_count_stays_inside_the_buffers(cuda, delta):
    """The kernels under a header count that is not 8 x the occupied parents: buffers of the HEADER's size inside
    sentinels, the rank raises the status word, emit and scatter clamp to the smaller count, every guard word intact."""
    from cnc_amd._lib import CNC_OCC_STATUS_COUNT
    from cnc_amd.backends import occ_pyramid as B
    g, m = _case("32x48x16")
    k = 0
    want, parent_np = m["per"][k], m["levels"][k + 1]
    n = want["n"] + delta
    keep = min(n, want["n"])
    parent = Guarded(parent_np, cuda)
    scratch = Guarded.empty((B.rank_scratch_words(parent_np.size),), np.int32, cuda)
    status = Guarded(np.zeros(1, np.int32), cuda)
    B.rank(parent.tensor(), scratch.tensor(), n_expected=n, status=status.tensor())
    idx, ctx = Guarded(np.zeros(n, np.int32), cuda), Guarded(np.zeros(n, np.uint8), cuda)
    B.emit(parent.tensor(), scratch.tensor(), n, ctx.tensor(), idx=idx.tensor())
    assert np.array_equal(idx.get()[:keep], want["idx"][:keep]) and np.array_equal(ctx.get()[:keep], want["ctx"][:keep])
    assert (idx.get()[keep:] == 0).all() and (ctx.get()[keep:] == 0).all()
    sym = Guarded(np.ones(n, np.float32), cuda)
    child = Guarded(np.zeros(m["levels"][k].shape, np.uint8), cuda)
    B.scatter(sym.tensor(), idx.tensor(), scratch.tensor(), parent_np.size, child.tensor(), status.tensor())
    expect = np.zeros(m["levels"][k].size, np.uint8)
    expect[want["idx"][:keep]] = 1
    assert np.array_equal(child.get().reshape(-1), expect)
    assert status.get()[0] == CNC_OCC_STATUS_COUNT
    for buf in (parent, scratch, status, idx, ctx, sym, child):
        assert buf.intact()


# occ_scan_kernel's trips: kScanThreads = 1024 counts of 256 parents each.  262144 parents: the last size of one trip;
# + 1: a second trip of one count (one parent in it); 2 * 262144 + 77: three trips, the last count a partial block
@pytest.mark.parametrize("n_parents", [262144, 262145, 2 * 262144 + 77])
def test_rank_scan_carries_between_its_chunks(cuda, n_parents):
    """cnc_occ_rank on random parent bytes: the scratch equals NumPy's exclusive cumulative sum of the per-256 counts with
    the total behind it — integers, so equal or not; the status word stays 0 for the right n_expected and takes
    CNC_OCC_STATUS_COUNT for one that is 8 off either way.  On the MI355X: 0 of 1025, 1026 and 2050 words differ."""
    from cnc_amd._lib import CNC_OCC_STATUS_COUNT
    from cnc_amd.backends import occ_pyramid as B
    rng = np.random.default_rng(n_parents)
    host = (rng.uniform(size=n_parents) < 0.3).astype(np.uint8) * rng.integers(1, 256, n_parents).astype(np.uint8)
    host[-1] = 1                                                  # the last trip's last count is not zero
    per_block = np.add.reduceat((host != 0).astype(np.int64), np.arange(0, n_parents, 256))
    want = np.concatenate([np.cumsum(per_block) - per_block, [per_block.sum()]]).astype(np.int32)
    assert want.size == (n_parents + 255) // 256 + 1 == B.rank_scratch_words(n_parents)
    assert (want.size - 1 > 1024) == (n_parents > 262144) and per_block[:1024].sum() > 0
    parent = Guarded(host.reshape(1, 1, 1, n_parents), cuda)
    total = int(want[-1])
    for n_expected, flag in ((-1, 0), (8 * total, 0), (8 * total + 8, CNC_OCC_STATUS_COUNT), (8 * total - 8, CNC_OCC_STATUS_COUNT)):
        scratch = Guarded.empty((want.size,), np.int32, cuda)
        status = Guarded(np.zeros(1, np.int32), cuda)
        B.rank(parent.tensor(), scratch.tensor(), n_expected=n_expected, status=status.tensor())
        got = scratch.get()
        wrong = np.flatnonzero(got != want)
        print(f"occ rank n_parents={n_parents} n_expected={n_expected}: {wrong.size} of {want.size} words differ")
        assert wrong.size == 0, (int(wrong[0]), int(got[wrong[0]]), int(want[wrong[0]]))
        assert status.get()[0] == flag
        assert scratch.intact() and status.intact() and parent.intact()


def test_container_and_trainer(cuda, tmp_path):
    """A small Trainer's container with the pyramid section loads into a fresh Trainer: same occupancy grid, same tables
    on coded rows; without the flag the file is what it was — the iid section, no `model` key, the same bytes."""
    import json
    import struct
    from cnc_amd.container import read_container, section_sizes, write_container
    from cnc_amd.context import encoder
    from cnc_amd.trainer import Trainer
    from test_gpu_trainer import _cfg
    a = Trainer(_cfg(tmp_path), device=cuda)
    a.train(steps=12, log=None)
    assert a.occupancy_coder_name() == "iid"
    plain = a.save_container(str(tmp_path / "plain.cnc"))
    assert "occupancy_KB" not in plain
    a.cfg.occupancy_coder = "pyramid"
    info = a.save_container(str(tmp_path / "pyr.cnc"))
    assert info["occupancy_KB"] * 1024 == section_sizes(str(tmp_path / "pyr.cnc"))["occupancy"]

    def header(path):
        raw = open(path, "rb").read()
        (hlen,) = struct.unpack("<I", raw[4:8])
        return json.loads(raw[8:8 + hlen]), raw[8 + hlen:]
    hp, _ = header(str(tmp_path / "pyr.cnc"))
    sec = hp["sections"]["occupancy"]
    assert sec["model"] == "pyramid1" and sec["shape"] == list(a.estimator.binaries.shape) and "pg" not in sec
    e = a.field.mlp_base
    tabs = (lambda t: (t.encoding_xyz, t.encoding_xy, t.encoding_xz, t.encoding_yz))
    orig = [torch.where(t.params.data >= 0, 1.0, -1.0) for t in tabs(e)]
    b = Trainer(_cfg(tmp_path, seed=7), device=cuda)
    b.load_container(str(tmp_path / "pyr.cnc"))                       # no flag: the file says what it is
    assert torch.equal(b.estimator.binaries, a.estimator.binaries) and b.estimator.binaries.dtype == a.estimator.binaries.dtype
    for t, o in zip(tabs(b.field.mlp_base), orig):
        dec = t.params.data
        uncoded = (dec == 1).all(dim=1)
        assert torch.all(dec.abs() == 1) and torch.equal(dec[~uncoded], o[~uncoded])
    with pytest.raises(RuntimeError):
        read_container(str(tmp_path / "pyr.cnc"), device="cpu")       # the product has no CPU path
    # without the flag: the parent's section, rebuilt here the way the parent built it
    h0, blob = header(str(tmp_path / "plain.cnc"))
    s0 = h0["sections"]["occupancy"]
    assert "model" not in s0 and sorted(s0) == ["offset", "pg", "shape", "size"]
    occ = a.estimator.binaries.reshape(-1).to(torch.float32).cpu()
    pg = float(occ.mean().clamp(1e-6, 1 - 1e-6))
    encoder(occ * 2 - 1, torch.full_like(occ, pg), str(tmp_path / "occ.b"))
    assert s0["pg"] == pg and blob[s0["offset"]:s0["offset"] + s0["size"]] == open(tmp_path / "occ.b", "rb").read()
    kw = dict(meta={"x": 1}, table_streams={"t": b"abc"}, binaries=a.estimator.binaries, field_mlp=a._mlp_state(),
              context_state=a.context.state_dict())
    write_container(str(tmp_path / "d.cnc"), **kw)
    write_container(str(tmp_path / "i.cnc"), occupancy_coder="iid", coder="device", **kw)
    assert open(tmp_path / "d.cnc", "rb").read() == open(tmp_path / "i.cnc", "rb").read()
    # the switch through the environment
    os.environ["CNC_OCC_CODER"] = "pyramid"
    try:
        assert Trainer.occupancy_coder_name(b) == "pyramid"
    finally:
        del os.environ["CNC_OCC_CODER"]
