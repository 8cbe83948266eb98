"""CPU-only: the "tree1" MLP section's NumPy twin (tests/mlp_tree_twin.py) round-trips, alone and through the host range
coder, and the product's host helpers (cnc_amd/mlp_codec.py) equal it on seeded inputs; payloads and headers that do not
fit raise RuntimeError, and the switch refuses what DESIGN §4.12 says it refuses."""
import functools

import numpy as np
import pytest
import torch

import mlp_tree_twin as twin

SIZES = (1, 7, 8, 9, 63, 64, 65, 160, 257)


def _indices(kind, n, bits, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.integers(0, 2 ** bits, size=n).astype(np.int64)
    if kind == "laplace":
        return twin.laplace_indices(n, bits, seed)
    if kind == "constant":
        return np.full(n, (2 ** bits) // 3, np.int64)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _mixed(bits):
    qs = [_indices(("laplace", "uniform", "constant")[k % 3], n, bits, 10 * bits + k) for k, n in enumerate(SIZES)]
    qs.append(_indices("laplace", 4096, bits, 99))
    for q in qs:
        q.setflags(write=False)
    return qs


def _header(m, coder="range", sizes=None):
    return dict(model="tree1", coder=coder, bits=m["bits"],
                tensors=[dict(name=f"t{k}", shape=[n], lo=-1.0, interval=0.25, depth=d)
                         for k, (n, d) in enumerate(zip(m["counts"], m["depths"]))],
                stream_sizes=list(sizes if sizes is not None else [pl["n"] for pl in m["planes"]]))


@pytest.mark.parametrize("bits", [8, 13, 16])
def test_twin_round_trips(bits):
    qs = _mixed(bits)
    for depths in (None, [k % 9 for k in range(len(qs))], [8] * len(qs), [0] * (len(qs) - 1) + [3]):
        m = twin.model(qs, bits, depths)
        back = twin.decode(m["c1"], m["low"], m["counts"], m["depths"], bits, lambda j, p: m["planes"][j]["sym"])
        assert all(np.array_equal(a, b) for a, b in zip(back, qs))
        for q, d, b in zip(qs, m["depths"], m["low"]):
            assert len(b) == twin.low_len(q.size, bits - d)
            assert np.array_equal(twin.unpack_low(b, q.size, bits - d), q & ((1 << (bits - d)) - 1))
        # the fake streams (one byte per symbol) through the payload's two directions
        streams = [pl["sym"].astype(np.int8).tobytes() for pl in m["planes"]]
        c1, low, st = twin.split_payload(twin.join_payload(m["c1"], m["low"], streams), m["counts"], m["depths"], bits,
                                         [len(s) for s in streams])
        assert st == streams and low == m["low"] and all(np.array_equal(a, b) for a, b in zip(c1, m["c1"]))


def test_low_bits_are_the_containers_bit_order():
    from cnc_amd.container import _pack_bits
    q = _indices("uniform", 257, 16, 5)
    for r in range(1, 17):
        v = q & ((1 << r) - 1)
        assert twin.pack_low(q, r) == _pack_bits(v.astype(np.uint32), r)


def test_depth_choice_of_known_inputs():
    assert twin.choose_depth(_indices("uniform", 160, 13, 1), 13) == 0          # a bias: the tables cost more than they save
    assert twin.choose_depth(_indices("uniform", 160 * 255, 13, 2), 13) == 0    # a freshly initialised layer
    assert twin.choose_depth(_indices("laplace", 160 * 255, 13, 3), 13) >= 4
    assert twin.choose_depth(_indices("constant", 4096, 13, 4), 13) == 8


def test_planes_round_trip_through_the_host_coder(tmp_path):
    from cnc_amd.context import decoder, encoder
    bits = 13
    qs = _mixed(bits)
    m = twin.model(qs, bits)
    assert m["D"] >= 1
    files = []
    for j, pl in enumerate(m["planes"]):
        files.append(str(tmp_path / f"p{j}.b"))
        encoder(torch.from_numpy(pl["sym"]), torch.from_numpy(pl["p"]), files[j])

    def decode_stream(j, p):
        assert np.array_equal(p, m["planes"][j]["p"])
        return decoder(torch.from_numpy(p), files[j]).numpy()
    back = twin.decode(m["c1"], m["low"], m["counts"], m["depths"], bits, decode_stream)
    assert all(np.array_equal(a, b) for a, b in zip(back, qs))


@pytest.mark.parametrize("bits", [8, 13, 16])
def test_host_helpers_equal_the_twin(bits):
    from cnc_amd import mlp_codec as mc
    assert mc.MODEL == "tree1"
    qs = _mixed(bits)
    m = twin.model(qs, bits)
    for q, d, tab, h in zip(qs, m["depths"], m["c1"], m["hist"]):
        assert np.array_equal(np.bincount(q >> (bits - 8), minlength=256), h)
        assert mc.choose_depth(h, q.size, bits) == d
        assert mc.depth_costs(h, q.size, bits) == twin.depth_costs(q, bits)
        for depth in range(9):
            assert np.array_equal(mc.tables_of_hist(h, depth), twin.tables(q, bits, depth))
        assert np.array_equal(mc.tables_of_hist(h, d), tab)
    for depths in (m["depths"], [k % 9 for k in range(len(qs))]):
        f = twin.model(qs, bits, depths)
        lay = mc.layout(f["counts"], depths, bits)
        assert lay["plane_n"][:f["D"]] == [pl["n"] for pl in f["planes"]] and not any(lay["plane_n"][f["D"]:])
        assert np.array_equal(lay["desc"][:, 8:], np.array(twin.plane_positions(f["counts"], depths)))
        assert lay["n_tab"] == sum(t.size for t in f["c1"]) and lay["n_low"] == sum(len(b) for b in f["low"])
        streams = [bytes([j + 1]) * (5 + j) for j in range(f["D"])]
        payload = mc.join_payload(f["c1"], b"".join(f["low"]), streams)
        assert payload == twin.join_payload(f["c1"], f["low"], streams)
        c1, low, st = mc.split_payload(payload, _header(f, sizes=[len(s) for s in streams]))
        assert st == streams and low == b"".join(f["low"]) and all(np.array_equal(a, b) for a, b in zip(c1, f["c1"]))


def test_misfit_payloads_and_headers_raise():
    from cnc_amd import mlp_codec as mc
    bits = 13
    m = twin.model(_mixed(bits), bits)
    streams = [b"\x01" * 9 for _ in range(m["D"])]
    payload = twin.join_payload(m["c1"], m["low"], streams)
    good = _header(m, sizes=[9] * m["D"])
    mc.split_payload(payload, good)
    for bad_payload in (payload[:-1], payload + b"\x00", b""):
        with pytest.raises(RuntimeError):
            mc.split_payload(bad_payload, good)

    def tensor0(**kw):
        return dict(good, tensors=[dict(good["tensors"][0], **kw)] + good["tensors"][1:])
    bad_headers = [
        dict(good, model="tree2"), dict(good, coder="huffman"), dict(good, bits=7), dict(good, bits=17), dict(good, bits="13"),
        dict(good, stream_sizes=good["stream_sizes"][:-1]), dict(good, stream_sizes=good["stream_sizes"] + [4]),
        dict(good, stream_sizes=[0] + good["stream_sizes"][1:]), dict(good, tensors=[]),
        tensor0(depth=9), tensor0(depth=-1), tensor0(depth=2.0), tensor0(shape=[0]), tensor0(shape=[-3, 2]),
        tensor0(name=good["tensors"][1]["name"]), tensor0(lo=float("nan")), tensor0(shape=[2 ** 31]), tensor0(shape=[2 ** 40, 2 ** 40]),
        {k: v for k, v in good.items() if k != "tensors"}, {k: v for k, v in good.items() if k != "bits"},
    ]
    for bad in bad_headers:
        with pytest.raises(RuntimeError):
            mc.split_payload(payload, bad)
    zero = bytearray(payload)
    k = next(i for i, t in enumerate(m["c1"]) if t.size)
    at = 2 * sum(t.size for t in m["c1"][:k])
    zero[at:at + 2] = b"\x00\x00"
    with pytest.raises(RuntimeError, match="zero probability"):
        mc.split_payload(bytes(zero), good)
    with pytest.raises(RuntimeError):
        mc.decode_mlp(payload, good, "cpu")                      # the product has no CPU path


def _container_kw():
    g = torch.Generator().manual_seed(3)
    return dict(meta={"x": 1}, table_streams={"t": b"abc"}, binaries=torch.rand(1, 6, 6, 6, generator=g) < 0.3,
                field_mlp={"w": torch.randn(16, 9, generator=g), "b": torch.randn(16, generator=g)},
                context_state={"c": torch.randn(4, 3, generator=g)})


def test_refusals(tmp_path):
    from cnc_amd import mlp_codec as mc
    from cnc_amd.container import write_container
    from cnc_amd.trainer import TrainConfig, Trainer
    kw = _container_kw()
    f = str(tmp_path / "a.cnc")
    with pytest.raises(ValueError, match="mlp_coder"):
        write_container(f, mlp_coder="huffman", **kw)
    for bits in (7, 17):
        with pytest.raises(ValueError, match="bits"):
            write_container(f, mlp_coder="tree", mlp_bits=bits, **kw)
        with pytest.raises(ValueError, match="bits"):
            mc.encode_mlp(kw["field_mlp"], bits=bits)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        write_container(f, mlp_coder="tree", **kw)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        mc.encode_mlp(kw["field_mlp"])
    with pytest.raises(ValueError, match="coder"):
        mc.encode_mlp(kw["field_mlp"], coder="huffman")
    assert TrainConfig().mlp_coder == "packed"

    class _T:
        cfg = TrainConfig(mlp_coder="zip")
    with pytest.raises(ValueError, match="mlp coder"):
        Trainer.mlp_coder_name(_T())
    _T.cfg = TrainConfig(mlp_coder="tree")
    assert Trainer.mlp_coder_name(_T()) == "tree"
    _T.cfg = TrainConfig()
    assert Trainer.mlp_coder_name(_T()) == "packed"


def test_env_and_flag(monkeypatch):
    from cnc_amd.train import build_parser
    from cnc_amd.trainer import TrainConfig, Trainer

    class _T:
        cfg = TrainConfig()
    monkeypatch.setenv("CNC_MLP_CODER", "tree")
    assert Trainer.mlp_coder_name(_T()) == "tree"
    monkeypatch.setenv("CNC_MLP_CODER", "lzma")
    with pytest.raises(ValueError):
        Trainer.mlp_coder_name(_T())
    ap = build_parser()
    assert ap.parse_args([]).mlp_coder == "packed" and ap.parse_args(["--mlp-coder", "tree"]).mlp_coder == "tree"
    with pytest.raises(SystemExit):
        ap.parse_args(["--mlp-coder", "zip"])


def test_packed_writes_todays_bytes(tmp_path):
    from cnc_amd.container import read_container, write_container
    kw = _container_kw()
    a, b = str(tmp_path / "a.cnc"), str(tmp_path / "b.cnc")
    write_container(a, **kw)
    write_container(b, mlp_coder="packed", **kw)
    assert open(a, "rb").read() == open(b, "rb").read()
    _, _, _, mlp, _ = read_container(a)
    assert sorted(mlp) == ["b", "w"]
