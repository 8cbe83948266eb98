"""Host tests of the occupancy grid's "pyramid1" model: the NumPy twin pinned on grids small enough to check
by hand, the probability the coders are handed against their own quantiser, the package's host helpers against the twin,
and a round trip through the host range coder.  No GPU."""
import os

import numpy as np
import pytest
import torch

import occ_pyramid_twin as twin
from cnc_amd import occupancy_codec as oc


def test_single_corner_cell_by_hand():
    """Cell (0, 0, 0) of a 16^3 grid: K = 4, one occupied cell per level, every level's candidates are the eight children of
    cell 0, child (ox, oy, oz) at ox * R^2 + oy * R + oz, all neighbours empty or outside: ctx 0, one occupied of eight."""
    g = np.zeros((1, 16, 16, 16), np.uint8)
    g[0, 0, 0, 0] = 1
    m = twin.model(g)
    assert m["K"] == 4 and [lv.shape for lv in m["levels"]] == [(1, 16, 16, 16), (1, 8, 8, 8), (1, 4, 4, 4), (1, 2, 2, 2), (1, 1, 1, 1)]
    assert all(int(lv.sum()) == 1 and lv[0, 0, 0, 0] == 1 for lv in m["levels"])
    assert m["raw"] == b"\x01"
    want_idx = {0: [0, 1, 16, 17, 256, 257, 272, 273], 1: [0, 1, 8, 9, 64, 65, 72, 73], 2: [0, 1, 4, 5, 16, 17, 20, 21],
                3: [0, 1, 2, 3, 4, 5, 6, 7]}
    for k in range(4):
        lv = m["per"][k]
        assert lv["n"] == 8 and lv["idx"].tolist() == want_idx[k] and lv["ctx"].tolist() == [0] * 8
        assert lv["sym"].tolist() == [1.0] + [-1.0] * 7
        assert lv["hist"][0].tolist() == [1, 8] and int(lv["hist"][1:].sum()) == 0
        assert lv["c1"][0] == 57344 and (lv["c1"][1:] == 32768).all()           # 7 / 8 of 2^16; unused contexts
        assert abs(lv["ideal_bits"] - (-np.log2(1 / 8) - 7 * np.log2(7 / 8))) < 1e-9


def test_two_cells_contexts_by_hand():
    """Cells (0,0,0) and (2,0,0) of 16^3: parents (0,0,0) and (1,0,0) of the 8^3 level.  A child on the side of the other
    parent sees it as a near face (ctx 4), a child on the far side as an opposite face (ctx 1)."""
    g = np.zeros((1, 16, 16, 16), np.uint8)
    g[0, 0, 0, 0] = g[0, 2, 0, 0] = 1
    lv = twin.model(g)["per"][0]
    assert lv["idx"].tolist() == [0, 1, 16, 17, 256, 257, 272, 273, 512, 513, 528, 529, 768, 769, 784, 785]
    assert lv["ctx"].tolist() == [1] * 4 + [4] * 4 + [4] * 4 + [1] * 4
    assert lv["sym"].tolist() == [1.0] + [-1.0] * 7 + [1.0] + [-1.0] * 7
    assert lv["hist"][1].tolist() == [1, 8] and lv["hist"][4].tolist() == [1, 8]


def test_empty_and_full_grids():
    e = twin.model(np.zeros((1, 16, 16, 16), np.uint8))
    assert e["raw"] == b"\x00" and all(lv["n"] == 0 and lv["ideal_bits"] == 0.0 for lv in e["per"])
    assert all((lv["c1"] == 32768).all() for lv in e["per"])
    f = twin.model(np.ones((2, 8, 8, 8), np.uint8))
    assert f["K"] == 3 and f["raw"] == b"\x03"
    for k, lv in enumerate(f["per"]):
        assert lv["n"] == 2 * 8 ** 3 >> (3 * k) and (lv["sym"] == 1).all()
        assert lv["idx"].tolist() != sorted(lv["idx"].tolist()) or lv["n"] == 16      # parent order, not child order
        assert sorted(lv["idx"].tolist()) == list(range(lv["n"]))
        used = lv["hist"][:, 1] > 0
        assert (lv["c1"][used] == 1).all() and (lv["c1"][~used] == 32768).all()     # P(empty) clamps at 1 / 2^16
    # the corner child of a full 4^3 parent level: its side is outside the grid, the three opposite faces are occupied
    lv = f["per"][0]
    assert lv["ctx"][0] == 3 and lv["idx"][0] == 0
    inner = np.ravel_multi_index((0, 1, 1, 1), (2, 4, 4, 4)) * 8                 # parent (1,1,1), octant 0: everything occupied
    assert lv["ctx"][inner] == 7 * 4 + 3


def test_odd_side_has_no_pyramid():
    for f in (twin.levels_of, oc.levels_of):
        with pytest.raises(ValueError):
            f((1, 17, 17, 17))
        with pytest.raises(ValueError):
            f((1, 16, 16, 18 + 1))
        assert f((1, 18, 18, 18)) == 1 and f((1, 32, 48, 16)) == 4 and f((2, 128, 128, 128)) == 4 and f((1, 24, 8, 40)) == 3


def test_c1_round_trip_through_both_quantisers():
    """The float handed to the coders gives back the stored c1 for every c1 in [1, 65535], under the range coder's
    quantiser and under rans1's."""
    from cnc_amd import _codec
    L = _codec.lib()
    c1 = np.arange(1, 65536)
    for p_of in (twin.p_of_c1, oc.p_of_c1):
        p = p_of(c1)
        assert p.dtype == np.float32 and (p >= 0).all() and (p <= 1).all()
        assert [int(L.cnc_rc_c1(float(v))) for v in p] == c1.tolist()
        assert [int(L.cnc_rans_c1(float(v))) for v in p] == c1.tolist()


def test_package_helpers_agree_with_the_twin():
    rng = np.random.default_rng(3)
    for ones, total in [(0, 1), (1, 1), (1, 2), (1, 3), (2, 3), (0, 10 ** 6), (10 ** 6, 10 ** 6), (1, 2 ** 21), (2 ** 21 - 1, 2 ** 21)] + \
            [(int(o), int(t)) for t in rng.integers(1, 2 ** 21, 200) for o in [rng.integers(0, t + 1)]]:
        assert oc.c1_of_counts(ones, total) == twin.c1_of_counts(ones, total)
        assert 1 <= oc.c1_of_counts(ones, total) <= 65535
    assert oc.c1_of_counts(0, 0) == 32768 == twin.c1_of_counts(0, 0)
    assert oc.c1_of_counts(1, 2) == 32768 and oc.c1_of_counts(1, 4) == 49152 and oc.c1_of_counts(3, 4) == 16384
    g = (rng.uniform(size=(2, 8, 16, 8)) < 0.2).astype(np.uint8)
    m = twin.model(g)
    c1 = np.stack([lv["c1"] for lv in m["per"]])
    streams = [bytes([k + 1]) * (k + 2) for k in range(m["K"])]
    payload = oc.join_payload(m["levels"][-1], c1, streams)
    info = dict(model="pyramid1", shape=list(g.shape), levels=m["K"], n=[8] * m["K"], stream_sizes=[len(s) for s in streams])
    for top, tab, st in (oc.split_payload(payload, info), twin.split_payload(payload, g.shape, info["n"], info["stream_sizes"])):
        assert np.array_equal(top, m["levels"][-1]) and np.array_equal(tab, c1) and list(st) == streams
    assert payload[:len(m["raw"])] == m["raw"]
    with pytest.raises(RuntimeError):
        oc.split_payload(payload[:-1], info)
    with pytest.raises(RuntimeError):
        oc.split_payload(payload, dict(info, n=[8] * (m["K"] - 1) + [4]))


def test_round_trip_through_the_host_coder(tmp_path):
    """twin -> encoder -> decoder -> twin on 32^3, and the coded size against the twin's ideal length with the bound the
    range coder is held to (1.002 x ideal + 64 bits per stream)."""
    from cnc_amd.context import decoder, encoder
    g = twin.ball(32, radius=0.6)
    g[0, 3:5, 28:31, 0] = 1
    g[0, 31, 31, 31] = 1
    m = twin.model(g)
    assert m["K"] == 4 and all(lv["n"] > 0 for lv in m["per"])
    files = {}
    for k, lv in enumerate(m["per"]):
        files[k] = str(tmp_path / f"l{k}.b")
        bits = encoder(torch.from_numpy(lv["sym"]), torch.from_numpy(twin.p_of_c1(lv["c1"])[lv["ctx"]]), files[k])
        assert bits == 8 * os.path.getsize(files[k]) and bits <= lv["ideal_bits"] * 1.002 + 64
    c1 = np.stack([lv["c1"] for lv in m["per"]])
    back = twin.decode(m["levels"][-1], c1, [lv["n"] for lv in m["per"]],
                       lambda k, p: decoder(torch.from_numpy(p), files[k]).numpy())
    assert np.array_equal(back, g)
    assert sum(os.path.getsize(f) for f in files.values()) < 32 ** 3 // 8 // 4      # a ball: far below a bit per cell


def test_mirror_and_codec_refuse_host_tensors():
    from cnc_amd.backends import occ_pyramid as B
    g = torch.zeros(1, 16, 16, 16, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        B.reduce(g, 4, torch.zeros(1000, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        B.rank(g, torch.zeros(64, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        B.emit(g, torch.zeros(64, dtype=torch.int32), 8, torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        B.probs(torch.zeros(8, dtype=torch.uint8), torch.zeros(32), torch.zeros(8))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        oc.encode_occupancy(g.bool())
    with pytest.raises(RuntimeError, match="GPU only"):
        oc.decode_occupancy(b"", dict(model="pyramid1"), "cpu")


def test_odd_grid_keeps_the_iid_section(tmp_path):
    """write_container with the pyramid selected on a grid that has no pyramid: the Bernoulli section, byte for byte."""
    from cnc_amd.container import read_container, write_container
    g = torch.from_numpy(twin.ball(17, radius=0.7)).bool()
    kw = dict(meta={}, table_streams={}, binaries=g, field_mlp={}, context_state={})
    write_container(str(tmp_path / "a.cnc"), **kw)
    write_container(str(tmp_path / "b.cnc"), occupancy_coder="pyramid", **kw)
    assert open(tmp_path / "a.cnc", "rb").read() == open(tmp_path / "b.cnc", "rb").read()
    assert torch.equal(read_container(str(tmp_path / "b.cnc"))[2], g)
    with pytest.raises(ValueError):
        write_container(str(tmp_path / "c.cnc"), occupancy_coder="octree", **kw)
