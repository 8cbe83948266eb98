"""The stream records of cnc_amd.context (`_Stream`, `_streams_3D`, `_stream_2D`): the one description of which .b
file carries which rows of which table, as the encoder and the decoder walk it on the toy model of
tests/test_gpu_context.py (F = 4, finest resolution 34, level 5 of the 3-D table in two chunks)."""
import os

import pytest
import torch

from test_gpu_context import setup  # noqa: F401  (fixture: golden vectors, toy model, its four encoders, occupancy grid)

pytestmark = pytest.mark.gpu
NAMES = ("xyz", "xy", "xz", "yz")


def _record(monkeypatch, m):
    """Every record the two helpers hand out from now on, as (table name, record), in walk order."""
    log = []
    streams_3D, stream_2D = m._streams_3D, m._stream_2D

    def logged_3D(*a):
        for s in streams_3D(*a):
            log.append(("xyz", s))
            yield s

    def logged_2D(Ec, axis, *a):
        s = stream_2D(Ec, axis, *a)
        log.append((axis, s))
        return s
    monkeypatch.setattr(m, "_streams_3D", logged_3D)
    monkeypatch.setattr(m, "_stream_2D", logged_2D)
    return log


def _round_trip(m, E, binary, prefix, coder, log):
    """encode, then decode into all-ones tables: (the encoder's walk, the decoder's walk, the decoded tables by name)."""
    os.makedirs(os.path.dirname(prefix))
    del log[:]
    with torch.no_grad():
        Pgs, _, _ = m.encode_binary_vxl_mixPg_3D2D(*E, binary, filename_prefix=prefix, coder=coder)
    enc_walk = list(log)
    del log[:]
    recs = [torch.ones_like(e.params.data) for e in E]
    out = m.decode_binary_vxl_mixPg_3D2D(*E, *recs, binary, Pgs, filename_prefix=prefix, coder=coder)
    return enc_walk, list(log), dict(zip(NAMES, out))


def test_stream_records_partition_what_a_decode_writes(setup, tmp_path, monkeypatch):
    g, m, encs, binary = setup
    E = [encs[k] for k in NAMES]
    dev = binary.device
    n_rows = {k: encs[k].params.shape[0] for k in NAMES}
    assert max(len(m._chunks_3D(n)) for n in range(m.n_levels) if m._coded_3D(n)) > 1      # a coded level in several chunks
    log = _record(monkeypatch, m)

    def rows_of(name, dst):
        return torch.arange(n_rows[name], device=dev)[dst]

    signs = {k: torch.where(encs[k].params.data >= 0, 1.0, -1.0) for k in NAMES}
    union = None
    for coder in ("host", "device"):
        enc_walk, dec_walk, out = _round_trip(m, E, binary, str(tmp_path / coder / "b"), coder, log)
        # the file list is the golden one, and the two walks describe every file alike
        assert sorted(f"b_{s.suffix}.b" for _, s in dec_walk) == list(g["enc_files"])
        enc_by_file = {s.suffix: (name, s) for name, s in enc_walk}
        assert len(enc_by_file) == len(enc_walk) == len(dec_walk)
        for name, s in dec_walk:
            e_name, e = enc_by_file[s.suffix]
            assert e_name == name and torch.equal(rows_of(name, e.dst), rows_of(name, s.dst)), s.suffix
            assert s.p.dim() == 1 and s.p.numel() == rows_of(name, s.dst).numel() * m.n_features, s.suffix
            assert (s.mean is None) == (s.p.stride(0) == 0), s.suffix
        # destinations: pairwise disjoint per table
        written = {}
        for name in NAMES:
            rows = torch.cat([rows_of(name, s.dst) for t, s in dec_walk if t == name])
            assert rows.numel() > 0 and torch.unique(rows).numel() == rows.numel(), name
            written[name] = torch.zeros(n_rows[name], dtype=torch.bool, device=dev)
            written[name][rows] = True
            assert not bool(written[name].all()), name              # the toy leaves rows uncoded: the union is a real subset
        if union is not None:
            assert all(torch.equal(union[k], written[k]) for k in NAMES)
        union = written
        # decode(encode(tables)) == the tables' signs on the union, the caller's ones elsewhere
        for name in NAMES:
            assert torch.equal(out[name][union[name]], signs[name][union[name]]), (coder, name)
            assert bool((out[name][~union[name]] == 1).all()), (coder, name)

    # the union is exactly what a decode into all-ones tables can change: tables of -1 alone, coded and decoded, come back
    # -1 on every row a stream carries and +1 on every other
    keep = [e.params.data.clone() for e in E]
    try:
        for e in E:
            e.params.data.fill_(-1.0)
        _, dec_walk, out = _round_trip(m, E, binary, str(tmp_path / "minus" / "b"), "host", log)
    finally:
        for e, k in zip(E, keep):
            e.params.data.copy_(k)
    for name in NAMES:
        assert torch.equal((out[name] == -1).all(dim=1), union[name]), name
        assert torch.equal((out[name] == 1).all(dim=1), ~union[name]), name
