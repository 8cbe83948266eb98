"""CPU-only: the reproducible mode's switch (cnc_amd._repro) — how it resolves, what it implies — the Trainer's
configuration field, and the C ABI of the two ordered entries: declared in the header, mirrored in the ctypes table,
workspace sizes without a GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    import cnc_amd
    monkeypatch.delenv("CNC_REPRODUCIBLE", raising=False)
    monkeypatch.delenv("CNC_ORDERED_BACKWARD", raising=False)
    det = torch.are_deterministic_algorithms_enabled()
    cnc_amd.reproducible(None)
    cnc_amd.ordered_backward(None)
    yield
    cnc_amd.reproducible(None)
    cnc_amd.ordered_backward(None)
    torch.use_deterministic_algorithms(det)


def test_resolution_order(monkeypatch):
    import cnc_amd
    on = cnc_amd.reproducible_enabled
    assert on() is False
    # torch's switch is the last resort ...
    torch.use_deterministic_algorithms(True)
    assert on() is True
    # ... behind the environment variable (read per call) ...
    torch.use_deterministic_algorithms(False)
    monkeypatch.setenv("CNC_REPRODUCIBLE", "1")
    assert on() is True
    monkeypatch.setenv("CNC_REPRODUCIBLE", "0")
    assert on() is False
    # ... behind the process-wide mode ...
    monkeypatch.setenv("CNC_REPRODUCIBLE", "1")
    cnc_amd.reproducible(False)
    assert on() is False
    torch.use_deterministic_algorithms(True)
    assert on() is False
    # ... behind an explicit argument
    assert on(True) is True
    cnc_amd.reproducible(True)
    assert on(False) is False and on() is True


def test_context_manager_restores_the_previous_state():
    import cnc_amd
    on = cnc_amd.reproducible_enabled
    with cnc_amd.reproducible(True):
        assert on() is True
        with cnc_amd.reproducible(False):
            assert on() is False
        assert on() is True
    assert on() is False
    cnc_amd.reproducible(True)                       # the plain setter stays set
    with cnc_amd.reproducible(None):
        assert on() is False
    assert on() is True


def test_mode_implies_the_ordered_encoder_backward(monkeypatch):
    import cnc_amd
    from cnc_amd.backends.gridencoder_backend import ordered_backward_enabled
    assert ordered_backward_enabled() is False
    with cnc_amd.reproducible(True):
        assert ordered_backward_enabled() is True
        with cnc_amd.ordered_backward(False):        # implied: not switched off from there
            assert ordered_backward_enabled() is True
    assert ordered_backward_enabled() is False
    monkeypatch.setenv("CNC_REPRODUCIBLE", "1")
    assert ordered_backward_enabled() is True
    monkeypatch.delenv("CNC_REPRODUCIBLE")
    # without the mode the encoder's own switches are what they were
    with cnc_amd.ordered_backward(True):
        assert ordered_backward_enabled() is True and cnc_amd.reproducible_enabled() is False
    torch.use_deterministic_algorithms(True)
    assert ordered_backward_enabled() is True and cnc_amd.reproducible_enabled() is True
    with cnc_amd.ordered_backward(False):
        assert ordered_backward_enabled() is False


def test_route_counters_are_exposed():
    import cnc_amd
    assert set(cnc_amd.REPRODUCIBLE_ROUTE_CALLS) == {"ctx_ordered", "ctx_default", "field_ordered", "field_default"}


def test_train_config_default_and_flag():
    from cnc_amd.trainer import TrainConfig
    assert TrainConfig().reproducible is False
    assert TrainConfig(reproducible=True).reproducible is True
    from cnc_amd import train
    src = open(train.__file__).read()
    assert "--reproducible" in src


NEW = ("cnc_ctx_mlp_backward_ordered_workspace", "cnc_ctx_mlp_backward_ordered", "cnc_field_backward_chain_ordered_workspace",
       "cnc_field_backward_chain_ordered")


def test_header_and_signature_table_agree_on_the_new_entries():
    from cnc_amd import _lib
    src = open(os.path.join(ROOT, "include", "cnc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, name
        args = [a.strip() for a in m.group(2).split(",")]
        sig = _lib.SIGNATURES[name]
        assert len(args) == len(sig), name
        for a, t in zip(args, sig):
            if "*" in a:
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, a)
            elif a.startswith("uint64_t"):
                assert t is ctypes.c_uint64, (name, a)
            else:
                assert a.startswith("uint32_t") and t is ctypes.c_uint32, (name, a)
        assert _lib.RESTYPES.get(name, ctypes.c_int) is (ctypes.c_uint64 if m.group(1) == "uint64_t" else ctypes.c_int)


def test_workspace_queries_without_a_gpu():
    from cnc_amd import _lib, build
    build.build_all()
    L = _lib.lib()
    assert L.cnc_abi_version() == _lib.ABI_VERSION
    # context heads: slots x image + a word per row + a word per (table entry, chunk of 16,384 rows), 16-byte multiples
    q = L.cnc_ctx_mlp_backward_ordered_workspace
    image1, image3 = 8 * 17 + 8, 32 * 25 + 32 + 32 * 32 + 32 + 8 * 32 + 8
    for N in (0, 1, 63, 64, 65):
        for n_layers, image, slots in ((1, image1, 2 * ((N + 127) // 128)), (3, image3, ((N + 15) // 16 + 3) // 4)):
            C = 17 if n_layers == 1 else 25
            for n_pg in (0, 1, 3):
                want = 0 if N == 0 else (4 * (slots * image + (N + n_pg if n_pg else 0)) + 15) // 16 * 16
                assert q(N, n_layers, 8, C, n_pg) == want, (N, n_layers, n_pg)
    assert q(20011, 1, 8, 17, 3) == (4 * (2 * 157 * image1 + 20011 + 3 * 2) + 15) // 16 * 16
    assert q(1 << 20, 3, 8, 25, 12) == (4 * (768 * image3 + (1 << 20) + 12 * 64) + 15) // 16 * 16      # the grid's cap
    # field chain: a slot of 3 H + 84 words per workgroup (at most 2048), nothing without the bias gradients
    f = _lib.FieldBwd()
    f.n_neurons, f.bias_grads = 160, 1 << 20
    qf = L.cnc_field_backward_chain_ordered_workspace
    for N in (0, 1, 63, 64, 65, 1 << 20):
        f.N = N
        assert qf(ctypes.byref(f)) == min((N + 31) // 32, 2048) * (3 * 160 + 84) * 4
    f.bias_grads = None
    assert qf(ctypes.byref(f)) == 0
