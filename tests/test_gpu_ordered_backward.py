"""The ordered encoder backward (cnc_grid_encode_backward_ordered, through the mirror and through GridEncoder) against the
CPU oracle's serial sum: every comparison is on the fp32 bits, there is no tolerance anywhere (one float64-shadow
check at the end is the sanity anchor the atomic routes' tests use)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ball_occupancy, make_grid

pytestmark = pytest.mark.gpu

LOG2_T = 12          # the fine levels hashed, the coarse ones dense
N_PTS = 4099
RES = {3: [4, 9, 33, 130], 2: [3, 17, 300], 1: [5, 64, 5000]}


def _points(N, D, seed):
    """Uniform in [-0.02, 1.02]^D (some out of range); the first 7 exactly 0, the next 7 exactly 1, 26 copies of one."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.02, 1.02, size=(N, D)).astype(np.float32)
    if N >= 64:
        x[:7] = 0.0
        x[7:14] = 1.0
        x[14:40] = rng.uniform(0.2, 0.8, size=D).astype(np.float32)
    return x


def _grads(L, N, F, seed):
    return np.random.default_rng(seed).normal(size=(L, N, F)).astype(np.float32)


def _same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _masks(dev, vxl, res, mask):
    """(occ_sat, vertex_bits) for mask in scan / sat / vertex_bits."""
    if vxl is None or mask == "scan":
        return None, None
    from cnc_amd.backends import gridencoder_backend as be
    v = torch.as_tensor(vxl, device=dev)
    sat = be.occupancy_sat(v)
    return sat, (be.occupancy_vertex_bits(v, sat, [int(r) for r in res]) if mask == "vertex_bits" else None)


def _ordered(dev, g, x, emb, offs, res, vxl=None, mli=None, ste=False, mask="scan", into=None, clip=None, **kw):
    """One ordered call through the mirror; `into`: the device buffer to accumulate into (default: fresh zeros)."""
    from cnc_amd.backends import gridencoder_backend as be
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev)
    L, N, F = g.shape
    D = x.shape[1]
    ge = torch.zeros(emb.shape, dtype=torch.float32, device=dev) if into is None else into
    Rb = 128 if vxl is None else vxl.shape[-1]
    sat, vb = _masks(dev, vxl, res, mask)
    before = be.ROUTE_CALLS["ordered"]
    be.grid_encode_backward(t(g), t(x), t(emb), t(offs), t(res), ge, N, D, F, L, 0, Rb, None, None, t(vxl), t(mli),
                            ste_binary=ste, ste_clip_count=clip, occ_sat=sat, vertex_bits=vb, ordered=True, **kw)
    assert be.ROUTE_CALLS["ordered"] == before + 1
    torch.cuda.synchronize()
    return ge.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("ste", [False, True], ids=["plain", "ste"])
@pytest.mark.parametrize("D,F", [(3, 1), (3, 2), (3, 4), (3, 8), (3, 16), (2, 2), (2, 8), (1, 4)])
def test_shapes_bit_equal_to_serial_oracle(cuda, oracle, D, F, ste):
    res = RES[D]
    offs, resl, emb = make_grid(res, LOG2_T, D, F, seed=10 * D + F)
    x = _points(N_PTS, D, seed=D)
    g = _grads(len(res), N_PTS, F, seed=F)
    want = oracle.grid_encode_backward(g, x, emb, offs, resl, ste_binary=ste, threads=1)
    got = _ordered(cuda, g, x, emb, offs, resl, ste=ste)
    assert np.count_nonzero(want) > 1000
    assert _same_bits(got, want)
    if ste:
        assert np.all(got[np.abs(emb) > 1] == 0)
    if D == 3 and F == 2:                                      # the same call again, into a fresh buffer
        assert _same_bits(_ordered(cuda, g, x, emb, offs, resl, ste=ste), got)


# ---------------------------------------------------------------------------------------------- 2. one long row
def test_one_long_row(cuda, oracle):
    """At R = 3 the single interior vertex receives every term: one row's sum of ~10^5 terms crosses any block or chunk
    boundary a parallel reduce might introduce."""
    N = 20011
    offs, resl, emb = make_grid([3, 5], LOG2_T, 3, 2, seed=2)
    x = _points(N, 3, seed=21)
    g = _grads(2, N, 2, seed=22)
    want = oracle.grid_encode_backward(g, x, emb, offs, resl, threads=1)
    assert np.count_nonzero(want[offs[0]:offs[1]].any(axis=1)) == 1       # one row holds the whole level
    assert _same_bits(_ordered(cuda, g, x, emb, offs, resl), want)


# ---------------------------------------------------------------------------------------------- 3. mask and windows
@pytest.mark.parametrize("mask", ["scan", "sat", "vertex_bits"])
def test_mask_and_per_point_windows(cuda, oracle, mask):
    """Per-point level windows make different slots hit the same rows: slot-major order is what is tested."""
    res = [4, 9, 33, 65, 130]
    offs, resl, emb = make_grid(res, LOG2_T, 3, 4, seed=31)
    vxl = ball_occupancy(16)
    x = _points(N_PTS, 3, seed=32)
    mli = np.random.default_rng(33).integers(0, 3, size=N_PTS).astype(np.int32)
    g = _grads(3, N_PTS, 4, seed=34)
    for ste in (False, True):
        want = oracle.grid_encode_backward(g, x, emb, offs, resl, binary_vxl=vxl, min_level_id=mli, ste_binary=ste,
                                           threads=1)
        got = _ordered(cuda, g, x, emb, offs, resl, vxl=vxl, mli=mli, ste=ste, mask=mask)
        assert np.count_nonzero(want) > 1000
        assert _same_bits(got, want)


# ---------------------------------------------------------------------------------------------- 4. a used buffer
def test_accumulates_into_a_used_buffer(cuda, oracle):
    """Two calls on point sets A and B into one buffer = the oracle on [A; B]: per element, A's terms, then B's."""
    res = RES[3]
    offs, resl, emb = make_grid(res, LOG2_T, 3, 8, seed=41)
    xa, xb = _points(N_PTS, 3, seed=42), _points(1531, 3, seed=43)
    ga, gb = _grads(len(res), N_PTS, 8, seed=44), _grads(len(res), 1531, 8, seed=45)
    want = oracle.grid_encode_backward(np.concatenate([ga, gb], axis=1), np.concatenate([xa, xb]), emb, offs, resl,
                                       ste_binary=True, threads=1)
    buf = torch.zeros(emb.shape, dtype=torch.float32, device=cuda)
    _ordered(cuda, ga, xa, emb, offs, resl, ste=True, into=buf)
    got = _ordered(cuda, gb, xb, emb, offs, resl, ste=True, into=buf)
    assert _same_bits(got, want)


# ---------------------------------------------------------------------------------------------- 5. layout and hint
def test_point_major_gradient_layout(cuda, oracle):
    res = RES[3]
    F, L = 4, len(RES[3])
    offs, resl, emb = make_grid(res, LOG2_T, 3, F, seed=51)
    x = _points(N_PTS, 3, seed=52)
    g = _grads(L, N_PTS, F, seed=53)
    want = oracle.grid_encode_backward(g, x, emb, offs, resl, threads=1)
    level_major = _ordered(cuda, g, x, emb, offs, resl)
    ld, col = L * F + 12, 8
    wide = np.random.default_rng(54).normal(size=(N_PTS, ld)).astype(np.float32)
    wide[:, col:col + L * F] = g.transpose(1, 0, 2).reshape(N_PTS, L * F)
    from cnc_amd.backends import gridencoder_backend as be
    t = lambda a: torch.as_tensor(a, device=cuda)
    ge = torch.zeros(emb.shape, dtype=torch.float32, device=cuda)
    be.grid_encode_backward(t(wide), t(x), t(emb), t(offs), t(resl), ge, N_PTS, 3, F, L, 0, 128, None, None, None, None,
                            grad_ld=ld, grad_col=col, ordered=True)
    assert _same_bits(ge.cpu().numpy(), level_major)
    assert _same_bits(level_major, want)


@pytest.mark.parametrize("outliers", [False, True])
def test_ste_clip_count_hint(cuda, oracle, outliers):
    """The counter reading 0 (no |v| > 1: the mask is the identity and is skipped) and reading non-zero."""
    from cnc_amd.backends import gridencoder_backend as be
    res = RES[3]
    offs, resl, emb = make_grid(res, LOG2_T, 3, 8, seed=55)
    if not outliers:
        emb = np.clip(emb, -1.0, 1.0)
    x = _points(N_PTS, 3, seed=56)
    g = _grads(len(res), N_PTS, 8, seed=57)
    clip = torch.empty(1, dtype=torch.int32, device=cuda)
    be.pack_sign_bits(torch.as_tensor(emb, device=cuda), None, clip)
    assert (int(clip.item()) != 0) == outliers
    want = oracle.grid_encode_backward(g, x, emb, offs, resl, ste_binary=True, threads=1)
    assert _same_bits(_ordered(cuda, g, x, emb, offs, resl, ste=True, clip=clip), want)


# ---------------------------------------------------------------------------------------------- 6. scratch, stream
def test_poisoned_scratch_and_side_stream(cuda, oracle):
    from cnc_amd import _lib
    from cnc_amd.backends import gridencoder_backend as be
    res = RES[3]
    offs, resl, emb = make_grid(res, LOG2_T, 3, 8, seed=61)
    x = _points(N_PTS, 3, seed=62)
    g = _grads(len(res), N_PTS, 8, seed=63)
    want = oracle.grid_encode_backward(g, x, emb, offs, resl, ste_binary=True, threads=1)
    nbytes = int(_lib.lib().cnc_grid_encode_backward_ordered_workspace(N_PTS, 3, emb.shape[0]))
    assert nbytes >= 5 * 4 * N_PTS * 8
    ws = be._workspace(cuda, nbytes, (_lib.stream(cuda), "ordered"))
    ws.fill_(0xFF)
    assert _same_bits(_ordered(cuda, g, x, emb, offs, resl, ste=True), want)
    assert be._workspace(cuda, nbytes, (_lib.stream(cuda), "ordered")) is ws          # the poisoned buffer was the one used
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        got = _ordered(cuda, g, x, emb, offs, resl, ste=True)
    torch.cuda.current_stream(cuda).wait_stream(side)
    assert _same_bits(got, want)


# ---------------------------------------------------------------------------------------------- 7. degenerate sizes
def test_degenerate_sizes_leave_the_buffer_untouched(cuda):
    res = RES[3]
    offs, resl, emb = make_grid(res, LOG2_T, 3, 2, seed=71)
    fill = np.random.default_rng(72).normal(size=emb.shape).astype(np.float32)
    buf = torch.as_tensor(fill, device=cuda)
    got = _ordered(cuda, np.zeros((len(res), 0, 2), np.float32), np.zeros((0, 3), np.float32), emb, offs, resl, into=buf)
    assert _same_bits(got, fill)
    x = np.random.default_rng(73).uniform(1.001, 2.0, size=(777, 3)).astype(np.float32)
    x[::2] *= -1.0
    got = _ordered(cuda, _grads(len(res), 777, 2, seed=74), x, emb, offs, resl, ste=True, into=buf)
    assert _same_bits(got, fill)


def test_undersized_workspace_is_refused(cuda, monkeypatch):
    from cnc_amd import _lib
    from cnc_amd.backends import gridencoder_backend as be
    res = RES[3]
    offs, resl, emb = make_grid(res, LOG2_T, 3, 2, seed=75)
    N = 1000
    x, g = _points(N, 3, seed=76), _grads(len(res), N, 2, seed=77)
    lib = _lib.lib()
    nbytes = int(lib.cnc_grid_encode_backward_ordered_workspace(N, 3, emb.shape[0]))
    t = lambda a: torch.as_tensor(a, device=cuda)
    gd, xd, ed, od, rd = t(g), t(x), t(emb), t(offs), t(resl)
    ge = torch.zeros(emb.shape, dtype=torch.float32, device=cuda)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    p = lambda a: C.c_void_p(a.data_ptr())
    args = (p(gd), p(xd), p(ed), p(od), p(rd), p(ge), N, 3, 2, len(res), 128, None, None, None, None, 0, None, None, None,
            None, 0, 0, p(ws))
    torch.cuda.synchronize()
    assert lib.cnc_grid_encode_backward_ordered(*args, nbytes - 1, None) == -1       # CNC_ERR_INVALID_VALUE
    torch.cuda.synchronize()
    assert not ge.any().item()                                                       # and nothing ran
    assert lib.cnc_grid_encode_backward_ordered(*args, nbytes, None) == 0
    torch.cuda.synchronize()
    assert ge.any().item()
    # the mirror raises what the library returns
    real = lib.cnc_grid_encode_backward_ordered_workspace
    monkeypatch.setattr(lib, "cnc_grid_encode_backward_ordered_workspace", lambda *a: int(real(*a)) - 1, raising=False)
    with pytest.raises(RuntimeError, match="grid_encode_backward_ordered"):
        be.grid_encode_backward(gd, xd, ed, od, rd, ge, N, 3, 2, len(res), 0, 128, None, None, None, None, ordered=True)
    # N * 2^D past 32 bits: refused
    assert real(1 << 30, 3, emb.shape[0]) == 0
    assert lib.cnc_grid_encode_backward_ordered(*args[:6], 1 << 30, *args[7:], nbytes, None) == -1


# ---------------------------------------------------------------------------------------------- 8. public interface
def _encoder(cuda, emb, res, **kw):
    from cnc_amd.gridencoder import GridEncoder
    enc = GridEncoder(num_dim=3, n_features=emb.shape[1], resolutions_list=res, log2_hashmap_size=LOG2_T,
                      ste_binary=True, **kw).to(cuda)
    with torch.no_grad():
        enc.params.copy_(torch.as_tensor(emb, device=cuda))
    enc.invalidate_caches()
    return enc


def _module_grad(enc, x, gout, **fw):
    enc.params.grad = None
    out = enc(x, **fw) if "min_level_id_list" not in fw else enc.forward_diff_levels(x, **fw)
    out.backward(gout)
    torch.cuda.synchronize()
    return enc.params.grad.cpu().numpy()


@pytest.fixture(scope="module")
def module_case(oracle):
    res = RES[3]
    F, L = 4, len(res)
    offs, resl, emb = make_grid(res, LOG2_T, 3, F, seed=81)
    x = _points(N_PTS, 3, seed=82)
    g = _grads(L, N_PTS, F, seed=83)
    want = oracle.grid_encode_backward(g, x, emb, offs, resl, ste_binary=True, threads=1)
    gout = g.transpose(1, 0, 2).reshape(N_PTS, L * F).copy()                   # the module's [N, L * F] output layout
    return res, emb, x, gout, want


def test_module_override(cuda, oracle, module_case):
    from cnc_amd.backends import gridencoder_backend as be
    res, emb, x, gout, want = module_case
    enc = _encoder(cuda, emb, res, ordered_backward=True)
    xd, gd = torch.as_tensor(x, device=cuda), torch.as_tensor(gout, device=cuda)
    before = dict(be.ROUTE_CALLS)
    assert _same_bits(_module_grad(enc, xd, gd), want)
    assert be.ROUTE_CALLS["ordered"] == before["ordered"] + 1 and be.ROUTE_CALLS["default"] == before["default"]
    # a masked forward_diff_levels call
    res5 = [4, 9, 33, 65, 130]
    offs, resl, emb5 = make_grid(res5, LOG2_T, 3, 4, seed=84)
    vxl = ball_occupancy(16)
    mli = np.random.default_rng(85).integers(0, 3, size=N_PTS).astype(np.int32)
    g = _grads(3, N_PTS, 4, seed=86)
    want5 = oracle.grid_encode_backward(g, x, emb5, offs, resl, binary_vxl=vxl, min_level_id=mli, ste_binary=True, threads=1)
    enc5 = _encoder(cuda, emb5, res5, ordered_backward=True)
    got5 = _module_grad(enc5, xd, torch.as_tensor(g.transpose(1, 0, 2).reshape(N_PTS, 12).copy(), device=cuda),
                        min_level_id_list=torch.as_tensor(mli, device=cuda), n_levels_calc=3,
                        binary_vxl=torch.as_tensor(vxl, device=cuda))
    assert _same_bits(got5, want5)


def test_process_wide_mode_and_torch_switch(cuda, module_case):
    import cnc_amd
    from cnc_amd.backends import gridencoder_backend as be
    res, emb, x, gout, want = module_case
    enc = _encoder(cuda, emb, res)                                             # ordered_backward=None: follows the mode
    xd, gd = torch.as_tensor(x, device=cuda), torch.as_tensor(gout, device=cuda)
    assert not be.ordered_backward_enabled()

    before = dict(be.ROUTE_CALLS)
    _module_grad(enc, xd, gd)                                                  # outside: today's route
    assert be.ROUTE_CALLS["default"] == before["default"] + 1 and be.ROUTE_CALLS["ordered"] == before["ordered"]

    with cnc_amd.ordered_backward():
        got = _module_grad(enc, xd, gd)
    assert be.ROUTE_CALLS["ordered"] == before["ordered"] + 1
    assert _same_bits(got, want)

    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        got = _module_grad(enc, xd, gd)
    finally:
        torch.use_deterministic_algorithms(was)
    assert be.ROUTE_CALLS["ordered"] == before["ordered"] + 2
    assert _same_bits(got, want)

    _module_grad(enc, xd, gd)                                                  # and outside again
    assert be.ROUTE_CALLS["default"] == before["default"] + 2 and be.ROUTE_CALLS["ordered"] == before["ordered"] + 2
    # an explicit False on the module beats the mode
    off = _encoder(cuda, emb, res, ordered_backward=False)
    with cnc_amd.ordered_backward():
        _module_grad(off, xd, gd)
    assert be.ROUTE_CALLS["default"] == before["default"] + 3


# ---------------------------------------------------------------------------------------------- sanity anchor
def test_float64_shadow_bound_holds(cuda, oracle):
    """The check the atomic routes' tests use (tests/test_gpu_encoder.py `_check_bwd`), on one case."""
    res = RES[3]
    offs, resl, emb = make_grid(res, LOG2_T, 3, 8, seed=91)
    x = _points(N_PTS, 3, seed=92)
    g = _grads(len(res), N_PTS, 8, seed=93)
    want32, acc64 = oracle.grid_encode_backward(g, x, emb, offs, resl, ste_binary=True, want_acc64=True)
    _, abs64 = oracle.grid_encode_backward(np.abs(g), x, emb, offs, resl, ste_binary=True, want_acc64=True)
    got = _ordered(cuda, g, x, emb, offs, resl, ste=True)
    eps = np.finfo(np.float32).eps
    bound = (N_PTS * 8 + 2) * eps * abs64 + 1e-30        # |fp32 sum in any order - exact| <= (n - 1) eps sum|terms|
    assert np.all(np.abs(got.astype(np.float64) - acc64) <= bound)
    assert np.all(np.abs(want32.astype(np.float64) - acc64) <= bound)
    assert np.all(got[abs64 == 0] == 0)
