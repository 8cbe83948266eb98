"""cnc_table_adam_scaled (cnc_amd/csrc/table_adam.hip) through the C ABI, bit for bit against tests/adam_twin.py fed the
scaled piece PRE-MULTIPLIED in NumPy float32 (the kernel forms each product in fp32, rounds it, then adds; a factor of
exactly 1 is not multiplied): p, m, v as uint32 on every element, the step counter, the sign plane and the clip counter.

Sizes: a block is 4,096 elements — 8, 4092, 4096, 4100, 3 * 4096 + 20 on the float4 path, 4099 for the scalar tail (no sign
plane: n % 8 != 0).  Factors 0.5, 0.125, float32(1/3), float32(1/7) on slot 0 and, in a second run, on slot 2, the other
slots at 1; pieces over the whole table or over a range that starts at element 4 and ends inside the table or at n.  NULL
and all-ones factors must equal cnc_table_adam on the same inputs.  Buffers, gradients and helpers are those of
tests/test_gpu_table_adam_matrix.py (guarded allocations; gradients with |g| in [1e-6, 1e3] or zero, so every product is
zero or normal); `test_subnormal_products` is the one case that holds subnormal products."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_twin as T
import test_gpu_table_adam_matrix as M
from guarded import Guarded

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
W = M.W
SIZES = [8, 4092, 4096, 4100, 3 * 4096 + 20, 4099]
FACTORS = [f32(0.5), f32(0.125), f32(1) / f32(3), f32(1) / f32(7)]
ONES = (1.0, 1.0, 1.0, 1.0)


def _scales(slot, w):
    s = [f32(1)] * 4
    s[slot] = f32(w)
    return tuple(s)


def _call(a, scale, hyper, lr, step, entry="cnc_table_adam_scaled"):
    b1, b2, eps, wd = hyper
    lib = M._L().lib()
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "cnc_table_adam":
        rc = lib.cnc_table_adam(C.byref(a), float(lr), b1, b2, eps, wd, float(step), stream)
    else:
        arr = None if scale is None else (C.c_float * 4)(*[float(x) for x in scale])
        rc = lib.cnc_table_adam_scaled(C.byref(a), arr, float(lr), b1, b2, eps, wd, float(step), stream)
    torch.cuda.synchronize()
    return rc


def _scaled_pieces(pieces, scale):
    """What the kernel sums: slot k's values times scale[k], a float32 product — unless the factor is exactly 1."""
    out = []
    for k, pc in enumerate(pieces):
        if pc is None or scale is None or f32(scale[k]) == f32(1):
            out.append(pc)
        else:
            with np.errstate(all="ignore"):
                out.append(((pc[0] * f32(scale[k])).astype(f32), pc[1], pc[2]))
    return out


def _step_and_check(tables, scale, hyper, lr, step, rng, grads=None, normal=True, what="", entry="cnc_table_adam_scaled"):
    """One call over `tables`; every output against the twin of the state the call started from, which then moves on to the
    kernel's own output (tests/test_gpu_table_adam_matrix.py's `_step_and_check`, with the factors)."""
    for k, t in enumerate(tables):
        t.draw(rng, None if grads is None else grads[k])
    assert _call(M._struct(tables), scale, hyper, lr, step, entry) == 0, what
    b1, b2, eps, wd = hyper
    for k, t in enumerate(tables):
        tag = f"{what} table {k} (n = {t.n}) step {step} scale {scale}"
        fed = _scaled_pieces(t.pieces, scale)
        if normal:
            assert all(M._zero_or_normal(pc[0]) for pc in fed if pc is not None), tag
        want = T.adam_step(t.p, t.m, t.v, fed, t.n, lr, b1, b2, eps, wd, step)
        if normal:
            assert all(M._zero_or_normal(x) for x in (want.p, want.m, want.v, want.gm)), tag
        got_p, got_m, got_v = t.P.get(), t.M.get(), t.V.get()
        M._assert_bits(got_m, want.m, tag + " m")
        M._assert_bits(got_v, want.v, tag + " v")
        M._assert_bits(got_p, want.p, tag + " p")
        for b in t.guards():
            assert b.intact(), tag + ": wrote outside a buffer"
        for pc, G in zip(t.pieces, t.G):
            if pc is not None and pc[0].size:
                assert np.array_equal(G.get().view(u32), pc[0].view(u32)), tag + ": a piece was modified"
        if t.step:
            t.steps += 1.0
            assert float(t.step.get()[0]) == t.steps, tag
        if t.bits is not None:
            t.clipped += want.clipped
            assert np.array_equal(t.bits.get(), want.bits), tag + " sign plane"
            assert int(t.clip.get()[0]) == t.clipped, tag + " clip counter"
        t.p, t.m, t.v = got_p, got_m, got_v


def _layouts(n, slot):
    """Three pieces in slots 0 .. 2 (slot 3 too in "four"); the one in `slot` covers the whole table, or starts at element
    4 and ends inside the table (n = 8: an empty range) or at n."""
    inside = 4 * max(1, n // 8) if n > 8 else 4
    out = {}
    for name, r in (("whole", W), ("[4, inside)", (4, inside)), ("[4, n)", (4, n))):
        slots = [W, W, W]
        slots[slot] = r
        out[name] = slots
    out["four"] = [W, (4, n), W, W] if slot != 1 else [W, W, W, W]
    out["alone"] = [None] * slot + [(4, n)]
    return out


def _clone(cuda, t, slots):
    """A second table with the same p, m, v in buffers of its own."""
    c = M._Table(cuda, np.random.default_rng(0), t.n, slots, with_step=t.step is not None, with_sign=t.bits is not None, p=t.p)
    c.m, c.v = t.m.copy(), t.v.copy()
    c.M, c.V = Guarded(c.m, cuda), Guarded(c.v, cuda)
    return c


@pytest.mark.parametrize("n", SIZES)
def test_null_and_all_ones_equal_the_unscaled_entry(cuda, n):
    """The same state and pieces through cnc_table_adam, through the new entry with NULL and with four ones: all three
    bit-equal to the twin of the unscaled sum — so to each other."""
    rng = np.random.default_rng(n)
    for name, slots in _layouts(n, 0).items():
        first = M._Table(cuda, rng, n, slots, with_sign=(n % 8 == 0))
        first.draw(rng)
        grads = [[None if pc is None else pc[0] for pc in first.pieces]]
        runs = [(first, "cnc_table_adam", None), (_clone(cuda, first, slots), "cnc_table_adam_scaled", None),
                (_clone(cuda, first, slots), "cnc_table_adam_scaled", ONES)]
        for t, entry, scale in runs:
            _step_and_check([t], scale, M.TRAINER_DECAY, 6e-3, 3, rng, grads=grads, what=f"{name} / {entry}", entry=entry)
        for t, _, _ in runs[1:]:
            for x, y in ((t.p, first.p), (t.m, first.m), (t.v, first.v)):
                assert np.array_equal(x.view(u32), y.view(u32)), name


@pytest.mark.parametrize("slot", [0, 2])
@pytest.mark.parametrize("n", SIZES)
def test_one_scaled_slot_every_layout(cuda, n, slot):
    """Every factor on `slot`, the others at 1: n % 4 != 0 (4099) takes the scalar tail, the others the float4 path, with a
    sign plane where n % 8 == 0."""
    rng = np.random.default_rng(100 * n + slot)
    for name, slots in _layouts(n, slot).items():
        for j, w in enumerate(FACTORS):
            hyper = (M.TRAINER, M.TRAINER_DECAY, M.OTHER)[j % 3]
            t = M._Table(cuda, rng, n, slots, with_sign=(n % 8 == 0))
            _step_and_check([t], _scales(slot, w), hyper, 6e-3, 3, rng, what=name)


def test_the_scale_changes_the_result(cuda):
    """(the check of the checks) a factor of 0.5 on slot 0 gives another table than no factor: the comparisons above are not
    satisfied by a kernel that ignores the factors."""
    rng = np.random.default_rng(5)
    a = M._Table(cuda, rng, 4100, [W, W])
    a.draw(rng)
    grads = [[None if pc is None else pc[0] for pc in a.pieces]]
    b = _clone(cuda, a, [W, W])
    _step_and_check([a], None, M.TRAINER, 6e-3, 3, rng, grads=grads)
    _step_and_check([b], _scales(0, 0.5), M.TRAINER, 6e-3, 3, rng, grads=grads)
    assert (a.p.view(u32) != b.p.view(u32)).mean() > 0.5
    assert (a.p[4096:].view(u32) != b.p[4096:].view(u32)).any()


@pytest.mark.parametrize("slot", [0, 2])
def test_four_tables_in_one_launch(cuda, slot):
    """Four tables of different sizes (the scalar tail among them), another layout each; slot k's factor holds for every table."""
    rng = np.random.default_rng(40 + slot)
    sizes = (4100, 8, 3 * 4096 + 20, 4099)
    tables = []
    for k, n in enumerate(sizes):
        slots = list(_layouts(n, slot).values())[k]
        tables.append(M._Table(cuda, rng, n, slots, with_step=(k % 2 == 0), with_sign=(n % 8 == 0), zero_state=True))
    for j, w in enumerate(FACTORS):
        _step_and_check(tables, _scales(slot, w), M.TRAINER_DECAY, 4e-3, j + 1, rng, what=str(sizes))
    assert [t.steps for t in tables] == [4.0, 0.0, 4.0, 0.0]


@pytest.mark.parametrize("n", SIZES)
def test_three_chained_calls_on_the_kernels_own_state(cuda, n):
    """Steps 1, 2, 3 from zero moments, a data-parallel step's pieces (the summed ray-loss gradient times 1 / world first,
    then three more), another world size each step."""
    rng = np.random.default_rng(2000 + n)
    t = M._Table(cuda, rng, n, [W, W, W, (4, n)], zero_state=True, with_sign=(n % 8 == 0))
    for step, w in ((1, FACTORS[2]), (2, FACTORS[0]), (3, FACTORS[3])):
        _step_and_check([t], _scales(0, w), M.TRAINER_DECAY, 6e-3 * step, step, rng)
    assert t.steps == 3.0


def test_subnormal_products(cuda):
    """The one case with float32 subnormals (the convention of test_subnormal_moments): gradients around 1e-38 times 0.125
    are subnormal products, the moments follow.  Bit-equal to the twin, which keeps them: the device does not flush."""
    n = 4096 + 7
    rng = np.random.default_rng(9)
    t = M._Table(cuda, rng, n, [W, W])
    t.m = M._signed(rng, n, -38.6, -37.2)
    t.v = np.abs(M._signed(rng, n, -44, -37)).astype(f32)
    t.M, t.V = Guarded(t.m, cuda), Guarded(t.v, cuda)
    g0 = M._signed(rng, n, -37.9, -37.0)                                      # |g0| in 1.3e-38 .. 1e-37: g0 / 8 is subnormal
    g1 = (t.m * rng.uniform(0.5, 1.5, n).astype(f32)).astype(f32)
    scale = _scales(0, 0.125)
    tiny = np.finfo(f32).tiny
    sub = lambda x: int(((np.abs(x) < tiny) & (x != 0)).sum())
    prod = (g0 * f32(0.125)).astype(f32)
    assert sub(prod) > n // 2
    fed = [(prod, 0, n), (g1, 0, n)]
    want = T.adam_step(t.p, t.m, t.v, fed, n, 6e-3, 0.9, 0.999, 1e-15, 0.0, 2)
    flushed = T.adam_step_flushing(t.p, t.m, t.v, fed, n, 6e-3, 0.9, 0.999, 1e-15, 0.0, 2)
    assert not M._same_bits(want.m, flushed.m).all()
    _step_and_check([t], scale, M.TRAINER, 6e-3, 2, rng, grads=[[g0, g1, None, None]], normal=False)


def test_every_refusal_leaves_every_buffer_alone(cuda):
    """A factor that is NaN, infinite, zero or negative, in any slot (one with a piece or without), and everything
    cnc_table_adam refuses: CNC_ERR_INVALID_VALUE before any launch, every allocation bit-identical."""
    rng = np.random.default_rng(10)
    n = 4100
    tables = [M._Table(cuda, rng, n, [W, (4, 4096), None, (8, n)]), M._Table(cuda, rng, 4096, [W], with_sign=True)]
    for t in tables:
        t.draw(rng)
    spare = Guarded.empty((n,), np.uint8, cuda)
    everything = [b for t in tables for b in t.guards()] + [spare]
    snaps = [b.snapshot() for b in everything]
    good = _scales(0, 0.5)

    def refused(change=lambda a: None, scale=good, step=3.0, what=""):
        a = M._struct(tables)
        change(a)
        assert _call(a, scale, M.TRAINER_DECAY, 6e-3, step) == M.INVALID, what
        assert all(b.unchanged_since(s) for b, s in zip(everything, snaps)), what

    def setter(field, value, k=None):
        def f(a):
            if k is None:
                setattr(a.table[0], field, value)
            else:
                getattr(a.table[0], field)[k] = value
        return f

    def n_tables(v):
        def f(a):
            a.n_tables = v
        return f

    for k in range(4):
        for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -0.0, -0.5):
            refused(scale=_scales(k, bad), what=f"scale[{k}] = {bad}")
    t0 = tables[0]
    for scale in (good, None):
        refused(n_tables(0), scale, what="n_tables 0")
        refused(n_tables(5), scale, what="n_tables 5")
        refused(setter("n", 0), scale, what="n = 0")
        for step in (0.0, 0.5, float("nan")):
            refused(scale=scale, step=step, what=f"step {step}")
        for field, buf in (("p", t0.P), ("m", t0.M), ("v", t0.V)):
            refused(setter(field, buf.ptr + 4), scale, what=f"{field} off alignment")
            refused(setter(field, None), scale, what=f"{field} null")
        for k in (0, 1, 3):
            refused(setter("g", t0.G[k].ptr + 4, k), scale, what=f"g[{k}] off alignment")
        refused(setter("g_lo", 6, 1), scale, what="g_lo % 4")
        refused(setter("g_hi", 4094, 1), scale, what="g_hi % 4 and not n")
        refused(setter("g_hi", n + 4, 3), scale, what="g_hi > n")
        refused(setter("g_lo", 4100, 1), scale, what="g_lo > g_hi")
        refused(setter("sign_bits", spare.ptr), scale, what="sign_bits with n % 8 != 0")
    ones = (C.c_float * 4)(1, 1, 1, 1)
    assert M._L().lib().cnc_table_adam_scaled(None, ones, 6e-3, 0.9, 0.999, 1e-15, 0.0, 1.0, None) == M.INVALID
    # and the same arguments unchanged are accepted
    _step_and_check(tables, good, M.TRAINER_DECAY, 6e-3, 3, np.random.default_rng(11))


# ------------------------------------------------------------------------------------------------------------------
# through cnc_amd._table_adam.TableAdam
# ------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_scales_the_grad_piece(cuda):
    """`TableAdam.step(pieces, grad_scale)`: the factor goes to `.grad` (slot 0), 1.0 takes cnc_table_adam; a factor on a
    table without `.grad` raises and changes nothing; a TableAdam built on an optimizer that has stepped takes its count over."""
    from cnc_amd._table_adam import TableAdam
    rng = np.random.default_rng(50)
    rows, F = 1027, 4
    n = rows * F
    p0 = M._signed(rng, n, -4, 0)
    tab = torch.nn.Parameter(torch.tensor(p0, device=cuda).view(rows, F))
    opt = M._optimizer([tab], cuda, weight_decay=2e-6)
    ta = TableAdam(opt, [tab])
    assert ta.steps_done == 0 and ta.last_grad_scale == 1.0
    p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    dev = lambda a: torch.tensor(a, device=cuda).view(-1, F)
    for step, w in ((1, 0.5), (2, 1.0), (3, float(FACTORS[2]))):
        g0, g1 = M._grad(rng, n), M._grad(rng, n)
        tab.grad = dev(g0)
        ta.step({id(tab): [(dev(g1), None)]}, grad_scale=w)
        torch.cuda.synchronize()
        fed0 = g0 if w == 1.0 else (g0 * f32(w)).astype(f32)
        want = T.adam_step(p, m, v, [(fed0, 0, n), (g1, 0, n)], n, 6e-3, 0.9, 0.999, 1e-15, 2e-6, step)
        st = opt.state[tab]
        M._assert_bits(M._host(tab), want.p, "p")
        M._assert_bits(M._host(st["exp_avg"]), want.m, "m")
        M._assert_bits(M._host(st["exp_avg_sq"]), want.v, "v")
        assert float(st["step"]) == step == ta.steps_done and ta.last_grad_scale == w and tab.grad is None
        p, m, v = want.p, want.m, want.v
    with pytest.raises(RuntimeError):
        ta.step({id(tab): [(dev(M._grad(rng, n)), None)]}, grad_scale=0.5)         # `.grad` is None
    torch.cuda.synchronize()
    M._assert_bits(M._host(tab), p, "p after the refused step")
    assert float(opt.state[tab]["step"]) == 3.0 and ta.steps_done == 3
    assert TableAdam(opt, [tab]).steps_done == 3                                   # resync() at construction
    assert ta.refusal({id(tab): [(1, 5)]}, 4) is None and ta.refusal({}, 5) is not None
    odd = torch.nn.Parameter(torch.zeros(1026, 2, device=cuda))
    ta2 = TableAdam(M._optimizer([odd], cuda), [odd])
    assert ta2.refusal({id(odd): [(3, 1026)]}, 4) is not None                      # starts at element 6
    assert ta2.refusal({id(odd): [(4, 1025)]}, 4) is not None                      # ends at 2050, not n
    assert ta2.refusal({id(odd): [(4, 1026)]}, 4) is None


def test_the_trainer_checks_the_pieces_once_and_falls_back(cuda, tmp_path, monkeypatch):
    """What the kernel would refuse in the middle of a step — here a finest level whose first element is no multiple of 4 — is
    found when the optimizers are built: one warning, `fused_table_adam` off, and the steps go through `.grad` and the
    library's Adam without raising.  `load_optimizer_state` re-reads the step count the kernel's bias corrections come from."""
    import warnings
    from cnc_amd.trainer import Trainer
    from test_gpu_trainer import _cfg
    monkeypatch.delenv("CNC_TABLE_ADAM", raising=False)           # the switch's default: the kernel is on
    tr = Trainer(_cfg(tmp_path, seed=3), device=cuda)
    assert tr.table_adam is not None and tr.fused_table_adam and tr.table_adam.steps_done == 0
    for s in range(3):
        tr.train_step(s)
    assert tr.table_adam.steps_done == 3
    saved = tr.opt.state_dict()
    xyz = tr.field.mlp_base.encoding_xyz.params
    row = xyz.numel() // xyz.shape[0]
    off = tr.context._off3_host
    assert (off[-2] * row) % 4 == 0
    shift = next(k for k in (1, 2, 3) if ((off[-2] + k) * row) % 4)
    off[-2] += shift
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            tr.build_optimizers()
            tr.build_optimizers()
        assert tr.table_adam is not None and not tr.fused_table_adam
        assert sum("tables' Adam kernel is off" in str(w.message) for w in seen) == 2      # one per build, none per step
    finally:
        off[-2] -= shift
    tr.build_optimizers()
    assert tr.fused_table_adam and tr.table_adam.steps_done == 0
    tr.load_optimizer_state(saved)
    assert tr.table_adam.steps_done == 3
    tr.fused_table_adam = False
    tr.train_step(3)
    torch.cuda.synchronize()
    assert xyz.grad is not None and float(tr.opt.state[xyz]["step"]) == 4.0 == tr.table_adam.steps_done
