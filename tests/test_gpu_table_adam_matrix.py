"""cnc_table_adam (cnc_amd/csrc/table_adam.hip) through the C ABI, bit for bit against tests/adam_twin.py: p, m and v
compared as uint32 on every element of every table (NaN equal to NaN), the sign plane and the clip counter equal to the
twin's, after one call and after chained calls on the kernel's own state; at the sizes where the kernel changes path
(its scalar tail when n % 4 != 0, its 4,096-element blocks, the block-to-table search), with 0 to 4 pieces in any
slots and ranges on, before and behind block edges; every refusal of the launcher.

Every buffer, pieces included, lies inside a larger sentinel-filled allocation (tests/guarded.py): what is outside [0, n)
must be untouched, the pieces unmodified.  The main matrix asserts that the twin's m, v, p and g - m are zero or normal,
so a mismatch is never a question of the device's denormal mode; `test_subnormal_moments` is the one case that holds
subnormals.  Finding (MI355X, gfx950): none — the device keeps float32 subnormals in every conversion and in the float
g - m, and the case is bit-equal to the unflushed twin.

Not covered: tables beyond 2^32 elements (16 GiB and more per buffer), out of reach of a test of a few seconds.  The
kernel indexes with 64-bit element offsets throughout and nothing in it depends on a size between 2^20 (covered) and
that limit; the launcher's only size limit is 2^31 blocks."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_twin as T
from guarded import FILL, FILLS, Guarded

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
INVALID = -1                                             # CNC_ERR_INVALID_VALUE (include/cnc_hip.h)
TRAINER = (0.9, 0.999, 1e-15, 0.0)                       # (beta1, beta2, eps, weight decay)
TRAINER_DECAY = (0.9, 0.999, 1e-15, 2e-6)
OTHER = (0.5, 0.9, 1e-8, 0.0)
HYPERS = {"trainer": TRAINER, "trainer_decay": TRAINER_DECAY, "other": OTHER}
SIZES = [1, 3, 4, 5, 7, 8, 4092, 4095, 4096, 4097, 4100, 8191, 3 * 4096 + 1]
W = "whole"


def _L():
    from cnc_amd import _lib
    return _lib


def _signed(rng, n, lo_exp, hi_exp):
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo_exp, hi_exp, n)).astype(f32)


def _grad(rng, n):
    """The training step's magnitudes: the pieces carry the 2^10 loss scale, |g| from 1e-6 to 1e3; a seventh exact zeros."""
    g = _signed(rng, n, -6, 3)
    g[rng.integers(0, 7, n) == 0] = 0.0
    return g


def _same_bits(got, want):
    got, want = np.asarray(got, f32).reshape(-1), np.asarray(want, f32).reshape(-1)
    return (got.view(u32) == want.view(u32)) | (np.isnan(got) & np.isnan(want))


def _assert_bits(got, want, what):
    ok = _same_bits(got, want)
    if not ok.all():
        i = int(np.argmin(ok))
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ, first at {i}: "
                             f"got {got.reshape(-1)[i]!r} want {want.reshape(-1)[i]!r}")


def _zero_or_normal(x):
    x = np.abs(np.asarray(x, np.float64))
    return bool(np.all((x == 0) | (x >= np.finfo(f32).tiny) | ~np.isfinite(x)))


class _Table:
    """One table's buffers on the device and the same state on the host."""

    def __init__(self, dev, rng, n, slots, with_step=True, with_sign=False, zero_state=False, p=None, p_scale=(-4, 0),
                 fill=FILL):
        """`fill`: the byte around (and, for the sign plane, inside) every buffer of this table (guarded.FILLS)."""
        self.dev, self.n, self.slots, self.fill_byte = dev, n, list(slots) + [None] * (4 - len(slots)), fill
        self.p = _signed(rng, n, *p_scale) if p is None else np.asarray(p, f32)
        self.m = np.zeros(n, f32) if zero_state else _signed(rng, n, -6, 2)
        self.v = np.zeros(n, f32) if zero_state else np.abs(_signed(rng, n, -10, 5))
        self.P, self.M, self.V = (Guarded(t, dev, fill=fill) for t in (self.p, self.m, self.v))
        self.step = Guarded(np.zeros(1, f32), dev, fill=fill) if with_step else None
        self.steps = 0.0
        self.bits = Guarded.empty((n // 8,), np.uint8, dev, fill=fill) if with_sign else None
        self.clip = Guarded(np.array([5], u32), dev, fill=fill) if with_sign else None       # the kernel adds to it
        self.clipped = 5
        self.pieces, self.G = [None] * 4, [None] * 4

    def ranges(self):
        return [None if s is None else ((0, self.n) if s == W else s) for s in self.slots]

    def draw(self, rng, grads=None):
        """Fresh gradient pieces for one call, each in its own guarded buffer."""
        for k, r in enumerate(self.ranges()):
            if r is None:
                continue
            q = _grad(rng, r[1] - r[0]) if grads is None else np.asarray(grads[k], f32)
            self.pieces[k] = (q, r[0], r[1])
            self.G[k] = Guarded(q if q.size else np.zeros(4, f32), self.dev, fill=self.fill_byte)     # an empty range still needs an address

    def fill(self, t):
        t.p, t.m, t.v, t.n = self.P.ptr, self.M.ptr, self.V.ptr, self.n
        t.step = self.step.ptr if self.step else None
        for k, pc in enumerate(self.pieces):
            if pc is not None:
                t.g[k], t.g_lo[k], t.g_hi[k] = self.G[k].ptr, pc[1], pc[2]
        if self.bits is not None:
            t.sign_bits, t.clip_count = self.bits.ptr, self.clip.ptr

    def guards(self):
        return [b for b in (self.P, self.M, self.V, self.step, self.bits, self.clip, *self.G) if b is not None]


def _struct(tables):
    a = _L().AdamTables()
    a.n_tables = len(tables)
    for k, t in enumerate(tables):
        t.fill(a.table[k])
    return a


def _call(a, hyper, lr, step):
    b1, b2, eps, wd = hyper
    rc = _L().lib().cnc_table_adam(C.byref(a), float(lr), b1, b2, eps, wd, float(step),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _step_and_check(tables, hyper, lr, step, rng, grads=None, twin=T.adam_step, normal=True, what=""):
    """One call over `tables`, every output against the twin of the state the call started from; the host state moves
    on to the kernel's own output."""
    for t in tables:
        t.draw(rng, None if grads is None else grads[tables.index(t)])
    assert _call(_struct(tables), hyper, lr, step) == 0, what
    b1, b2, eps, wd = hyper
    for k, t in enumerate(tables):
        tag = f"{what} table {k} (n = {t.n}) step {step}"
        want = twin(t.p, t.m, t.v, t.pieces, t.n, lr, b1, b2, eps, wd, step)
        if normal:
            assert all(_zero_or_normal(x) for x in (want.p, want.m, want.v, want.gm)), tag
        got_p, got_m, got_v = t.P.get(), t.M.get(), t.V.get()
        _assert_bits(got_m, want.m, tag + " m")
        _assert_bits(got_v, want.v, tag + " v")
        _assert_bits(got_p, want.p, tag + " p")
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


def _layouts(n):
    """Piece layouts a table of n elements can have: name -> slots (None, W, or (lo, hi) in elements)."""
    q = 4 * max(1, n // 8)                                # a multiple of 4 inside the table (n > 4)
    out = {"no piece": [], "one": [W], "two": [W, W], "three": [W, W, W], "four": [W, W, W, W],
           "slots 1 and 3": [None, W, None, W], "slot 3": [None, None, None, W], "empty range": [W, (0, 0), (n, n) if n % 4 == 0 else (0, 0)]}
    if n > 4:
        out["[0, 4k)"] = [(0, q)]
        out["[4k, n)"] = [None, (q, n)]
        out["4 elements"] = [None, None, (q - 4, q), W]
        out["overlap"] = [(0, q), (q - 4, n), W]
    if n >= 12:
        out["gap"] = [(0, 4), None, (8, n)]
        out["empty inside"] = [W, (q, q)]
    if n > 4096:
        out["ends at 4096"] = [(4088, 4096), (0, 4096)]
        out["starts at 4096"] = [(4096, n), None, (4096, 4096 + 4 * ((n - 4096) // 4))]
        out["across the edge"] = [None, (4092, n)]
    if n >= 8200:
        out["three blocks"] = [(4092, 8196), W]
    return out


@pytest.mark.parametrize("n", SIZES)
def test_one_table_every_layout(cuda, n):
    """One call from a random state per (layout, hyper-parameter set).  n % 4 != 0 runs the scalar tail; 4092 .. 4100
    put the tail and a block edge side by side; 3 * 4096 + 1 leaves one element to a fourth block."""
    rng = np.random.default_rng(n)
    for name, slots in _layouts(n).items():
        for hname, hyper in HYPERS.items():
            for fill in FILLS:                            # the bytes around (and between) the buffers: guarded.FILLS
                t = _Table(cuda, rng, n, slots, with_step=(name != "one"), fill=fill)
                _step_and_check([t], hyper, 6e-3, 3, rng, what=f"{name} / {hname} / fill {fill:#x}")


@pytest.mark.parametrize("hname", list(HYPERS))
@pytest.mark.parametrize("n", SIZES)
def test_chained_calls_on_the_kernels_own_state(cuda, n, hname):
    """Steps 1 .. 6 from zero moments with a moving learning rate, then one call each at step 1000 and at 20000 (the
    trainer's max_steps): the bias corrections of the late steps, on the state the kernel itself left."""
    rng = np.random.default_rng(1000 + n)
    lay = _layouts(n)
    slots = lay.get("overlap", lay["two"])
    for fill in FILLS:
        t = _Table(cuda, rng, n, slots, zero_state=True, with_sign=(n % 8 == 0), fill=fill)
        for step in [1, 2, 3, 4, 5, 6, 1000, 20000]:
            _step_and_check([t], HYPERS[hname], 6e-3 * (0.5 + 0.1 * (step % 7)), step, rng, what=f"{hname} / fill {fill:#x}")
        assert t.steps == 8.0


SEVERAL = [(4096, 4, 8200, 12289), (5, 4096 * 3, 8, 1 << 20), (4100, 4096), (2 * 4096 + 4, 4096, 7), (8192, 8, 4096 * 5, 3)]


@pytest.mark.parametrize("sizes", SEVERAL, ids=lambda s: "-".join(map(str, s)))
def test_several_tables_in_one_call(cuda, sizes):
    """Two to four tables: the block-to-table search (a one-block table between large ones, a table smaller than a block
    first and last), a different piece count per table, step words and sign planes given for some tables only."""
    rng = np.random.default_rng(sum(sizes))
    for fill in FILLS:
        tables = []
        for k, n in enumerate(sizes):
            lay = list(_layouts(n).values())
            slots = [[W, W, W, W], [], lay[-1], [None, W]][k]
            tables.append(_Table(cuda, rng, n, slots, with_step=(k % 2 == 0), with_sign=(n % 8 == 0 and k != 2), zero_state=True,
                                 fill=fill))
        assert len({sum(s is not None for s in t.slots) for t in tables}) >= 2
        for hyper in (TRAINER_DECAY, OTHER):
            for step in (1, 2, 3):
                _step_and_check(tables, hyper, 4e-3 * step, step, rng, what=f"{sizes} / fill {fill:#x}")
        assert [t.steps for t in tables] == [6.0 if k % 2 == 0 else 0.0 for k in range(len(sizes))]


@pytest.mark.parametrize("n", [8, 4088, 4096, 4104, 40 * 1024 + 8])
def test_sign_plane_and_clip_counter(cuda, n):
    """Tables around +-1 and a step large enough to carry entries across 0 and +-1: plane and counter equal the twin's,
    the counter (pre-loaded with 5) is added to, the plane's bytes behind n / 8 stay; a second table of the same call
    gets no plane."""
    rng = np.random.default_rng(n)
    p = rng.uniform(-1.2, 1.2, n).astype(f32)
    a = _Table(cuda, rng, n, [W, (0, 4 * (n // 8))], with_sign=True, zero_state=True, p=p)
    b = _Table(cuda, rng, n + 4, [W], with_sign=False, zero_state=True)
    for step in (1, 2, 3):
        before = a.p.copy()
        _step_and_check([b, a] if step == 2 else [a, b], TRAINER, 0.3, step, rng)
        crossed = (np.sign(before) != np.sign(a.p)).mean()
        assert n < 4096 or crossed > 0.02                                    # the signs do move
    assert a.clipped > 5


def _specials():
    one = f32(1)
    return np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(one, f32(2)), np.nextafter(-one, f32(-2)), np.nextafter(one, f32(0)),
                     np.nextafter(-one, f32(0)), np.inf, -np.inf, np.nan], f32)


def test_special_values_reach_the_plane_and_the_counter(cuda):
    """lr = 0 leaves the table as it is (p - 0 m / denom), so +-0, +-1, their neighbours, +-inf and NaN go straight into
    the nibble, the shuffle and the clip test: at even and odd float4 positions, in the first and the last byte, either
    side of a block edge.  Against the twin and against cnc_pack_sign_bits on the same table."""
    L = _L()
    n = 4096 + 64
    rng = np.random.default_rng(7)
    sp = _specials()
    p = rng.uniform(-0.9, 0.9, n).astype(f32)
    edges = np.concatenate([np.arange(0, 16), np.arange(n - 16, n), np.arange(4096 - 12, 4096 + 12)])
    for j, i in enumerate(edges):                                            # first and last byte, the block edge
        p[i] = sp[j % sp.size]
    for k in range(sp.size):                                                 # every value at every bit of a byte: at all
        for r in range(8):                                                   # four float4 lanes, even and odd float4s
            p[8 * (13 + 8 * k + r) + r] = sp[k]
    t = _Table(cuda, rng, n, [], with_sign=True, p=p)
    t.m = np.abs(t.m)                                                        # m > 0: p - (+0) keeps -0.0
    t.M = Guarded(t.m, cuda)
    _step_and_check([t], TRAINER, 0.0, 2, rng, normal=False)
    _assert_bits(t.p, p, "lr = 0 leaves the table")
    want_bits, want_clip = T.sign_plane(p)
    assert np.array_equal(t.bits.get(), want_bits) and t.clipped - 5 == want_clip
    assert want_clip >= 5 * 8                                                # 1+, -1-, +-inf and NaN, eight places each
    packed = Guarded.empty((n // 8,), np.uint8, cuda)
    count = Guarded(np.array([77], u32), cuda)                               # cnc_pack_sign_bits sets its counter
    assert L.lib().cnc_pack_sign_bits(t.P.ptr, packed.ptr, n // 8, 8, count.ptr, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(packed.get(), t.bits.get()) and int(count.get()[0]) == want_clip
    assert packed.intact() and count.intact()


def test_non_finite_gradients_follow_ieee(cuda):
    """inf and NaN in one piece: m, v and p of those elements become what IEEE arithmetic makes of them (the twin's),
    every other element is stepped as if they were not there."""
    n = 4096 + 9
    rng = np.random.default_rng(8)
    t = _Table(cuda, rng, n, [W, W])
    g0, g1 = _grad(rng, n), _grad(rng, n)
    bad = np.array([0, 5, 4095, 4096, n - 1, n - 6, 2000])
    g1[bad] = [np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf, np.inf]
    g0[2000] = -np.inf                                                       # inf + -inf in the sum
    clean = _Table(cuda, rng, n, [W, W], p=t.p)
    clean.m, clean.v = t.m.copy(), t.v.copy()
    clean.M, clean.V = Guarded(clean.m, cuda), Guarded(clean.v, cuda)
    g1c = g1.copy()
    g1c[bad] = 0.0
    _step_and_check([t], TRAINER_DECAY, 6e-3, 4, rng, grads=[[g0, g1, None, None]], normal=False)
    _step_and_check([clean], TRAINER_DECAY, 6e-3, 4, rng, grads=[[g0, g1c, None, None]], normal=False)
    assert np.isnan(t.p[bad]).all() and not np.isfinite(t.m[bad]).any()
    rest = np.setdiff1d(np.arange(n), bad)
    for x, y in ((t.p, clean.p), (t.m, clean.m), (t.v, clean.v)):
        assert np.array_equal(x[rest].view(u32), y[rest].view(u32)) and np.isfinite(x[rest]).all()


def test_subnormal_moments(cuda):
    """The one case with float32 subnormals: m and g around 1e-38 (g - m and the new m subnormal), g^2 (1 - b2) below the
    normal range (v subnormal).  Bit-equal to the twin, which keeps them: the device does not flush."""
    n = 4096 + 7
    rng = np.random.default_rng(9)
    t = _Table(cuda, rng, n, [W])
    t.m = _signed(rng, n, -38.6, -37.2)
    t.v = np.abs(_signed(rng, n, -44, -37)).astype(f32)
    t.M, t.V = Guarded(t.m, cuda), Guarded(t.v, cuda)
    g = (t.m * rng.uniform(0.5, 1.5, n).astype(f32)).astype(f32)
    g[::3] = _signed(rng, g[::3].size, -20, -17)
    want = T.adam_step(t.p, t.m, t.v, [(g, 0, n)], n, 6e-3, 0.9, 0.999, 1e-15, 0.0, 2)
    tiny = np.finfo(f32).tiny
    sub = lambda x: int(((np.abs(x) < tiny) & (x != 0)).sum())
    assert sub(want.gm) > n // 10 and sub(want.v) > n // 10 and sub(want.m) > n // 100
    flushed = T.adam_step_flushing(t.p, t.m, t.v, [(g, 0, n)], n, 6e-3, 0.9, 0.999, 1e-15, 0.0, 2)
    assert not _same_bits(want.m, flushed.m).all() and not _same_bits(want.v, flushed.v).all()
    _step_and_check([t], TRAINER, 6e-3, 2, rng, grads=[[g, None, None, None]], normal=False)


def test_every_refusal_leaves_every_buffer_alone(cuda):
    """What the launcher rejects before any launch: CNC_ERR_INVALID_VALUE, and every allocation bit-identical."""
    rng = np.random.default_rng(10)
    n = 4100
    tables = [_Table(cuda, rng, n, [W, (4, 4096), None, (8, n)]), _Table(cuda, rng, 4096, [W], with_sign=True)]
    for t in tables:
        t.draw(rng)
    spare = Guarded.empty((n,), np.uint8, cuda)
    everything = [b for t in tables for b in t.guards()] + [spare]
    snaps = [b.snapshot() for b in everything]

    def refused(change, step=3.0, what=""):
        a = _struct(tables)
        change(a)
        assert _call(a, TRAINER_DECAY, 6e-3, step) == INVALID, what
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

    t0 = tables[0]
    refused(n_tables(0), what="n_tables 0")
    refused(n_tables(5), what="n_tables 5")
    refused(setter("n", 0), what="n = 0")
    for step in (0.0, 0.5, float("nan")):
        refused(lambda a: None, step=step, what=f"step {step}")
    for field, buf in (("p", t0.P), ("m", t0.M), ("v", t0.V)):
        refused(setter(field, buf.ptr + 4), what=f"{field} off alignment")
        refused(setter(field, None), what=f"{field} null")
    for k in (0, 1, 3):
        refused(setter("g", t0.G[k].ptr + 4, k), what=f"g[{k}] off alignment")
    refused(setter("g_lo", 6, 1), what="g_lo % 4")
    refused(setter("g_hi", 4094, 1), what="g_hi % 4 and not n")
    refused(setter("g_hi", n + 4, 3), what="g_hi > n")
    refused(setter("g_lo", 4100, 1), what="g_lo > g_hi")
    refused(setter("sign_bits", spare.ptr), what="sign_bits with n % 8 != 0")
    assert _L().lib().cnc_table_adam(None, 6e-3, 0.9, 0.999, 1e-15, 0.0, 1.0, None) == INVALID
    # and the same arguments unchanged are accepted
    _step_and_check(tables, TRAINER_DECAY, 6e-3, 3, np.random.default_rng(11))


# ------------------------------------------------------------------------------------------------------------------
# through cnc_amd._table_adam.TableAdam
# ------------------------------------------------------------------------------------------------------------------
def _optimizer(tables, cuda, **kw):
    other = torch.nn.Parameter(torch.ones(3, device=cuda))
    return torch.optim.Adam([{"params": [other]}, {"params": tables}], lr=6e-3, eps=1e-15, fused=True, **kw)


def _host(t):
    return t.detach().cpu().numpy().reshape(-1).copy()


@pytest.mark.parametrize("F", [1, 2])
def test_narrow_tables_through_the_wrapper(cuda, F):
    """Tables of F = 1, 2 features (numel a multiple of 4): row ranges whose element range is a multiple of 4 step as
    the twin does; one whose range is not raises and changes nothing; numel % 4 != 0 is refused at construction."""
    from cnc_amd._table_adam import TableAdam
    rng = np.random.default_rng(20 + F)
    rows = 8200 // F                                                # numel 8200: two blocks and 8 elements
    p0 = _signed(rng, rows * F, -4, 0)
    tab = torch.nn.Parameter(torch.tensor(p0, device=cuda).view(rows, F))
    opt = _optimizer([tab], cuda, weight_decay=2e-6)
    ta = TableAdam(opt, [tab])
    p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    r0, r1 = 8 // F, 4096 // F + 8 // F                             # elements [8, 4104): across the block edge
    for step in (1, 2, 3):
        whole, part, tail = _grad(rng, rows * F), _grad(rng, (r1 - r0) * F), _grad(rng, (rows - r1) * F)
        dev = lambda a: torch.tensor(a, device=cuda).view(-1, F)
        ta.step({id(tab): [(dev(whole), None), (dev(part), (r0, r1)), (dev(tail), (r1, rows))]})
        torch.cuda.synchronize()
        want = T.adam_step(p, m, v, [(whole, 0, rows * F), (part, r0 * F, r1 * F), (tail, r1 * F, rows * F)], rows * F,
                           6e-3, 0.9, 0.999, 1e-15, 2e-6, step)
        st = opt.state[tab]
        _assert_bits(_host(tab), want.p, "p")
        _assert_bits(_host(st["exp_avg"]), want.m, "m")
        _assert_bits(_host(st["exp_avg_sq"]), want.v, "v")
        assert float(st["step"]) == step == ta.steps_done
        p, m, v = want.p, want.m, want.v
    odd = (4 // F + 1, 12 // F)                                      # starts at element 5 (F = 1) or 6 (F = 2)
    with pytest.raises(RuntimeError):
        ta.step({id(tab): [(torch.ones((odd[1] - odd[0]), F, device=cuda), odd)]})
    torch.cuda.synchronize()
    st = opt.state[tab]
    _assert_bits(_host(tab), p, "p after the refused step")
    _assert_bits(_host(st["exp_avg"]), m, "m after the refused step")
    _assert_bits(_host(st["exp_avg_sq"]), v, "v after the refused step")
    assert float(st["step"]) == 3.0 and ta.steps_done == 3
    bad = torch.nn.Parameter(torch.zeros(4102 // F, F, device=cuda))
    with pytest.raises(ValueError):
        TableAdam(_optimizer([bad], cuda), [bad])


def test_a_piece_that_is_a_slice_of_an_arena(cuda):
    """A piece at a nonzero offset of a larger buffer, as cnc_amd._gradsink's table views are."""
    from cnc_amd._table_adam import TableAdam
    rng = np.random.default_rng(30)
    rows, F = 1027, 8
    n = rows * F
    p0 = _signed(rng, n, -4, 0)
    tab = torch.nn.Parameter(torch.tensor(p0, device=cuda).view(rows, F))
    opt = _optimizer([tab], cuda)
    ta = TableAdam(opt, [tab])
    arena_host = _grad(rng, 3 * n + 64)
    arena = torch.tensor(arena_host, device=cuda)
    off, off2, r0, r1 = 36, 36 + n + 12, 100, 613
    views = [(arena[off:off + n].view(rows, F), None), (arena[off2:off2 + (r1 - r0) * F].view(r1 - r0, F), (r0, r1))]
    ta.step({id(tab): views})
    torch.cuda.synchronize()
    want = T.adam_step(p0, np.zeros(n, f32), np.zeros(n, f32),
                       [(arena_host[off:off + n], 0, n), (arena_host[off2:off2 + (r1 - r0) * F], r0 * F, r1 * F)], n,
                       6e-3, 0.9, 0.999, 1e-15, 0.0, 1)
    _assert_bits(_host(tab), want.p, "p")
    _assert_bits(_host(opt.state[tab]["exp_avg"]), want.m, "m")
    _assert_bits(_host(opt.state[tab]["exp_avg_sq"]), want.v, "v")
    assert np.array_equal(arena.cpu().numpy().view(u32), arena_host.view(u32))
