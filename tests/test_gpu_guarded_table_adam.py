"""cnc_table_adam_guarded (cnc_amd/csrc/table_adam.hip) through the C ABI, behind a seal of cnc_step_verdict_seal, over the
shapes of tests/test_gpu_table_adam_matrix.py: table sizes around the 4,096-element block, a tail that is no multiple of 4,
one to four tables, sub-range pieces, piece factors, sign planes.

go:    p, m, v, the sign plane and the clip counter bit-equal to tests/guarded_step_twin.py fed the scalars READ BACK from the
       verdict buffer; m and v bit-equal to cnc_table_adam at the same step t (neither depends on b^t); p within one float32
       ulp of cnc_table_adam's — the factors lr / (1 - b1^t) and sqrt(1 - b2^t) differ from the pow-based ones by at most
       t 2^-52 relative, which can move the final rounding of p to its neighbour and no further.
skip:  p, m, v, the device step, the sign plane, the clip counter and every sentinel around them keep every bit.

Every buffer lies inside a sentinel-filled allocation (tests/guarded.py)."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import guarded_step_twin as G
import test_gpu_table_adam_matrix as M
import test_gpu_table_adam_scaled as S
from guarded import Guarded

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
W = M.W
SIZES = [8, 4096, 4096 + 8, 3 * 4096 + 4, 7, 4099]              # the last two: the scalar tail
THIRD = (f32(1) / f32(3), f32(1), f32(1), f32(1))


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Verdict:
    """A cnc_step_verdict_t on the device seeded for t0 updates, and the twin of its contents."""

    def __init__(self, dev, b1, b2, t0):
        L = M._L()
        self.twin = G.seeded(b1, b2, t0)
        host = L.StepVerdict()
        host.b1_pow, host.b2_pow = self.twin.b1_pow, self.twin.b2_pow
        self.buf = Guarded(np.frombuffer(bytes(host), u32).copy(), dev)
        self.found = Guarded.empty((1,), np.float32, dev)
        self.b1, self.b2 = b1, b2

    def poison(self, reasons):
        w = self.buf.tensor()
        w[0] = reasons
        self.twin.acc = reasons

    def seal(self, lr, eps, wd, clips=()):
        L = M._L()
        a = L.VerdictSeal()
        a.verdict, a.found_inf = self.buf.ptr, self.found.ptr
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = lr, self.b1, self.b2, eps, wd
        for k, c in enumerate(clips):
            a.clip_count[k] = c.ptr
        assert L.lib().cnc_step_verdict_seal(C.byref(a), _stream()) == 0
        torch.cuda.synchronize()
        self.twin, _, _ = G.seal(self.twin, lr, self.b1, self.b2, eps, wd)
        raw = self.buf.get().tobytes()
        got = G.Verdict(*struct.unpack("4I", raw[:16]), *struct.unpack("9d", raw[16:88]))
        assert raw[16:88] == struct.pack("9d", *self.twin.doubles()), "the seal's scalars are not the twin's"
        return got                                                # what the kernel will read, read back from the device


def _guarded(tables, verdict, scale=None):
    arr = None if scale is None else (C.c_float * 4)(*[float(x) for x in scale])
    rc = M._L().lib().cnc_table_adam_guarded(C.byref(M._struct(tables)), arr, verdict.buf.ptr, _stream())
    torch.cuda.synchronize()
    return rc


def _ulps(a, b):
    a, b = (np.asarray(x, f32).view(np.int32).astype(np.int64) for x in (a, b))
    a, b = (np.where(x < 0, np.int64(-2 ** 31) - x, x) for x in (a, b))          # sign-magnitude -> ordered
    return np.abs(a - b)


def _go_and_check(cuda, tables, hyper, lr, t, rng, scale=None, t0=None, what=""):
    """One guarded go-step at step t over `tables` (fresh pieces), and the same step through cnc_table_adam /
    cnc_table_adam_scaled on clones; the host state moves on to the guarded kernel's output."""
    b1, b2, eps, wd = hyper
    for tb in tables:
        tb.draw(rng)
    clones = [S._clone(cuda, tb, tb.slots) for tb in tables]
    for tb, c in zip(tables, clones):
        c.draw(rng, grads=[None if pc is None else pc[0] for pc in tb.pieces])
    ver = _Verdict(cuda, b1, b2, t - 1 if t0 is None else t0)
    sealed = ver.seal(lr, eps, wd, [tb.clip for tb in tables if tb.clip is not None])
    assert sealed.skip == 0 and ver.found.get().view(u32)[0] == 0
    assert _guarded(tables, ver, scale) == 0, what
    assert S._call(M._struct(clones), scale, hyper, lr, t, "cnc_table_adam" if scale is None else "cnc_table_adam_scaled") == 0
    for k, (tb, c) in enumerate(zip(tables, clones)):
        tag = f"{what} table {k} (n = {tb.n}) step {t}"
        fed = S._scaled_pieces(tb.pieces, scale)
        want = G.guarded_adam_step(sealed, tb.p, tb.m, tb.v, fed, tb.n, b1, b2)
        got_p, got_m, got_v = tb.P.get(), tb.M.get(), tb.V.get()
        M._assert_bits(got_m, want.m, tag + " m against the twin")
        M._assert_bits(got_v, want.v, tag + " v against the twin")
        M._assert_bits(got_p, want.p, tag + " p against the twin")
        M._assert_bits(got_m, c.M.get(), tag + " m against cnc_table_adam")
        M._assert_bits(got_v, c.V.get(), tag + " v against cnc_table_adam")
        assert int(_ulps(got_p, c.P.get()).max()) <= 1, tag + " p against cnc_table_adam"
        for b in tb.guards():
            assert b.intact(), tag + ": wrote outside a buffer"
        for pc, Gd in zip(tb.pieces, tb.G):
            if pc is not None and pc[0].size:
                assert np.array_equal(Gd.get().view(u32), pc[0].view(u32)), tag + ": a piece was modified"
        if tb.step:
            tb.steps += 1.0
            assert float(tb.step.get()[0]) == tb.steps, tag
        if tb.bits is not None:
            assert np.array_equal(tb.bits.get(), want.bits), tag + " sign plane"
            assert int(tb.clip.get()[0]) == want.clipped, tag + " clip counter (zeroed by the seal, then added to)"
        tb.p, tb.m, tb.v = got_p, got_m, got_v
    assert ver.buf.intact() and ver.found.intact()


@pytest.mark.parametrize("n", SIZES)
def test_go_one_table_every_layout(cuda, n):
    rng = np.random.default_rng(n)
    for name, slots in M._layouts(n).items():
        hname, hyper = list(M.HYPERS.items())[len(name) % 3]
        tb = M._Table(cuda, rng, n, slots, with_step=(name != "one"), with_sign=(n % 8 == 0 and name != "two"))
        scale = THIRD if (slots and slots[0] is not None and len(name) % 2) else None
        _go_and_check(cuda, [tb], hyper, 6e-3, 3, rng, scale=scale, what=f"{name} / {hname}")


@pytest.mark.parametrize("n", [8, 4096 + 8, 3 * 4096 + 4, 4099])
def test_go_chained_on_the_kernels_own_state(cuda, n):
    """Steps 1 .. 4 from zero moments with ONE verdict buffer sealed step after step (the running products as the trainer
    has them), then single steps at t = 1000 and 20000 from pow-seeded products."""
    rng = np.random.default_rng(100 + n)
    lay = M._layouts(n)
    tb = M._Table(cuda, rng, n, lay.get("overlap", lay["two"]), zero_state=True, with_sign=(n % 8 == 0))
    for t in (1, 2, 3, 4, 1000, 20000):
        _go_and_check(cuda, [tb], M.TRAINER_DECAY, 6e-3 * (0.5 + 0.1 * (t % 7)), t, rng, what="chained")
    # the products advanced on the device over consecutive seals, no re-seeding in between
    b1, b2, eps, wd = M.TRAINER_DECAY
    tb = M._Table(cuda, rng, n, [W, W], zero_state=True, with_sign=(n % 8 == 0))
    ver = _Verdict(cuda, b1, b2, 0)
    for t in (1, 2, 3, 4, 5):
        tb.draw(rng)
        sealed = ver.seal(4e-3 * t, eps, wd, [tb.clip] if tb.clip is not None else [])
        assert _guarded([tb], ver) == 0
        want = G.guarded_adam_step(sealed, tb.p, tb.m, tb.v, tb.pieces, n, b1, b2)
        ref = M.T.adam_step(tb.p, tb.m, tb.v, tb.pieces, n, 4e-3 * t, b1, b2, eps, wd, t)
        got_p, got_m, got_v = tb.P.get(), tb.M.get(), tb.V.get()
        for got, w_, what in ((got_m, want.m, "m"), (got_v, want.v, "v"), (got_p, want.p, "p")):
            M._assert_bits(got, w_, f"running products, step {t}: {what}")
        M._assert_bits(got_m, ref.m, "m against pow")
        M._assert_bits(got_v, ref.v, "v against pow")
        assert int(_ulps(got_p, ref.p).max()) <= 1
        assert float(tb.step.get()[0]) == t
        tb.p, tb.m, tb.v = got_p, got_m, got_v


@pytest.mark.parametrize("sizes", M.SEVERAL[:3] + [(3 * 4096 + 4, 8, 4096 + 8, 4096)], ids=lambda s: "-".join(map(str, s)))
def test_go_several_tables_in_one_call(cuda, sizes):
    rng = np.random.default_rng(sum(sizes))
    tables = []
    for k, n in enumerate(sizes):
        lay = list(M._layouts(n).values())
        slots = [[W, W, W, W], [W], lay[-1], [W, W]][k]
        tables.append(M._Table(cuda, rng, n, slots, with_step=(k % 2 == 0), with_sign=(n % 8 == 0 and k != 2), zero_state=True))
    for t, scale in ((1, None), (2, THIRD if all(tb.slots[0] is not None for tb in tables) else None), (3, None)):
        _go_and_check(cuda, tables, M.TRAINER_DECAY, 4e-3 * t, t, rng, scale=scale, what=str(sizes))


@pytest.mark.parametrize("reasons", [G.NONFINITE, G.RANGE_GUARD, G.NONFINITE | G.RANGE_GUARD])
@pytest.mark.parametrize("sizes", [(8,), (4096 + 8,), (4099,), (3 * 4096 + 4, 8, 4096 + 8, 4096), (4096, 7)],
                         ids=lambda s: "-".join(map(str, s)))
def test_skip_leaves_every_bit(cuda, sizes, reasons):
    rng = np.random.default_rng(sum(sizes) + reasons)
    tables = []
    for k, n in enumerate(sizes):
        lay = M._layouts(n)
        tables.append(M._Table(cuda, rng, n, lay.get("overlap", lay["two"]), with_step=True, with_sign=(n % 8 == 0)))
        tables[-1].draw(rng)
        if k == 0:
            tables[0].pieces[0][0][0] = np.nan                    # the gradient IS bad, and must not arrive anywhere
            tables[0].G[0] = Guarded(tables[0].pieces[0][0], cuda)
    b1, b2, eps, wd = M.TRAINER_DECAY
    ver = _Verdict(cuda, b1, b2, 5)
    ver.seal(6e-3, eps, wd, [tb.clip for tb in tables if tb.clip is not None])          # a go-step first: scalars in place,
    for tb in tables:                                                                    # counters zeroed ...
        if tb.clip is not None:
            tb.clip.tensor().fill_(5)                                                    # ... and loaded again
    ver.poison(reasons)
    everything = [b for tb in tables for b in tb.guards()]
    snaps = [b.snapshot() for b in everything]
    sealed = ver.seal(6e-3, eps, wd, [tb.clip for tb in tables if tb.clip is not None])
    assert sealed.skip == reasons and sealed.skipped == 1 and ver.found.get().view(u32)[0] == 0x3f800000
    for scale in (None, THIRD):
        assert _guarded(tables, ver, scale) == 0
        assert all(b.unchanged_since(s) for b, s in zip(everything, snaps)), f"a skipped step wrote something (scale {scale})"
    for tb in tables:
        assert float(tb.step.get()[0]) == 0.0 and (tb.clip is None or int(tb.clip.get()[0]) == 5)
        assert G.guarded_adam_step(sealed, tb.p, tb.m, tb.v, tb.pieces, tb.n, b1, b2) is None


def test_refusals_and_the_wrapper(cuda):
    """No verdict, a misaligned one, and cnc_table_adam's own refusals: CNC_ERR_INVALID_VALUE with every buffer untouched;
    `TableAdam.step(guard=...)` goes through the entry, leaves the counters to the seal and counts attempts."""
    from cnc_amd._step_guard import StepGuard
    from cnc_amd._table_adam import TableAdam
    rng = np.random.default_rng(5)
    tb = M._Table(cuda, rng, 4100, [W])
    tb.draw(rng)
    ver = _Verdict(cuda, 0.9, 0.999, 0)
    ver.seal(6e-3, 1e-15, 0.0)
    snaps = [b.snapshot() for b in tb.guards()]
    lib = M._L().lib()
    a = M._struct([tb])
    assert lib.cnc_table_adam_guarded(C.byref(a), None, None, _stream()) == M.INVALID
    assert lib.cnc_table_adam_guarded(C.byref(a), None, ver.buf.ptr + 4, _stream()) == M.INVALID
    assert lib.cnc_table_adam_guarded(None, None, ver.buf.ptr, _stream()) == M.INVALID
    a.table[0].g_lo[0] = 6
    assert lib.cnc_table_adam_guarded(C.byref(a), None, ver.buf.ptr, _stream()) == M.INVALID
    bad = (C.c_float * 4)(0.0, 1.0, 1.0, 1.0)
    assert lib.cnc_table_adam_guarded(C.byref(M._struct([tb])), bad, ver.buf.ptr, _stream()) == M.INVALID
    torch.cuda.synchronize()
    assert all(b.unchanged_since(s) for b, s in zip(tb.guards(), snaps))
    # through the wrapper: a go-step, a skipped step, a go-step
    n = 8200
    p0 = M._signed(rng, n, -4, 0)
    tab = torch.nn.Parameter(torch.tensor(p0, device=cuda).view(-1, 8))
    opt = M._optimizer([tab], cuda, weight_decay=2e-6)
    ta = TableAdam(opt, [tab])
    guard = StepGuard(cuda, 0.9, 0.999, 0)
    twin = G.seeded(0.9, 0.999, 0)
    p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    dev = lambda x: torch.tensor(x, device=cuda).view(-1, 8)
    for k, poisoned in enumerate((False, True, False)):
        g = M._grad(rng, n)
        small = torch.ones(5, device=cuda)
        if poisoned:
            small[2] = float("inf")
        guard.scan([small])
        guard.seal(6e-3, 1e-15, 2e-6, ta.clip_counters())
        twin, _ = G.scan(twin, [small.cpu().numpy()])
        twin, _, _ = G.seal(twin, 6e-3, 0.9, 0.999, 1e-15, 2e-6)
        ta.step({id(tab): [(dev(g), None)]}, guard=guard)
        torch.cuda.synchronize()
        want = G.guarded_adam_step(twin, p, m, v, [(g, 0, n)], n, 0.9, 0.999)
        if want is not None:
            p, m, v = want.p, want.m, want.v
        st = opt.state[tab]
        M._assert_bits(M._host(tab), p, "p")
        M._assert_bits(M._host(st["exp_avg"]), m, "m")
        M._assert_bits(M._host(st["exp_avg_sq"]), v, "v")
        assert ta.steps_done == k + 1                                  # attempts
    assert float(opt.state[tab]["step"]) == 2.0 and guard.stats() == {"skipped": 1, "reasons": G.NONFINITE}
    ta.resync()
    assert ta.steps_done == 2                                          # the device's count
