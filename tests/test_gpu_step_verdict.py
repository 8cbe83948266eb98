"""cnc_step_verdict_scan / cnc_step_verdict_seal (cnc_amd/csrc/step_verdict.hip) through the C ABI, against
tests/guarded_step_twin.py: which reasons a scan ORs into the verdict — one non-finite element at the places where the
kernel changes its load width, views at every 4-byte offset with non-finite neighbours on both sides, more tensors than one
call takes, null and empty entries, each clause of the range guard's predicate — and what the seal moves and leaves, bit
for bit.  Every buffer the kernels write lies inside a sentinel-filled allocation (tests/guarded.py)."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import guarded_step_twin as G
from guarded import Guarded

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
INVALID = -1
LENGTHS = [1, 3, 4, 63, 64, 65, 4097]
BAD = {"+inf": 0x7f800000, "-inf": 0xff800000, "quiet NaN": 0x7fc00000, "NaN with a payload": 0xffa5a5a5}
B1, B2 = 0.9, 0.999


def _L():
    from cnc_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Verdict:
    """A cnc_step_verdict_t on the device, inside a guarded allocation."""

    def __init__(self, dev, twin=None):
        L = _L()
        host = L.StepVerdict()
        twin = twin or G.Verdict()
        for name, _ in L.StepVerdict._fields_:
            setattr(host, name, getattr(twin, name))
        self.buf = Guarded(np.frombuffer(bytes(host), u32).copy(), dev)
        self.ptr = self.buf.ptr

    def raw(self):
        return self.buf.get().tobytes()

    def words(self):
        return list(struct.unpack("4I", self.raw()[:16]))

    def doubles_bits(self):
        return list(struct.unpack("9Q", self.raw()[16:88]))

    def acc(self):
        return self.words()[0]


def _twin_bits(v):
    return [struct.unpack("Q", struct.pack("d", x))[0] for x in v.doubles()]


def _scan(verdict, entries=(), guard=None, seen=0, pack_id=0, poison=None):
    """entries: (device address or None, element count)."""
    L = _L()
    a = L.VerdictScan()
    a.n_tensors = len(entries)
    for k, (p, n) in enumerate(entries):
        a.ptr[k], a.n[k] = p, n
    a.verdict = verdict.ptr
    a.guard, a.guard_seen, a.pack_id = (guard.ptr if guard is not None else None), seen, pack_id
    a.poison = poison.ptr if poison is not None else None
    rc = L.lib().cnc_step_verdict_scan(C.byref(a), _stream())
    torch.cuda.synchronize()
    return rc


def _clean(rng, n):
    """Finite values that press on the test's edges: the largest finite floats, denormals, both zeros."""
    x = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 30, n)).astype(f32)
    special = np.array([0x7f7fffff, 0xff7fffff, 0x00000001, 0x807fffff, 0x80000000, 0x00000000, 0x7f000000], u32).view(f32)
    x[rng.integers(0, n, min(n, 7))] = special[:min(n, 7)]
    return x


# k_verdict_scan's grid is capped at kScanMaxBlocks = 64 blocks of 256 lanes, one uint4 a lane: 65536 elements a pass, the
# lanes going on `i += stride`.  4097 elements take two blocks; 300003 take the 64 and five passes (on the MI355X every bad
# word is found at each of the five places behind the first pass, and the clean array gives go)
ABOVE_THE_GRID_CAP = 300003
PASS = 64 * 256 * 4


def _places(n):
    """First, last, either side of every 16-byte boundary the length reaches at its start, and of the last one.  Above the
    grid's cap only the places behind the first grid-wide pass: the second element of each later pass, and the last."""
    if n == ABOVE_THE_GRID_CAP:
        return [PASS * k + 1 for k in range(1, 5)] + [n - 1]
    last4 = 4 * ((n - 1) // 4)
    return sorted({i for i in (0, n - 1, 3, 4, last4 - 1, last4, n // 2) if 0 <= i < n})


@pytest.mark.parametrize("n", LENGTHS + [ABOVE_THE_GRID_CAP])
def test_one_non_finite_element_anywhere_is_found(cuda, n):
    rng = np.random.default_rng(n)
    v = _Verdict(cuda)
    base = _clean(rng, n)
    t = Guarded(base, cuda)
    assert _scan(v, [(t.ptr, n)]) == 0 and v.acc() == 0, "FLT_MAX, denormals and -0 alone give go"
    before = v.buf.snapshot()
    for name, word in BAD.items():
        for i in _places(n):
            x = base.copy()
            x.view(u32)[i] = word
            t = Guarded(x, cuda)
            fresh = _Verdict(cuda)
            assert _scan(fresh, [(t.ptr, n)]) == 0
            assert fresh.words() == [G.NONFINITE, 0, 0, 0], (name, i)
            assert fresh.buf.intact() and t.intact()
    assert v.buf.unchanged_since(before)


@pytest.mark.parametrize("offset", [1, 2, 3, 5])
def test_views_at_odd_offsets_see_their_own_elements_only(cuda, offset):
    """A window of finite values inside an array that is NaN everywhere else: the scan of the window — its pointer 4, 8 or 12
    bytes off a 16-byte boundary — gives go at every length; one bad element at the window's first or last place, skip."""
    rng = np.random.default_rng(offset)
    for n in LENGTHS:
        arr = np.full(offset + n + 7, np.nan, f32)
        arr[offset:offset + n] = _clean(rng, n)
        t = Guarded(arr, cuda)
        v = _Verdict(cuda)
        assert _scan(v, [(t.ptr + 4 * offset, n)]) == 0
        assert v.words() == [0, 0, 0, 0], (offset, n)
        for i in {0, n - 1, min(n - 1, 4 - offset % 4), max(0, n - 1 - (offset + n) % 4)}:
            bad = arr.copy()
            bad[offset + i] = np.inf
            tb = Guarded(bad, cuda)
            assert _scan(v, [(tb.ptr + 4 * offset, n)]) == 0
            assert v.acc() == G.NONFINITE, (offset, n, i)
            v = _Verdict(cuda)
    # the same through Guarded's own shift: an allocation-relative misalignment, the bad element in the tail
    x = _clean(rng, 66)
    x[65] = -np.inf
    t = Guarded(x, cuda, shift=4 * (offset % 4))
    v = _Verdict(cuda)
    assert _scan(v, [(t.ptr, 65)]) == 0 and v.acc() == 0
    assert _scan(v, [(t.ptr, 66)]) == 0 and v.acc() == G.NONFINITE


def test_fifty_tensors_take_two_calls_that_accumulate(cuda):
    rng = np.random.default_rng(50)
    sizes = [int(s) for s in rng.choice(LENGTHS, 50)]
    hosts = [_clean(rng, s) for s in sizes]
    hosts[49].view(u32)[sizes[49] - 1] = BAD["quiet NaN"]                  # the last tensor of the list
    bufs = [Guarded(h, cuda, shift=4 * (k % 4)) for k, h in enumerate(hosts)]
    entries = [(b.ptr, s) for b, s in zip(bufs, sizes)]
    v = _Verdict(cuda)
    assert _scan(v, entries[:48]) == 0 and v.acc() == 0
    assert _scan(v, entries[48:]) == 0 and v.acc() == G.NONFINITE
    # the last tensor of a full call
    v = _Verdict(cuda)
    assert _scan(v, entries[2:50]) == 0 and v.acc() == G.NONFINITE
    # the accumulation word keeps what an earlier call left, and 49 tensors in one call are refused
    guard = Guarded(np.array([0, 0, 0, 4, 0, 0, 0, 0], u32), cuda)
    assert _scan(v, [], guard=guard, seen=1, pack_id=4) == 0 and v.acc() == G.NONFINITE | G.RANGE_GUARD
    L = _L()
    a = L.VerdictScan()
    a.n_tensors, a.verdict = 49, v.ptr
    assert L.lib().cnc_step_verdict_scan(C.byref(a), _stream()) == INVALID
    assert L.lib().cnc_step_verdict_scan(None, _stream()) == INVALID
    assert all(b.intact() for b in bufs) and v.buf.intact()


def test_null_and_empty_entries_are_passed_over(cuda):
    nan = Guarded(np.full(8, np.nan, f32), cuda)
    ok = Guarded(np.ones(9, f32), cuda)
    v = _Verdict(cuda)
    assert _scan(v, [(None, 100), (nan.ptr, 0), (ok.ptr, 9), (None, 0)]) == 0 and v.words() == [0, 0, 0, 0]
    assert _scan(v, []) == 0 and v.words() == [0, 0, 0, 0]
    assert _scan(v, [(ok.ptr, 9), (None, 5), (nan.ptr, 1)]) == 0 and v.acc() == G.NONFINITE
    assert _scan(_Verdict(cuda), [(ok.ptr + 2, 4)]) == INVALID              # not a float's address


GUARD_CASES = [("a saturated forward since `seen`", [9, 0, 0, 0, 0, 0], 9, 3, True),
               ("a later one", [12, 0, 0, 0, 0, 0], 9, 3, True),
               ("a stamp older than `seen`", [8, 0, 0, 0, 0, 0], 9, 3, False),
               ("no stamp", [0, 0, 0, 0, 0, 0], 0, 3, False),
               ("the first layer of this pack", [0, 3, 0, 0, 0, 0], 9, 3, True),
               ("the last layer of this pack", [0, 0, 0, 0, 0, 3], 9, 3, True),
               ("a layer of an older pack", [0, 2, 2, 2, 2, 2], 9, 3, False),
               ("words behind the guard's six", [0, 0, 0, 0, 0, 0, 3, 3], 9, 3, False),
               ("stamps beyond 2^31", [0xF0000000, 0, 0, 0, 0, 0], 0xE0000000, 3, True)]


@pytest.mark.parametrize("name,words,seen,pack_id,fires", GUARD_CASES, ids=[c[0] for c in GUARD_CASES])
def test_range_guard_predicate_and_poison(cuda, name, words, seen, pack_id, fires):
    assert G.guard_fired(words, seen, pack_id) == fires
    guard = Guarded(np.array((words + [0, 0])[:8], u32), cuda)
    poison = Guarded.empty((1,), np.float32, cuda)
    ok = Guarded(np.ones(70, f32), cuda)
    for entries in ([], [(ok.ptr, 70)]):                                   # guard-only form, and next to a tensor scan
        v = _Verdict(cuda)
        assert _scan(v, entries, guard=guard, seen=seen, pack_id=pack_id, poison=poison) == 0
        assert v.words() == [G.RANGE_GUARD if fires else 0, 0, 0, 0]
        got = poison.get().view(u32)[0]
        assert got == (0x7f800000 if fires else 0x00000000)                # +inf or +0, nothing else
        assert poison.intact() and guard.intact() and v.buf.intact()
    v = _Verdict(cuda)                                                     # without `poison`: the verdict alone
    assert _scan(v, [], guard=guard, seen=seen, pack_id=pack_id) == 0 and v.acc() == (G.RANGE_GUARD if fires else 0)


def _seal(verdict, found, lr, eps, wd, clips, b1=B1, b2=B2):
    L = _L()
    a = L.VerdictSeal()
    a.verdict, a.found_inf = verdict.ptr, found.ptr
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = lr, b1, b2, eps, wd
    for k, c in enumerate(clips):
        a.clip_count[k] = None if c is None else c.ptr
    rc = L.lib().cnc_step_verdict_seal(C.byref(a), _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("t0", [0, 7])
def test_seal_on_go_is_the_twin_bit_for_bit(cuda, t0):
    """Five consecutive go-steps with a moving learning rate: words, products and scalars equal the twin's, found_inf is
    exactly 0.0, the clip counters are zeroed (a null slot between them is passed over)."""
    twin = G.seeded(B1, B2, t0)
    v = _Verdict(cuda, twin)
    found = Guarded.empty((1,), np.float32, cuda)
    for k in range(5):
        clips = [Guarded(np.array([5 + k], u32), cuda), None, Guarded(np.array([0], u32), cuda), Guarded(np.array([77], u32), cuda)]
        lr, wd = 6e-3 * (0.01 + 0.2 * k), (2e-6 if k % 2 else 0.0)
        assert _seal(v, found, lr, 1e-15, wd, clips) == 0
        twin, f, _ = G.seal(twin, lr, B1, B2, 1e-15, wd)
        assert v.words() == [0, 0, 0, 0]
        assert v.doubles_bits() == _twin_bits(twin), (t0, k)
        assert found.get().view(u32)[0] == np.array([f], f32).view(u32)[0] == 0
        assert all(int(c.get()[0]) == 0 and c.intact() for c in clips if c is not None)
        assert v.buf.intact() and found.intact()
    if t0 == 0:
        assert twin.b1_pow == B1 ** 5 or abs(twin.b1_pow / B1 ** 5 - 1) <= 5 * 2.0 ** -52


def test_seal_on_skip_moves_only_its_counters(cuda):
    twin = G.seeded(B1, B2, 7)
    v = _Verdict(cuda, twin)
    found = Guarded.empty((1,), np.float32, cuda)
    clips = [Guarded(np.array([c], u32), cuda) for c in (5, 0, 9, 1)]
    assert _seal(v, found, 6e-3, 1e-15, 2e-6, clips) == 0                 # one go-step first: the scalars are in place
    twin, _, _ = G.seal(twin, 6e-3, B1, B2, 1e-15, 2e-6)
    for c, val in zip(clips, (5, 0, 9, 1)):
        c.tensor().fill_(val)
    reasons_so_far = 0
    for step, reasons in enumerate([G.NONFINITE, G.RANGE_GUARD, G.NONFINITE | G.RANGE_GUARD]):
        bad = Guarded(np.array([1.0, np.nan], f32), cuda)
        guard = Guarded(np.array([4, 0, 0, 0, 0, 0, 0, 0], u32), cuda)
        assert _scan(v, [(bad.ptr, 2)] if reasons & G.NONFINITE else [], guard=guard if reasons & G.RANGE_GUARD else None,
                     seen=2, pack_id=1) == 0
        assert v.acc() == reasons
        doubles, snaps = v.doubles_bits(), [c.snapshot() for c in clips]
        assert _seal(v, found, 3e-3, 1e-8, 0.5, clips) == 0               # other hyper-parameters: none may land
        reasons_so_far |= reasons
        assert v.words() == [0, reasons, step + 1, reasons_so_far]
        assert v.doubles_bits() == doubles == _twin_bits(twin)
        assert found.get().view(u32)[0] == 0x3f800000                      # exactly 1.0f
        assert all(c.unchanged_since(s) for c, s in zip(clips, snaps))
        assert v.buf.intact() and found.intact()
    # the accumulation word was cleared: the next seal goes ahead from the untouched products
    assert _seal(v, found, 3e-3, 1e-15, 0.0, clips) == 0
    twin, _, _ = G.seal(twin, 3e-3, B1, B2, 1e-15, 0.0)
    assert v.words() == [0, 0, 3, 3] and v.doubles_bits() == _twin_bits(twin)
    assert found.get().view(u32)[0] == 0 and all(int(c.get()[0]) == 0 for c in clips)


def test_seal_refusals(cuda):
    v = _Verdict(cuda)
    found = Guarded.empty((1,), np.float32, cuda)
    snap = v.buf.snapshot()
    L = _L()
    assert L.lib().cnc_step_verdict_seal(None, _stream()) == INVALID
    for b1, b2 in ((1.0, 0.999), (0.9, 1.5), (-0.1, 0.999), (float("nan"), 0.999)):
        assert _seal(v, found, 6e-3, 1e-15, 0.0, [], b1=b1, b2=b2) == INVALID
    a = L.VerdictSeal()
    a.beta1, a.beta2 = B1, B2
    assert L.lib().cnc_step_verdict_seal(C.byref(a), _stream()) == INVALID   # no verdict
    torch.cuda.synchronize()
    assert v.buf.unchanged_since(snap)


def test_step_guard_object(cuda):
    """cnc_amd._step_guard.StepGuard: tensors in chunks of 48, non-contiguous and empty ones, `stats`, the non-waiting `poll`
    and its single warning, `seed`."""
    import warnings
    from cnc_amd._step_guard import NONFINITE, RANGE_GUARD, StepGuard
    g = StepGuard(cuda, B1, B2, steps_taken=7)
    twin = G.seeded(B1, B2, 7)
    tensors = [torch.ones(k % 9 + 1, device=cuda) for k in range(60)] + [None, torch.zeros(0, device=cuda),
                                                                          torch.ones(6, 5, device=cuda).t()]
    for _ in range(2):
        g.scan(tensors)
        g.seal(6e-3, 1e-15, 2e-6)
        twin, _, _ = G.seal(twin, 6e-3, B1, B2, 1e-15, 2e-6)
    assert g.stats() == {"skipped": 0, "reasons": 0} and g.last_skip() == 0 and float(g.found_inf) == 0.0
    assert [struct.unpack("Q", struct.pack("d", x))[0] for x in g._buf[2:].tolist()] == _twin_bits(twin)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        torch.cuda.synchronize()
        assert g.poll() == {"skipped": 0, "reasons": 0}
    tensors[55][-1] = float("nan")                                            # in the second chunk
    g.scan(tensors)
    words = torch.tensor([3, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=cuda)
    g.scan((), range_guard=(words, 2, 9))
    g.seal(6e-3, 1e-15, 2e-6)
    assert g.stats() == {"skipped": 1, "reasons": NONFINITE | RANGE_GUARD} and float(g.found_inf) == 1.0
    torch.cuda.synchronize()
    with pytest.warns(UserWarning, match="skipped an optimizer update"):
        assert g.poll() == {"skipped": 1, "reasons": NONFINITE | RANGE_GUARD}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g.poll()                                                              # once
    assert [struct.unpack("Q", struct.pack("d", x))[0] for x in g._buf[2:].tolist()] == _twin_bits(twin)
    g.seed(0)
    assert g._buf[2:4].tolist() == [1.0, 1.0]
    with pytest.raises(RuntimeError):
        g.scan([torch.ones(3, device=cuda, dtype=torch.float64)])
