"""The device entropy coder (cnc_amd/csrc/rans_coder.hip): the C ABI on sentinel-guarded buffers against the NumPy
restatement of the "rans1" format (tests/rans_twin.py) and the host twin in libcnc_codec.so; then `coder="device"`
through the context model, the container and the Trainer against the host range coder's path."""
import os

import numpy as np
import pytest
import torch

import rans_twin as tw
from guarded import FILL, Guarded
from test_gpu_context import setup  # noqa: F401  (the toy context model, tables and occupancy grid of that module)
from test_gpu_trainer import _cfg
from test_rans_twin import DAMAGE, damaged_table, extreme, twin_verdict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs(cuda):
    from cnc_amd import _codec, _lib
    return _lib, _lib.lib(), _codec.lib()


class Table:
    """A table of streams on guarded buffers: p, x, bytes per stream, sizes / status for the call."""

    def __init__(self, dev, specs, caps=None, shifts=(1, 3)):
        """specs: [(p float32 [n] or [1], x float32 [n], S)]; the byte buffers are shifted by 1 and 3 bytes in turn."""
        self.dev, self.specs = dev, specs
        self.p = [Guarded(np.asarray(p, np.float32).reshape(-1), dev) for p, _, _ in specs]
        self.x = [Guarded(np.asarray(x, np.float32).reshape(-1), dev) for _, x, _ in specs]
        self.caps = [tw.bound(len(x), S) + 7 for _, x, S in specs] if caps is None else caps
        self.bytes = [Guarded.empty((cap,), np.uint8, dev, shift=shifts[k % len(shifts)]) for k, cap in enumerate(self.caps)]

    def table(self, _lib, x=None, lens=None):
        t = (_lib.RansStream * len(self.specs))()
        for k, (p, xs, S) in enumerate(self.specs):
            n = len(xs)
            stride = 0 if (np.size(p) == 1 and n != 1) else 1
            t[k] = _lib.RansStream(self.p[k].ptr, stride, (self.x if x is None else x)[k].ptr, n, S, self.bytes[k].ptr,
                                   self.caps[k] if lens is None else lens[k])
        return t

    def encode(self, libs):
        _lib, L, _ = libs
        t = self.table(_lib)
        need = L.cnc_rans_scratch_bytes(t, len(t))
        scratch = Guarded.empty((max(int(need), 16),), np.uint8, self.dev)
        sizes = Guarded(np.full(2 * len(t), -7, np.int32), self.dev)          # int64 [n_streams] as pairs of words
        _lib.check(L.cnc_rans_encode_pm1(t, len(t), scratch.ptr, int(need), sizes.ptr, _lib.stream(self.dev)), "rans encode")
        torch.cuda.synchronize()
        assert scratch.intact() and sizes.intact()
        for g in self.p + self.x + self.bytes:
            assert g.intact()
        return sizes.get().view(np.int64)

    def decode(self, libs, lens):
        """Decodes `bytes` into fresh guarded buffers: (status [n_streams], [x per stream])."""
        _lib, L, _ = libs
        out = [Guarded.empty((len(x),), np.float32, self.dev) for _, x, _ in self.specs]
        status = Guarded(np.full(len(self.specs), 5, np.int32), self.dev)
        t = self.table(_lib, x=out, lens=lens)
        _lib.check(L.cnc_rans_decode_pm1(t, len(t), status.ptr, _lib.stream(self.dev)), "rans decode")
        torch.cuda.synchronize()
        assert status.intact()
        for g in self.p + out + self.bytes:
            assert g.intact()
        return status.get(), [o.get() for o in out]


def draw(rng, p, n):
    return np.where(rng.uniform(size=n) < np.broadcast_to(p, (n,)), 1.0, -1.0).astype(np.float32)


def abi_specs():
    rng = np.random.default_rng(5)
    specs = []
    for n in (64, 1, 63, 0, 65, 1023, 1024, 1025):          # K = 64 +- 1 lanes at S = 16, an empty stream in the middle
        p = rng.uniform(1e-6, 1 - 1e-6, size=n).astype(np.float32)
        specs.append((p, draw(rng, p, n), 16))
    p = np.array([0.83], np.float32)                          # p_stride = 0
    specs.append((p, draw(rng, p, 777), 16))
    p = rng.uniform(0.01, 0.99, size=5000).astype(np.float32)  # more than one symbol per lane step, S not dividing n
    specs.append((p, draw(rng, p, 5000), 37))
    ext = np.resize(np.array([1e-6, 1 - 1e-6, 1e-6, 1 - 1e-6, 0.5], np.float32), 1029)
    specs.append((ext, np.resize(np.array([1, -1, -1, 1, 1], np.float32), 1029), 16))
    # 30 streams make two launches of the table (24 per launch)
    for k in range(19):
        n = 40 + 13 * k
        p = rng.uniform(0.05, 0.95, size=n).astype(np.float32)
        specs.append((p, draw(rng, p, n), 1 + k))
    return specs


def test_abi_encode_decode_equal_the_twin(cuda, libs):
    specs = abi_specs()
    assert len(specs) == 30
    want = [tw.encode(p, x, S) for p, x, S in specs]
    tab = Table(cuda, specs)
    sizes = tab.encode(libs)
    assert sizes.tolist() == [len(w) for w in want]
    for k, w in enumerate(want):
        got = tab.bytes[k].get()
        assert got[:len(w)].tobytes() == w, k
        assert np.all(got[len(w):] == FILL), k                 # nothing behind the reported size
    status, xs = tab.decode(libs, [len(w) for w in want])
    assert not status.any()
    for k, (_, x, _) in enumerate(specs):
        assert np.array_equal(xs[k], x), k


def test_cross_decoding_between_host_and_device(cuda, libs):
    _lib, L, Lc = libs
    specs = abi_specs()[:12]
    tab = Table(cuda, specs)
    sizes = tab.encode(libs)
    host = []
    for k, (p, x, S) in enumerate(specs):
        n = len(x)
        stream = np.ascontiguousarray(tab.bytes[k].get()[:sizes[k]])
        # device-encoded -> the host twin
        assert Lc.cnc_rans_check(stream.ctypes.data, stream.size, n) == tw.lanes(n, S)
        out = np.zeros(max(n, 1), np.float32)
        pp = np.ascontiguousarray(p, np.float32)
        stride = 0 if (pp.size == 1 and n != 1) else 1
        assert Lc.cnc_rans_decode_pm1_host(pp.ctypes.data, stride, n, stream.ctypes.data, stream.size, out.ctypes.data) == 0
        assert np.array_equal(out[:n], x)
        # host-encoded, at another lane count -> the device
        S2 = 3 * S + 1
        buf = np.zeros(tw.bound(n, S2), np.uint8)
        xx = np.ascontiguousarray(x, np.float32)
        got = Lc.cnc_rans_encode_pm1_host(pp.ctypes.data, stride, xx.ctypes.data, n, S2, buf.ctypes.data, buf.size)
        assert got == len(tw.encode(p, x, S2))
        host.append(buf[:got])
    for k, h in enumerate(host):
        assert len(h) <= tab.caps[k]
        tab.bytes[k] = Guarded(np.concatenate([h, np.full(tab.caps[k] - len(h), FILL, np.uint8)]), cuda, shift=(3, 1)[k % 2])
    status, xs = tab.decode(libs, [len(h) for h in host])
    assert not status.any()
    for k, (_, x, _) in enumerate(specs):
        assert np.array_equal(xs[k], x), k


def test_worst_case_stream_and_short_cap(cuda, libs):
    n, S = 1025, 16
    p = np.full(n, 1.0, np.float32)                           # every symbol -1 at P(-1) = 1 / 2^16: two bytes each
    x = -np.ones(n, np.float32)
    want = tw.encode(p, x, S)
    assert len(want) == tw.bound(n, S)
    rng = np.random.default_rng(2)
    q = rng.uniform(0.1, 0.9, size=300).astype(np.float32)
    other = (q, draw(rng, q, 300), 16)
    tab = Table(cuda, [(p, x, S), other, (p, x, S), (p, x, S)],
                caps=[len(want), tw.bound(300, 16), len(want) - 1, 100])
    sizes = tab.encode(libs)
    assert sizes.tolist() == [len(want), len(tw.encode(*other)), -1, -1]
    assert tab.bytes[0].get().tobytes() == want
    for k in (2, 3):                                           # too small: nothing written, inside cap or past it
        assert np.all(tab.bytes[k].get() == FILL)


def test_malformed_streams_are_refused_on_the_host_before_any_launch(cuda, libs, tmp_path):
    """`DeviceCoder.decode_group` runs cnc_rans_check on every file before it uploads anything: a truncated file, a
    directory that does not fit and K > n raise, and no kernel runs (the outputs are never allocated)."""
    from cnc_amd.context import DeviceCoder
    rng = np.random.default_rng(9)
    n = 1029
    p = rng.uniform(0.02, 0.98, size=n).astype(np.float32)
    good = bytearray(tw.encode(p, draw(rng, p, n), 16))
    K, w = tw.lanes(n, 16), tw.dir_width(n, tw.lanes(n, 16))
    bad = {"truncated": bytes(good[:-5])}
    b = bytearray(good)
    b[6 + 3 * w] = 0xFF
    bad["directory"] = bytes(b)
    b = bytearray(good)
    b[2:6] = (n + 1).to_bytes(4, "little")
    bad["lanes"] = bytes(b)
    pd = torch.from_numpy(p).to(cuda)
    ok = str(tmp_path / "ok.b")
    open(ok, "wb").write(bytes(good))
    coder = DeviceCoder()
    launched = []
    real = coder._launch_decode
    coder._launch_decode = lambda *a, **k: (launched.append(1), real(*a, **k))[1]
    for name, data in bad.items():
        f = str(tmp_path / f"{name}.b")
        open(f, "wb").write(data)
        with pytest.raises(RuntimeError, match="not a valid rans1 stream"):
            coder.decode_group([(pd, ok), (pd, f)])
    assert not launched
    out = coder.decode_group([(pd, ok)])
    assert launched == [1] and out[0].shape == (n,)


def _encode_equals(tab, libs, want):
    """One encode call of the table: sizes, bytes and the fill behind them against the twin's streams."""
    sizes = tab.encode(libs)
    assert sizes.tolist() == [len(w) for w in want]
    for k, w in enumerate(want):
        got = tab.bytes[k].get()
        assert got[:len(w)].tobytes() == w, k
        assert np.all(got[len(w):] == FILL), k                 # nothing behind the reported size
    return sizes


def _decode_equals(tab, libs, lens):
    status, xs = tab.decode(libs, lens)
    assert not status.any()
    for k, (_, x, _) in enumerate(tab.specs):
        assert np.array_equal(xs[k], x), k


def _put(tab, k, data, shift):
    """Stream k's byte buffer holds `data` (shorter than its capacity: the rest is the fill)."""
    assert len(data) <= tab.caps[k]
    rest = np.full(tab.caps[k] - len(data), FILL, np.uint8)
    tab.bytes[k] = Guarded(np.concatenate([np.frombuffer(bytes(data), np.uint8), rest]), tab.dev, shift=shift)


@pytest.fixture(scope="module")
def production():
    """name -> (p, x, S) at the lane shapes of a full-size container, and the twin's stream of each (made once)."""
    rng = np.random.default_rng(16384)

    def uniform(n):
        p = rng.uniform(1e-6, 1 - 1e-6, size=n).astype(np.float32)
        return p, draw(rng, p, n)
    specs = {"a": uniform(1000003) + (16384,)}                 # K = 62 lanes of 16129 / 16130 symbols, w = 2
    specs["j"] = (np.zeros(0, np.float32), np.zeros(0, np.float32), 16384)      # empty, between two large streams
    one = np.array([0.97], np.float32)
    specs["b"] = (one, draw(rng, one, 200000), 16384)          # p_stride = 0: long lanes, tiny output
    specs["c"] = extreme(100000) + (16384,)
    specs["d"] = uniform(3 * 32768) + (32768,)                 # w = 3
    specs["e"] = uniform(3 * 32767) + (32767,)                 # w = 2, the other side of that boundary
    specs["f"] = uniform(313 * 128) + (128,)                   # w = 2 and K > 256: the strided directory loops of the pack
    specs["g"] = uniform(313 * 127) + (127,)                   # w = 1 and K > 256
    p, x = uniform(16454)                                      # K = 16454 > 256 * 64: the decoder's second round of groups
    p[-70:], x[-70:] = extreme(70)                             # ... whose lanes emit bytes: improbable symbols among them
    specs["h"] = (p, x, 1)
    specs["i"] = uniform(5000) + (16,)                         # K = 313, w = 1
    want = {k: tw.encode(*v) for k, v in specs.items()}
    widths = {k: w[1] for k, w in want.items()}
    assert widths == dict(a=2, j=1, b=2, c=2, d=3, e=2, f=2, g=1, h=1, i=1)
    lanes = {k: int.from_bytes(w[2:6], "little") for k, w in want.items()}
    assert lanes == dict(a=62, j=0, b=13, c=7, d=3, e=3, f=313, g=313, h=16454, i=313)
    return specs, want


def test_production_lane_shapes_equal_the_twin(cuda, libs, production):
    """The default lane length (16384 symbols, a two-byte directory), both directory width boundaries, more lanes than
    one pack block sums in one pass (256) and than one decode launch holds (256 blocks of 64), in one encode and one
    decode call; then stream a across the host twin and the device, at another lane count."""
    _lib, L, Lc = libs
    specs, want = production
    names = list(specs)
    assert names[:3] == ["a", "j", "b"]
    tab = Table(cuda, [specs[k] for k in names])
    _encode_equals(tab, libs, [want[k] for k in names])
    _decode_equals(tab, libs, [len(want[k]) for k in names])
    # stream a: device-encoded -> the host twin
    p, x, S = specs["a"]
    n = len(x)
    stream = np.ascontiguousarray(tab.bytes[0].get()[:len(want["a"])])
    assert Lc.cnc_rans_check(stream.ctypes.data, stream.size, n) == tw.lanes(n, S)
    out = np.zeros(n, np.float32)
    assert Lc.cnc_rans_decode_pm1_host(p.ctypes.data, 1, n, stream.ctypes.data, stream.size, out.ctypes.data) == 0
    assert np.array_equal(out, x)
    # host-encoded at S = 4096 -> the device: K comes from the header, the decoder's blocks from n
    buf = np.zeros(tw.bound(n, 4096), np.uint8)
    got = Lc.cnc_rans_encode_pm1_host(p.ctypes.data, 1, x.ctypes.data, n, 4096, buf.ctypes.data, buf.size)
    assert got > 0 and buf[1] == 2 and int.from_bytes(buf[2:6].tobytes(), "little") == tw.lanes(n, 4096) == 245
    other = Table(cuda, [(p, x, S)])
    _put(other, 0, buf[:got], 3)
    _decode_equals(other, libs, [got])


def test_a_damaged_lane_of_the_second_round_of_groups_is_refused(cuda, libs, production):
    """Stream h has 16454 lanes and the decoder 256 blocks of 64: lanes from 16384 on are reached only by a block's
    second turn.  One payload bit of such a lane flipped: that stream is refused, its neighbours are not."""
    specs, want = production
    names = ["i", "h", "g"]
    at, cnt = tw.lane_starts(want["h"])
    j = next(j for j in range(64 * 256, len(cnt)) if cnt[j] > 0)
    bad = bytearray(want["h"])
    bad[at[j] + 4] ^= 0x04
    p, x, _ = specs["h"]
    assert tw.check(bytes(bad), len(x)) == len(cnt) and tw.decode(p, len(x), bytes(bad))[0] == -3
    tab = Table(cuda, [specs[k] for k in names])
    data = [want["i"], bytes(bad), want["g"]]
    for k, d in enumerate(data):
        _put(tab, k, d, (1, 3)[k % 2])
    status, xs = tab.decode(libs, [len(d) for d in data])
    assert status.tolist() == [0, -3, 0]
    for k in (0, 2):
        assert np.array_equal(xs[k], specs[names[k]][1])
    _put(tab, 1, want["h"], 3)                                 # the sound stream again: the verdict was the bit's
    _decode_equals(tab, libs, [len(want[k]) for k in names])


def test_launches_that_begin_and_end_on_an_empty_stream(cuda, libs):
    """49 streams are two full launches of the table (24 each) and one more; streams 0, 23, 24 and 48 are empty, so each
    launch begins or ends on one.  Then the 24-stream prefix: a call that is exactly one launch."""
    rng = np.random.default_rng(49)
    specs = []
    for k in range(49):
        n = 0 if k in (0, 23, 24, 48) else 40 + 13 * k
        p = rng.uniform(0.05, 0.95, size=n).astype(np.float32)
        specs.append((p, draw(rng, p, n), 1 + k % 19))
    want = [tw.encode(p, x, S) for p, x, S in specs]
    for count in (49, 24):
        tab = Table(cuda, specs[:count])
        _encode_equals(tab, libs, want[:count])
        _decode_equals(tab, libs, [len(w) for w in want[:count]])


def test_damaged_streams_are_refused_by_the_device_and_only_they(cuda, libs):
    """Every way a stream can be damaged (test_rans_twin.DAMAGE) between sound streams, 27 streams in two launches: the
    status words are the twin's verdicts, whether the host check would have let the stream through or not, and every
    sound stream decodes exactly.  All streams are small (n <= 1100, S = 16: at most 69 lanes of a few bytes, w = 1) and
    lie in guarded buffers, so no address the decoder can form from a damaged directory leaves the allocation."""
    _lib, L, Lc = libs
    table = damaged_table()
    assert len(table) >= 8 and table[0][0] is None and table[-1][0] is None
    verdict = []
    for name, p, x, buf, length in table:                      # on the CPU first: what the twin and the host check say
        passes, status, _ = twin_verdict(p, len(x), buf, length)
        assert (passes, status) == ((True, 0) if name is None else DAMAGE[name]), name
        s = np.frombuffer(buf, np.uint8).copy()
        assert (Lc.cnc_rans_check(s.ctypes.data, length, len(x)) >= 0) == passes, name
        assert len(x) <= 1100 and buf[1] in (0, 1, 5) and len(buf) < 2 * 1100 + 6 + 5 * 69 + 8
        verdict.append(status)
    assert sorted(set(verdict)) == [-3, 0] and verdict.count(-3) == len(DAMAGE) - 1
    tab = Table(cuda, [(p, x, 16) for _, p, x, _, _ in table], caps=[len(buf) + 7 for _, _, _, buf, _ in table])
    for k, (_, _, _, buf, _) in enumerate(table):
        _put(tab, k, buf, (1, 3)[k % 2])
    status, xs = tab.decode(libs, [length for _, _, _, _, length in table])       # asserts every guard
    assert status.tolist() == verdict
    for k, (name, _, x, _, _) in enumerate(table):
        if verdict[k] == 0:
            assert np.array_equal(xs[k], x), (k, name)


def test_device_coder_at_its_default_lane_length_and_check(cuda, tmp_path):
    """`DeviceCoder()` as the Trainer uses it: 16384 symbols per lane, files byte-equal to the twin's streams, and a
    damaged file that passes the host check is named by `check()`, once."""
    from cnc_amd.context import DEVICE_CODER_SYMBOLS_PER_LANE, DeviceCoder
    assert DEVICE_CODER_SYMBOLS_PER_LANE == 16384
    rng = np.random.default_rng(20)
    n = 1 << 20
    ps = [rng.uniform(1e-6, 1 - 1e-6, size=n).astype(np.float32), np.array([0.9], np.float32),
          rng.uniform(0.3, 0.7, size=n).astype(np.float32)]
    xs = [draw(rng, p, n) for p in ps]
    want = [tw.encode(p, x, 16384) for p, x in zip(ps, xs)]
    files = [str(tmp_path / f"stream{k}.b") for k in range(3)]
    pd = [torch.from_numpy(p).to(cuda) for p in ps]
    pd[1] = pd[1].expand(n)                                    # an expanded scalar: read with stride 0
    coder = DeviceCoder()
    for p, x, f in zip(pd, xs, files):
        coder.encode(torch.from_numpy(x).to(cuda), p, f)
    assert coder.finish() == 8 * sum(len(w) for w in want)
    for f, w in zip(files, want):
        assert open(f, "rb").read() == w, f
    items = list(zip(pd, files))
    for got, x in zip(coder.decode_group(items), xs):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), x)
    coder.check()
    at, cnt = tw.lane_starts(want[1])
    j = len(cnt) // 2
    bad = bytearray(want[1])
    bad[at[j] + 4 + cnt[j] // 2] ^= 0x20
    assert cnt[j] > 0 and tw.check(bytes(bad), n) == len(cnt)
    open(files[1], "wb").write(bytes(bad))
    outs = coder.decode_group(items)                           # the file passes the host check: no error here
    with pytest.raises(RuntimeError, match="damaged stream") as err:
        coder.check()
    assert files[1] in str(err.value) and files[0] not in str(err.value) and files[2] not in str(err.value)
    for k in (0, 2):                                           # its neighbours in the same launch are whole
        assert np.array_equal(outs[k].cpu().numpy(), xs[k])
    coder.check()                                              # reported once


def _format_overhead_bits(directory, n_features):
    """40 bits per lane + directory + header of every rans1 file in `directory`."""
    total = 0
    for f in os.listdir(directory):
        if f.endswith(".b"):
            blob = open(os.path.join(directory, f), "rb").read()
            assert blob[0] == tw.FORMAT_ID
            w, K = blob[1], int.from_bytes(blob[2:6], "little")
            total += 40 * K + 8 * (6 + K * w)
    return total


@pytest.mark.parametrize("S", [None, 64])
def test_context_model_device_coder_equals_the_host_path(setup, tmp_path, S):
    g, m, encs, binary = setup
    args = (encs["xyz"], encs["xy"], encs["xz"], encs["yz"])
    out, sizes, Pgs = {}, {}, {}
    for coder in ("host", "device"):
        d = tmp_path / coder
        d.mkdir()
        with torch.no_grad():
            Pgs[coder], est, coded = m.encode_binary_vxl_mixPg_3D2D(*args, binary, filename_prefix=str(d / "b"), coder=coder,
                                                                    symbols_per_lane=S)
        files = sorted(f for f in os.listdir(d) if f.endswith(".b"))
        sizes[coder] = sum(os.path.getsize(d / f) for f in files)
        assert files == list(g["enc_files"])
        assert abs(coded * 1024 * 1024 - sizes[coder]) < 1e-6
        recs = [torch.ones_like(encs[n].params.data) for n in ("xyz", "xy", "xz", "yz")]
        out[coder] = m.decode_binary_vxl_mixPg_3D2D(*args, *recs, binary, Pgs[coder], filename_prefix=str(d / "b"), coder=coder)
    for a, b in zip(out["host"], out["device"]):
        assert a.is_cuda and b.is_cuda and torch.equal(a, b)
    for name, t in zip(("xyz", "xy", "xz", "yz"), out["device"]):
        assert np.array_equal(t.cpu().numpy().astype(np.int8), g[f"dec_{name}"]), name
    lanes = sum(int.from_bytes(open(tmp_path / "device" / f, "rb").read()[2:6], "little")
                for f in os.listdir(tmp_path / "device"))
    assert lanes > len(g["enc_files"]) if S == 64 else lanes >= 1
    print(f"S={S}: host {sizes['host']} B, device {sizes['device']} B, {lanes} lanes")
    assert 8 * sizes["device"] <= 8 * sizes["host"] + _format_overhead_bits(tmp_path / "device", m.n_features)
    # a file of the other coder is refused, not decoded into noise
    recs = [torch.ones_like(encs[n].params.data) for n in ("xyz", "xy", "xz", "yz")]
    with pytest.raises(RuntimeError, match="not a valid rans1 stream"):
        m.decode_binary_vxl_mixPg_3D2D(*args, *recs, binary, Pgs["host"], filename_prefix=str(tmp_path / "host" / "b"),
                                       coder="device")


def test_container_and_trainer_with_the_device_coder(cuda, tmp_path, monkeypatch):
    from cnc_amd.container import read_container
    from cnc_amd.trainer import Trainer
    monkeypatch.delenv("CNC_DEVICE_CODER", raising=False)
    a = Trainer(_cfg(tmp_path), device=cuda)
    a.train(steps=120, log=None)
    psnr_a = a.evaluate()
    assert a.coder_name() == "host"
    host_info = a.save_container(str(tmp_path / "host.cnc"))
    monkeypatch.setenv("CNC_DEVICE_CODER", "1")
    assert a.coder_name() == "device"
    monkeypatch.delenv("CNC_DEVICE_CODER")
    a.cfg.device_coder = True
    a.cfg.symbols_per_lane = 256
    dev_info = a.save_container(str(tmp_path / "dev.cnc"))
    assert "coder" not in read_container(str(tmp_path / "host.cnc"), device=cuda)[0]
    meta, streams = read_container(str(tmp_path / "dev.cnc"), device=cuda)[:2]
    assert meta["coder"] == "rans1" and all(b[0] == tw.FORMAT_ID for b in streams.values())
    lanes = sum(int.from_bytes(b[2:6], "little") for b in streams.values())
    width = sum(int.from_bytes(b[2:6], "little") * b[1] for b in streams.values())
    assert 8 * 1024 * dev_info["embeddings_KB"] <= 8 * 1024 * host_info["embeddings_KB"] + 40 * lanes + 8 * (6 * len(streams) + width) + 1e-6
    b = Trainer(_cfg(tmp_path, seed=7), device=cuda)          # a fresh Trainer with the HOST coder configured: the file says
    assert b.coder_name() == "host"
    assert abs(b.evaluate() - psnr_a) > 3.0
    b.load_container(str(tmp_path / "dev.cnc"))
    tables = lambda t: [e.params.data.clone() for e in (t.field.mlp_base.encoding_xyz, t.field.mlp_base.encoding_xy,
                                                        t.field.mlp_base.encoding_xz, t.field.mlp_base.encoding_yz)]
    from_dev, psnr_dev = tables(b), b.evaluate()
    assert abs(psnr_dev - psnr_a) < 0.5, (psnr_a, psnr_dev)
    q = [torch.where(t >= 0, 1.0, -1.0) for t in tables(a)]
    for dec, want in zip(from_dev, q):
        coded = ~(dec == 1).all(dim=1)
        assert coded.any() and torch.equal(dec[coded], want[coded])
    b.load_container(str(tmp_path / "host.cnc"))               # a container of the host coder still loads
    for x, y in zip(from_dev, tables(b)):
        assert torch.equal(x, y)
    assert abs(b.evaluate() - psnr_dev) < 1e-3                 # the same tables, MLP and occupancy: the same views (to summation order)
