"""The entropy coders behind one call shape.

`encoder` / `decoder` are the reference's pair (examples/utils_bpp_acc.py:77-110) on the host range coder of
libcnc_codec.so.  `CoderPool` (the host range coder on worker threads) and `DeviceCoder` (the "rans1" coder on the GPU,
cnc_amd/csrc/rans_coder.hip) code many streams and share five methods, so a caller never asks which one it holds:

    encode(x, p, file_name)     hand over one stream of symbols x in {-1, +1} with P(x = +1) = p
    finish() -> bits            every stream handed over is in its .b file; their total size
    decode_group(items)         items: [(p, file_name)] that do not depend on each other -> their symbols as float32
                                +-1 tensors on p's device, in order
    check()                     raises if a stream decoded so far was damaged (the device coder's status words)
    shutdown()

`make_coder(kind)` builds one of the two.  The two kinds of file are not interchangeable.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from ._codec import lib as _codec_lib  # noqa: E402  (libcnc_codec.so, include/cnc_codec.h)


def _encode_host(x, p, file_name):
    """x, p: contiguous float32 HOST tensors.  Writes the .b file, returns its size in bits."""
    n = x.numel()
    L = _codec_lib()
    cap = int(L.cnc_rc_bound(n))
    buf = np.empty(cap, dtype=np.uint8)
    nbytes = L.cnc_rc_encode_pm1(p.data_ptr(), x.data_ptr(), n, buf.ctypes.data, cap)
    if nbytes < 0:
        raise RuntimeError("range coder: output buffer too small")
    with open(file_name, "wb") as fout:
        fout.write(buf[:nbytes].tobytes())
    return int(nbytes) * 8


def _decode_host(p, file_name):
    with open(file_name, "rb") as fin:
        stream = np.frombuffer(fin.read(), dtype=np.uint8)
    out = torch.empty(p.numel(), dtype=torch.float32)
    _codec_lib().cnc_rc_decode_pm1(p.data_ptr(), p.numel(), stream.ctypes.data, stream.shape[0], out.data_ptr())
    return out


def encoder(x, p, file_name):
    """Code x in {-1,+1} with P(x=+1)=p into `file_name` (.b); returns the size in bits
    (utils_bpp_acc.py:77-93)."""
    assert file_name[-2:] == ".b"
    x = x.detach().to(torch.float32).cpu().contiguous().view(-1)
    p = p.detach().to(torch.float32).cpu().contiguous().view(-1)
    return _encode_host(x, p, file_name)


def decoder(p, file_name):
    """Inverse of `encoder`: returns float32 ±1 on p's device (utils_bpp_acc.py:95-110)."""
    assert file_name[-2:] == ".b"
    dvc = p.device
    return _decode_host(p.detach().to(torch.float32).cpu().contiguous().view(-1), file_name).to(dvc)


class CoderPool:
    """The reference codes its 33 streams one after the other, each behind two blocking `.cpu()` copies
    (utils_bpp_acc.py:77-110, call sites :722-804).  The streams are independent files, so here they are
    coded CONCURRENTLY: `encode` / `decode` start a device->pinned-host copy on a side stream and hand the
    rest (wait for the copy, run the C coder — ctypes drops the GIL —, touch the file) to a worker thread;
    the GPU goes on computing the next stream's probabilities meanwhile.  Same bytes as `encoder` /
    `decoder` (tests/test_gpu_context.py).  At most `max_in_flight` streams hold pinned buffers at once."""

    def __init__(self, workers=None, max_in_flight=8):
        import concurrent.futures as cf
        import threading
        self.pool = cf.ThreadPoolExecutor(max_workers=workers or min(8, os.cpu_count() or 1))
        self.slots = threading.Semaphore(max_in_flight)
        self.copy_stream = {}
        self._encoding = []          # the futures `encode` has handed out since the last `finish`

    def _to_host(self, t):
        """float32 flat copy of `t` in pinned memory + the event that says it has arrived."""
        t = t.detach().to(torch.float32).contiguous().view(-1)
        if not t.is_cuda:
            return t, None
        side = self.copy_stream.setdefault(t.device, torch.cuda.Stream(device=t.device))
        side.wait_stream(torch.cuda.current_stream(t.device))
        host = torch.empty(t.numel(), dtype=torch.float32, pin_memory=True)
        with torch.cuda.stream(side):
            host.copy_(t, non_blocking=True)
            t.record_stream(side)
            ev = torch.cuda.Event()
            ev.record(side)
        return host, ev

    def encode(self, x, p, file_name):
        """Future of the stream's size in bits."""
        assert file_name[-2:] == ".b"
        self.slots.acquire()
        (xh, ex), (ph, ep) = self._to_host(x), self._to_host(p)

        def job():
            try:
                for ev in (ex, ep):
                    if ev is not None:
                        ev.synchronize()
                return _encode_host(xh, ph, file_name)
            finally:
                self.slots.release()
        self._encoding.append(self.pool.submit(job))
        return self._encoding[-1]

    def finish(self):
        """Waits for every stream handed to `encode`; returns their total size in bits."""
        done, self._encoding = self._encoding, []
        return sum(f.result() for f in done)

    def decode(self, p, file_name):
        """Future of the decoded float32 +-1 HOST tensor (pinned when p lives on a GPU)."""
        assert file_name[-2:] == ".b"
        self.slots.acquire()
        ph, ep = self._to_host(p)

        def job():
            try:
                if ep is not None:
                    ep.synchronize()
                return _decode_host(ph, file_name)
            finally:
                self.slots.release()
        return self.pool.submit(job)

    def decode_group(self, items):
        """items: (p, file name) of streams that do not depend on each other, taken one by one: a stream is being
        decoded while the caller's iterable works out the next one's p.  Returns their symbols on p's device, in order."""
        pending = [(self.decode(p, file_name), p.device) for p, file_name in items]
        return [fut.result().to(dev) for fut, dev in pending]

    def check(self):
        """Nothing to report: the range coder's streams carry no status."""

    def shutdown(self):
        self.pool.shutdown(wait=True)


# Symbols per rANS lane of the device coder when the caller names none: the smallest of 2^12, 2^14, 2^16 whose
# full-size container stays within 1 % of the host coder's (profiles/device_coder.md).
DEVICE_CODER_SYMBOLS_PER_LANE = 16384


def _flat_p(p):
    """(float32 device tensor, p_stride, n) of a probability tensor: an expanded scalar (the levels coded with one
    Pg) stays one element, read with stride 0."""
    n = p.numel()
    if p.dim() == 1 and n > 1 and p.stride(0) == 0:
        return p.detach()[:1].to(torch.float32).contiguous(), 0, n
    return p.detach().to(torch.float32).contiguous().view(-1), 1, n


class DeviceCoder:
    """The call shape of `CoderPool` on the device entropy coder (cnc_amd/csrc/rans_coder.hip, the "rans1" format of
    include/cnc_codec.h): symbols and probabilities stay where they are, one batched call codes every stream handed
    over, and only compressed bytes cross PCIe.  `encode` collects; `finish` launches, copies sizes and bytes to the
    host, writes the .b files and returns the bits.  `decode_group` checks the files on the host (`cnc_rans_check`),
    uploads their bytes in one copy and returns the decoded DEVICE tensors without waiting; the streams' status words
    are read by `check()`, once, when the caller is done."""

    def __init__(self, symbols_per_lane=None):
        self.S = int(symbols_per_lane or DEVICE_CODER_SYMBOLS_PER_LANE)
        if self.S < 1:
            raise ValueError("symbols_per_lane must be >= 1")
        self._queued = []            # (x, p, p_stride, n, file name)
        self._status = []            # (status tensor, file names) of the decode groups so far

    # ---- encode
    def encode(self, x, p, file_name):
        assert file_name[-2:] == ".b"
        if not x.is_cuda:
            raise RuntimeError("x must be a CUDA tensor")
        x = x.detach().to(torch.float32).contiguous().view(-1)
        p, stride, n = _flat_p(p)
        assert n == x.numel() or (stride == 1 and n == 1 == x.numel())
        self._queued.append((x, p, stride, x.numel(), file_name))

    def finish(self):
        """Codes everything queued; returns the total size in bits."""
        from . import _lib
        if not self._queued:
            return 0
        L, Lc = _lib.lib(), _codec_lib()
        dev = self._queued[0][0].device
        caps = [int(Lc.cnc_rans_bound(n, self.S)) for _, _, _, n, _ in self._queued]
        at = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        out = torch.empty(int(at[-1]), dtype=torch.uint8, device=dev)
        table = (_lib.RansStream * len(caps))()
        for k, (x, p, stride, n, _) in enumerate(self._queued):
            table[k] = _lib.RansStream(p.data_ptr(), stride, x.data_ptr(), n, self.S, out.data_ptr() + int(at[k]), caps[k])
        need = int(L.cnc_rans_scratch_bytes(table, len(caps)))
        scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        sizes = torch.empty(len(caps), dtype=torch.int64, device=dev)
        _lib.check(L.cnc_rans_encode_pm1(table, len(caps), scratch.data_ptr(), need, sizes.data_ptr(), _lib.stream(dev)),
                   "rans_encode_pm1")
        sizes_h = sizes.cpu().tolist()
        if min(sizes_h) < 0:
            raise RuntimeError("device coder: output buffer too small")
        # the streams packed on the device, then one copy of what was written (a few hundred KB of the worst-case buffer)
        packed = torch.cat([out[int(at[k]):int(at[k]) + s] for k, s in enumerate(sizes_h)]).cpu().numpy()
        pos = 0
        for (_, _, _, _, file_name), s in zip(self._queued, sizes_h):
            with open(file_name, "wb") as fout:
                fout.write(packed[pos:pos + s].tobytes())
            pos += s
        self._queued = []
        return 8 * sum(sizes_h)

    # ---- decode
    def decode_group(self, items):
        """items: [(p, file name)], streams that do not depend on each other.  Returns their symbols as float32 +-1
        DEVICE tensors, in order.  A file that is not a well-formed rans1 stream for p's length raises here, on the host,
        before anything is uploaded or launched."""
        Lc = _codec_lib()
        items = list(items)
        blobs, ps = [], []
        for p, file_name in items:
            assert file_name[-2:] == ".b"
            if not p.is_cuda:
                raise RuntimeError("p must be a CUDA tensor")
            with open(file_name, "rb") as fin:
                blob = np.frombuffer(fin.read(), dtype=np.uint8)
            p, stride, n = _flat_p(p)
            if Lc.cnc_rans_check(blob.ctypes.data, blob.shape[0], n) < 0:
                raise RuntimeError(f"{file_name}: not a valid rans1 stream of {n} symbols")
            blobs.append(blob)
            ps.append((p, stride, n))
        return self._launch_decode(ps, blobs, [f for _, f in items])

    def _launch_decode(self, ps, blobs, names):
        from . import _lib
        L = _lib.lib()
        dev = ps[0][0].device
        at = np.concatenate([[0], np.cumsum([b.shape[0] for b in blobs])]).astype(np.int64)
        host = torch.from_numpy(np.concatenate(blobs))
        data = (host.pin_memory() if dev.type == "cuda" else host).to(dev, non_blocking=True)
        outs = [torch.empty(n, dtype=torch.float32, device=dev) for _, _, n in ps]
        status = torch.empty(len(ps), dtype=torch.int32, device=dev)
        table = (_lib.RansStream * len(ps))()
        for k, (p, stride, n) in enumerate(ps):
            table[k] = _lib.RansStream(p.data_ptr(), stride, outs[k].data_ptr(), n, 0, data.data_ptr() + int(at[k]),
                                       int(blobs[k].shape[0]))
        _lib.check(L.cnc_rans_decode_pm1(table, len(ps), status.data_ptr(), _lib.stream(dev)), "rans_decode_pm1")
        self._status.append((status, names))
        return outs

    def check(self):
        """One host wait for every group decoded so far: raises if a lane of any stream did not end where it began,
        naming every such stream of every group.  The groups are forgotten either way: a verdict is given once."""
        groups, self._status = self._status, []
        bad = [n for status, names in groups for n, s in zip(names, status.cpu().tolist()) if s != 0]
        if bad:
            raise RuntimeError(f"device coder: damaged stream(s) {bad}")

    def shutdown(self):
        self._queued = []


def make_coder(kind, symbols_per_lane=None):
    """`CoderPool()` for kind "host", `DeviceCoder(symbols_per_lane)` for "device"."""
    if kind not in ("host", "device"):
        raise ValueError(f"coder must be 'host' or 'device', not {kind!r}")
    return DeviceCoder(symbols_per_lane) if kind == "device" else CoderPool()
