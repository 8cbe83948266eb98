"""Device buffers for tests that call the C ABI directly: each buffer lies in the middle of a larger allocation filled
with a sentinel byte, 32 KiB (two of the widest kernels' blocks) on either side, so that a kernel writing before or
behind its buffer fails an assertion instead of faulting, and nothing is ever placed at the end of an allocation.

The sentinel byte is a parameter (`fill`, one of `FILLS`), and `under_fills` runs one call under each of them: a kernel
whose result depends on bytes outside its inputs — past a row, in the gap between the rows of a column window
(`Guarded.window`), past a count array — gives outputs that move with the fill, or NaN under 0xFF.

What this catches is a read outside a buffer whose VALUE reaches an output (a pad column multiplied by a zero weight
included: 0xFF reads as NaN).  What it does not catch is an outside read whose value is then discarded or overwritten:
only a fault or a memory tool shows that one.  These helpers pin the value-level contract; they do not claim memory
safety."""
import numpy as np
import torch

PAD = 32768          # bytes on either side; a multiple of 256, so the buffer keeps the allocation's alignment
FILL = 0xA5
# 0x00: what a fresh allocation often holds (why such bugs hide); 0xA5: a tiny negative float32, a large negative int;
# 0xFF: a NaN float32 / float64, the int -1.  No fill reads as a large positive integer: a miscounted loop stays short.
FILLS = (0x00, 0xA5, 0xFF)
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32,
          np.dtype(np.uint32): torch.int32, np.dtype(np.int16): torch.int16, np.dtype(np.int64): torch.int64,
          np.dtype(np.float64): torch.float64, np.dtype(np.bool_): torch.bool}
_NUMPY = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8, torch.int16: np.int16,
          torch.int64: np.int64, torch.float64: np.float64, torch.bool: np.bool_}


class Guarded:
    role = "in"          # "in": under_fills requires it unchanged; "out": returned by it; "scratch": neither

    def __init__(self, host, dev, shift=0, fill=FILL):
        """`host`: a NumPy array (float32, float64, int16, int32, uint32, int64, uint8 or bool, any shape) to upload;
        `shift` bytes move the buffer off its alignment; `fill`: the sentinel byte around it."""
        host = np.ascontiguousarray(host)
        self._place(host.shape, host.dtype, dev, shift, fill)
        self._upload(host)

    def _place(self, shape, dtype, dev, shift, fill=FILL):
        self.dtype, self.shape, self.shift, self.fill = np.dtype(dtype), tuple(shape), shift, int(fill)
        if self.dtype not in _TORCH:
            raise TypeError(f"Guarded: unsupported dtype {self.dtype}")
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.alloc = torch.full((2 * PAD + self.nbytes + 256,), self.fill, dtype=torch.uint8, device=dev)
        self.lo = PAD + shift
        self.ptr = self.alloc.data_ptr() + self.lo
        self.win = None

    def _upload(self, host):
        if self.nbytes:
            raw = torch.from_numpy(host.reshape(-1).view(np.uint8).copy())       # bool travels as its 0 / 1 bytes
            self.alloc[self.lo:self.lo + self.nbytes] = raw.to(self.alloc.device)

    @classmethod
    def empty(cls, shape, dtype, dev, shift=0, fill=FILL):
        """A buffer whose own bytes are the sentinel too: what a kernel leaves unwritten inside it still shows."""
        g = cls.__new__(cls)
        g._place(shape, dtype, dev, shift, fill)
        g.role = "out"
        return g

    @classmethod
    def like(cls, t, fill=FILL):
        """A guarded copy of a device tensor, made on the device."""
        g = cls.empty(tuple(t.shape), _NUMPY[t.dtype], t.device, fill=fill)
        g.tensor().copy_(t)
        g.role = "in"
        return g

    @classmethod
    def window(cls, host2d, ld, col, dev, fill=FILL, shift=0):
        """The [N, K] array `host2d` as columns [col, col + K) of an [N, ld] buffer whose other columns hold the fill:
        a kernel that uses a row's gap sees poison.  `.ptr` and `.tensor()` address the window (row stride `ld`
        elements), `.get()` returns it, `.full()` the whole [N, ld] buffer; `intact()` includes the gap columns."""
        host2d = np.ascontiguousarray(host2d)
        N, K = host2d.shape
        if col < 0 or col + K > ld:
            raise ValueError("Guarded.window: columns [col, col + K) do not fit in ld")
        g = cls.__new__(cls)
        g._place((N, ld), host2d.dtype, dev, shift, fill)
        g.win = (col, K)
        g.ld = ld
        g.ptr += col * g.dtype.itemsize
        if host2d.size:
            item = g.dtype.itemsize
            rows = g.alloc[g.lo:g.lo + g.nbytes].view(N, ld * item)
            raw = torch.from_numpy(host2d.view(np.uint8).reshape(N, K * item).copy())
            rows[:, col * item:(col + K) * item] = raw.to(g.alloc.device)
        return g

    @classmethod
    def empty_window(cls, N, K, ld, col, dtype, dev, fill=FILL, shift=0):
        """An output window: like `window`, its own elements the sentinel too."""
        g = cls.__new__(cls)
        g._place((N, ld), dtype, dev, shift, fill)
        if col < 0 or col + K > ld:
            raise ValueError("Guarded.empty_window: columns [col, col + K) do not fit in ld")
        g.win, g.ld, g.role = (col, K), ld, "out"
        g.ptr += col * g.dtype.itemsize
        return g

    def out(self):
        """Mark an uploaded buffer as an output (an accumulator the kernel adds to)."""
        self.role = "out"
        return self

    def scratch(self):
        self.role = "scratch"
        return self

    def whole(self):
        """Every element of the buffer as a contiguous device tensor; of a window, the [N, ld] matrix with its gap columns
        (for entry points that take the matrix, a leading dimension and a first column)."""
        return self.alloc[self.lo:self.lo + self.nbytes].view(_TORCH[self.dtype]).view(self.shape)

    def tensor(self):
        """The buffer as a device tensor (a view of the allocation); of a window, the strided [N, K] view."""
        t = self.whole()
        return t if self.win is None else t[:, self.win[0]:self.win[0] + self.win[1]]

    def full(self):
        """Every element of the buffer on the host (of a window: the gap columns too)."""
        raw = self.alloc[self.lo:self.lo + self.nbytes].cpu().numpy()
        return raw.view(self.dtype).reshape(self.shape).copy()

    def get(self):
        a = self.full()
        return a if self.win is None else np.ascontiguousarray(a[:, self.win[0]:self.win[0] + self.win[1]])

    def intact(self):
        """The bytes around the buffer (and in the gap columns of a window) are still the sentinel."""
        a = self.alloc
        ok = bool((a[:self.lo] == self.fill).all()) and bool((a[self.lo + self.nbytes:] == self.fill).all())
        if ok and self.win is not None and self.nbytes:
            rows = a[self.lo:self.lo + self.nbytes].view(self.shape[0], self.ld * self.dtype.itemsize)
            b0, b1 = self.win[0] * self.dtype.itemsize, (self.win[0] + self.win[1]) * self.dtype.itemsize
            ok = bool((rows[:, :b0] == self.fill).all()) and bool((rows[:, b1:] == self.fill).all())
        return ok

    def snapshot(self):
        return self.alloc.clone()

    def unchanged_since(self, snap):
        return bool(torch.equal(self.alloc, snap))


def sentinel(dtype, fill=FILL):
    """The value an element of `dtype` has while it still holds the fill bytes."""
    return np.full(np.dtype(dtype).itemsize, fill, np.uint8).view(dtype)[0]


def holds_fill(a, fill):
    """Every byte of the NumPy array `a` is the fill: nothing wrote there."""
    return bool((np.ascontiguousarray(a).reshape(-1).view(np.uint8) == fill).all())


def same_bits(a, b):
    """Equality of shape, type and raw bytes (NumPy arrays or tensors): NaN payloads and -0 count."""
    a, b = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (a, b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8),
                          np.ascontiguousarray(b).reshape(-1).view(np.uint8))


class _Bufs(dict):
    """The buffers of one run of `under_fills`.  A buffer entered while the call is being made (`bufs[name] = g`: helpers
    that build their operands themselves) is held to the same rules as one `build` returned: it must carry the run's fill,
    and an input is snapshotted the moment it is entered."""

    def __init__(self, fill):
        super().__init__()
        self.fill, self.snaps = fill, {}

    def __setitem__(self, name, g):
        assert name not in self, f"two buffers named '{name}'"
        assert g.fill == self.fill, f"{name} was not built with fill {self.fill:#x}"
        if g.role == "in":
            self.snaps[name] = g.snapshot()
        super().__setitem__(name, g)


def under_fills(build, run, fills=FILLS):
    """One call under every fill.  `build(fill)` -> {name: Guarded or None} (inputs, outputs, scratch: see `role`);
    `run(bufs)` makes the call and may enter further buffers into `bufs`.  After each run every buffer must be
    `intact()` and every input byte-identical to its snapshot.  -> {fill: {name: host array of each output}}."""
    res = {}
    for fill in fills:
        bufs = _Bufs(fill)
        for k, g in build(fill).items():
            if g is not None:
                bufs[k] = g
        run(bufs)
        if any(g.alloc.is_cuda for g in bufs.values()):
            torch.cuda.synchronize()
        for k, g in bufs.items():
            assert g.intact(), f"fill {fill:#x}: bytes around '{k}' were written"
        for k, s in bufs.snaps.items():
            assert bufs[k].unchanged_since(s), f"fill {fill:#x}: input '{k}' was modified"
        res[fill] = {k: g.get() for k, g in bufs.items() if g.role == "out"}
    return res


def moved_with_fill(per_fill):
    """Names of the outputs of `under_fills` that are not `same_bits` under every fill."""
    fills = list(per_fill)
    return sorted(k for k in per_fill[fills[0]]
                  if not all(same_bits(per_fill[fills[0]][k], per_fill[f][k]) for f in fills[1:]))
