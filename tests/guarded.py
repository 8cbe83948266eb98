"""Device buffers for tests that call the C ABI directly: each buffer lies in the middle of a larger allocation filled
with a sentinel byte, 32 KiB (two of the widest kernels' blocks) on either side, so that a kernel writing before or
behind its buffer fails an assertion instead of faulting, and nothing is ever placed at the end of an allocation."""
import numpy as np
import torch

PAD = 32768          # bytes on either side; a multiple of 256, so the buffer keeps the allocation's alignment
FILL = 0xA5
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32,
          np.dtype(np.uint32): torch.int32}


class Guarded:
    def __init__(self, host, dev, shift=0):
        """`host`: a NumPy array (float32, int32, uint32 or uint8, any shape) to upload; `shift` bytes move the buffer off
        its alignment."""
        host = np.ascontiguousarray(host)
        self._place(host.shape, host.dtype, dev, shift)
        if self.nbytes:
            self.alloc[self.lo:self.lo + self.nbytes] = torch.from_numpy(host.reshape(-1).view(np.uint8).copy()).to(dev)

    def _place(self, shape, dtype, dev, shift):
        self.dtype, self.shape, self.shift = np.dtype(dtype), tuple(shape), shift
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.alloc = torch.full((2 * PAD + self.nbytes + 256,), FILL, dtype=torch.uint8, device=dev)
        self.lo = PAD + shift
        self.ptr = self.alloc.data_ptr() + self.lo

    @classmethod
    def empty(cls, shape, dtype, dev, shift=0):
        """A buffer whose own bytes are the sentinel too: what a kernel leaves unwritten inside it still shows."""
        g = cls.__new__(cls)
        g._place(shape, dtype, dev, shift)
        return g

    @classmethod
    def like(cls, t):
        """A guarded copy of a device tensor (float32, int32 or uint8), made on the device."""
        dt = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}[t.dtype]
        g = cls.empty(tuple(t.shape), dt, t.device)
        g.tensor().copy_(t)
        return g

    def tensor(self):
        """The buffer as a device tensor (a view of the allocation)."""
        return self.alloc[self.lo:self.lo + self.nbytes].view(_TORCH[self.dtype]).view(self.shape)

    def get(self):
        raw = self.alloc[self.lo:self.lo + self.nbytes].cpu().numpy()
        return raw.view(self.dtype).reshape(self.shape).copy()

    def intact(self):
        """The bytes around the buffer are still the sentinel."""
        a = self.alloc
        return bool((a[:self.lo] == FILL).all()) and bool((a[self.lo + self.nbytes:] == FILL).all())

    def snapshot(self):
        return self.alloc.clone()

    def unchanged_since(self, snap):
        return bool(torch.equal(self.alloc, snap))


def sentinel(dtype):
    """The value an element of `dtype` has while it still holds the fill bytes."""
    return np.full(np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)[0]
