"""The guarded training step's verdict (csrc/step_verdict.hip): go, or skip, decided on the device before the optimizer's
update — `TrainConfig(guarded_step=True)`, `CNC_GUARDED_STEP=1`, `python -m cnc_amd.train --guarded-step`.

A `StepGuard` owns the verdict buffer (cnc_step_verdict_t) and the float torch's fused Adam takes as `found_inf`.  A step

    guard.scan(tensors, range_guard=(words, seen, pack_id))      # any number of times; the reasons accumulate
    guard.seal(lr, beta1, beta2, eps, weight_decay, clip_counters)
    table_adam.step(pieces, guard=guard); opt.found_inf = guard.found_inf; opt.step()

never waits for the device: the kernels that follow read the verdict where it lies.  A skipped step leaves parameters,
moments, step counts, sign planes and clip counters as they were.  The bias corrections of the tables' update come from two
running products b1^t, b2^t in the buffer, advanced by the seal on every step that goes ahead (seeded here from the
optimizer's own step count: `seed`), not from a host mirror of the step count — which a skipped step would leave one ahead.

Reference: GradScaler(2**10) whose `step` is never called (examples/train_CNC_nerf_synthetic.py:211,361-363): it has no such
check; torch.amp.GradScaler.step is the behaviour this follows (skip on a non-finite gradient, schedulers step regardless).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib

NONFINITE = _lib.CNC_VERDICT_NONFINITE
RANGE_GUARD = _lib.CNC_VERDICT_RANGE_GUARD
_N64 = C.sizeof(_lib.StepVerdict) // 8


class StepGuard:
    def __init__(self, device, beta1: float, beta2: float, steps_taken: int = 0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("StepGuard: the verdict lives on the GPU (no CPU fallback)")
        self.beta1, self.beta2 = float(beta1), float(beta2)
        self._buf = torch.zeros(_N64, dtype=torch.float64, device=self.device)        # cnc_step_verdict_t, 8-byte aligned
        self.words = self._buf.view(torch.int32)                # [0..3] = acc, skip, skipped, reasons_seen
        self.found_inf = torch.zeros((), dtype=torch.float32, device=self.device)
        self._scans: Dict[int, Tuple[tuple, _lib.VerdictScan]] = {}                   # chunk -> (key, filled struct)
        self._keep: List[torch.Tensor] = []
        self._host = self._evt = None                           # `poll`
        self._warned = False
        self.seed(steps_taken)

    @property
    def ptr(self) -> int:
        return self._buf.data_ptr()

    def seed(self, steps_taken: int) -> None:
        """The running products for an optimizer that has taken `steps_taken` updates: pow(beta, t0), the one place a library
        pow enters (at t0 = 0: exactly 1).  At construction and wherever a state is loaded; not per step."""
        t0 = int(steps_taken)
        if t0 < 0:
            raise ValueError("StepGuard.seed: a negative step count")
        seeds = torch.tensor([math.pow(self.beta1, t0), math.pow(self.beta2, t0)], dtype=torch.float64)
        self._buf[2:4].copy_(seeds)

    def _stream(self) -> int:
        return _lib.stream(self.device)

    def scan(self, tensors: Sequence[Optional[torch.Tensor]] = (), range_guard=None,
             poison: Optional[torch.Tensor] = None) -> None:
        """OR this step's reasons into the verdict: NONFINITE when any element of `tensors` (float32, on this device; None and
        empty ones are passed over) is +-inf or NaN, RANGE_GUARD when `range_guard` = (the field's guard words, seen,
        pack_id) satisfies `check_range_guard`'s predicate.  `poison` (one float32 element on the device): receives +inf
        when that predicate held, else 0.  On the current stream; 48 tensors a launch."""
        ts = []
        for t in tensors:
            if t is None or t.numel() == 0:
                continue
            if t.dtype != torch.float32 or t.device != self.device:
                raise RuntimeError("StepGuard.scan: float32 tensors on the guard's device")
            ts.append(t if t.is_contiguous() else t.contiguous())
        self._keep = ts
        L, stream, cap = _lib.lib(), self._stream(), _lib.CNC_VERDICT_MAX_TENSORS
        n_chunks = max(1, -(-len(ts) // cap)) if (ts or range_guard is not None or poison is not None) else 0
        for c in range(n_chunks):
            part = ts[c * cap:(c + 1) * cap]
            key = tuple((t.data_ptr(), t.numel()) for t in part)
            hit = self._scans.get(c)
            if hit is None or hit[0] != key:                   # the list is rebuilt only when a tensor moved
                a = _lib.VerdictScan()
                a.n_tensors = len(part)
                for k, (p, n) in enumerate(key):
                    a.ptr[k], a.n[k] = p, n
                a.verdict = self.ptr
                self._scans[c] = hit = (key, a)
            a = hit[1]
            a.guard = a.poison = None
            a.guard_seen = a.pack_id = 0
            if c == 0:                                         # the guard's share rides in the first launch
                if range_guard is not None:
                    words, seen, pack_id = range_guard
                    if words.device != self.device or words.dtype != torch.int32 or words.numel() < 6:
                        raise RuntimeError("StepGuard.scan: the range guard's words are six int32 on the guard's device")
                    a.guard, a.guard_seen, a.pack_id = words.data_ptr(), int(seen) & 0xFFFFFFFF, int(pack_id) & 0xFFFFFFFF
                if poison is not None:
                    if poison.device != self.device or poison.dtype != torch.float32 or poison.numel() != 1:
                        raise RuntimeError("StepGuard.scan: `poison` is one float32 element on the guard's device")
                    a.poison = poison.data_ptr()
            _lib.check(L.cnc_step_verdict_scan(C.byref(a), stream), "cnc_step_verdict_scan")

    def seal(self, lr: float, eps: float, weight_decay: float, clip_counters: Sequence[torch.Tensor] = ()) -> None:
        """Close the step's verdict behind its last scan: `skip` and `found_inf` stand until the next seal.  lr, eps,
        weight_decay: the tables' parameter group at this step; `clip_counters` (up to four int32 device scalars): zeroed
        when the step goes ahead."""
        if len(clip_counters) > 4:
            raise RuntimeError("StepGuard.seal: up to four clip counters")
        a = _lib.VerdictSeal()
        a.verdict, a.found_inf = self.ptr, self.found_inf.data_ptr()
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = float(lr), self.beta1, self.beta2, float(eps), float(weight_decay)
        for k, cc in enumerate(clip_counters):
            if cc.device != self.device or cc.dtype != torch.int32 or cc.numel() != 1:
                raise RuntimeError("StepGuard.seal: a clip counter is one int32 element on the guard's device")
            a.clip_count[k] = cc.data_ptr()
        _lib.check(_lib.lib().cnc_step_verdict_seal(C.byref(a), self._stream()), "cnc_step_verdict_seal")
        self._snapshot()

    def _snapshot(self) -> None:
        """The verdict's four words on their way to pinned host memory (16 bytes, no wait), unless the copy before is still
        in flight — `poll` looks at what has arrived."""
        if self._evt is not None and not self._evt.query():
            return
        if self._host is None:
            self._host = torch.zeros(4, dtype=torch.int32).pin_memory()
        self._host.copy_(self.words[:4], non_blocking=True)
        self._evt = torch.cuda.Event()
        self._evt.record()

    def poll(self) -> Optional[Dict[str, int]]:
        """What the last arrived snapshot shows, {"skipped", "reasons"}, or None while none has arrived.  Never waits.  Warns
        once, the first time a skipped step is seen."""
        if self._evt is None or not self._evt.query():
            return None
        w = self._host.tolist()
        seen = {"skipped": w[2], "reasons": w[3]}
        if w[2] and not self._warned:
            import warnings
            self._warned = True
            why = [n for b, n in ((NONFINITE, "a non-finite gradient or loss"), (RANGE_GUARD, "the fp16 range guard")) if w[3] & b]
            warnings.warn(f"cnc_amd: the guarded step skipped an optimizer update ({' and '.join(why)}); "
                          f"{w[2]} skipped so far")
        return seen

    def stats(self) -> Dict[str, int]:
        """{"skipped": n, "reasons": bits} as the device has them now.  Synchronises: for logs and tests."""
        w = self.words[:4].tolist()
        return {"skipped": w[2], "reasons": w[3]}

    def last_skip(self) -> int:
        """The sealed step's reasons (0 = it went ahead).  Synchronises: for tests."""
        return int(self.words[1].item())
