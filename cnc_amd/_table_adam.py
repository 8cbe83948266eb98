"""The optimizer's update of the feature tables as ONE kernel that sums the step's gradient pieces on the way in
(cnc_table_adam, csrc/table_adam.hip) — for the training step (cnc_amd.trainer), single-process and data-parallel alike: the
data-parallel step hands the all-reduced SUM of the ray-loss gradient over as the first piece with the factor 1 / world
(cnc_table_adam_scaled), so the mean is taken inside the kernel.

The tables stay in the Trainer's torch.optim.Adam (their own parameter group: one learning-rate schedule for everything),
and the kernel works on THAT optimizer's state tensors (`exp_avg`, `exp_avg_sq`, the float32 device-side `step` of its
fused form): a step may go through either — `TableAdam.step(...)` leaves the tables' `.grad` None, which is how
`Optimizer.step()` skips a parameter, so the library's step that follows updates everything else; a step whose gradients
were flushed into `.grad` instead (`Trainer.fused_table_adam = False`, the tests that read `.grad`) goes through the library
as before.

Reference: torch.optim.Adam(lr, eps=1e-15, weight_decay) over every parameter, stepped once per iteration
(examples/train_CNC_nerf_synthetic.py:254-259,363).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _caches, _lib

Piece = Tuple[torch.Tensor, Optional[Tuple[int, int]]]       # (gradient piece, the ROWS of the table it covers or None = all)


class TableAdam:
    def __init__(self, opt: torch.optim.Adam, tables: Sequence[torch.nn.Parameter], encoders: Optional[Sequence] = None):
        """`encoders` (optional, one GridEncoder per table, `encoder.params is table`): the kernel then also leaves each
        updated table's sign bit plane and clip counter in the encoder's cache buffers (what `GridEncoder._bit_plane` would
        make by reading the table again at the next forward); `mark_planes_current()` re-validates them after the library
        optimizers' post-step hook has dropped every cache."""
        self.opt = opt
        self.tables: List[torch.nn.Parameter] = list(tables)
        self.encoders = list(encoders) if encoders is not None else None
        if self.encoders is not None and (len(self.encoders) != len(self.tables)
                                          or any(e.params is not p for e, p in zip(self.encoders, self.tables))):
            raise ValueError("TableAdam: one encoder per table, in the tables' order")
        self._planes_written: List = []
        if not 1 <= len(self.tables) <= 4:
            raise ValueError("TableAdam: one to four tables")
        ids = {id(p) for p in self.tables}
        groups = [g for g in opt.param_groups if any(id(p) in ids for p in g["params"])]
        if len(groups) != 1 or {id(p) for p in groups[0]["params"]} != ids:
            raise ValueError("TableAdam: the tables must be one parameter group of the optimizer, and all of it")
        self.group = groups[0]
        g = self.group
        if g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable") \
                or g.get("decoupled_weight_decay"):
            raise ValueError("TableAdam: plain Adam only (no amsgrad / maximize / capturable / decoupled decay)")
        for p in self.tables:
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or p.numel() % 4:
                raise ValueError("TableAdam: contiguous float32 device tables of a multiple of 4 elements")
        # host mirror of the state's step count (the bias corrections are host scalars).  With a guard (`step(guard=...)`):
        # the steps ATTEMPTED — a skipped one counts here and not on the device — and no arithmetic reads it
        self.steps_done = 0
        self.last_grad_scale = 1.0     # the factor of the last `step`'s `.grad` pieces (for the tests)
        self.resync()                  # an optimizer that has stepped (or loaded a state) before this was built

    def refusal(self, row_ranges: Dict[int, Sequence[Tuple[int, int]]], max_pieces: int) -> Optional[str]:
        """What cnc_table_adam would refuse in the middle of a step, checked once: `row_ranges[id(p)]` = every (first row, end
        row) a piece of table `p` can cover short of the whole table, `max_pieces` = the most pieces any schedule hands
        over for one table, `.grad` included.  Returns the reason, or None when every step can go through the kernel."""
        if max_pieces > 4:
            return f"a step can hold {max_pieces} gradient pieces for one table, the kernel takes four"
        for p in self.tables:
            row = p.numel() // p.shape[0]
            for r0, r1 in row_ranges.get(id(p), ()):
                lo, hi = r0 * row, r1 * row
                if not 0 <= lo <= hi <= p.numel() or lo % 4 or (hi % 4 and hi != p.numel()):
                    return f"a gradient piece covers elements [{lo}, {hi}) of a table of {p.numel()}: not whole float4s"
        return None

    def _state(self, p):
        st = self.opt.state[p]
        if len(st) == 0:               # as Adam._init_group lays it out for the fused form
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if not (torch.is_tensor(st["step"]) and st["step"].is_cuda and st["step"].dtype == torch.float32):
            raise RuntimeError("TableAdam: the optimizer keeps its step count on the host (not the fused form)")
        return st

    def resync(self) -> None:
        """Take the step count over from the optimizer's state (after steps that went through the library).  Nothing
        re-reads it per step: whoever loads a state into the optimizer calls this — `Trainer.load_optimizer_state` does;
        `opt.load_state_dict` on its own leaves `steps_done`, and with it the bias corrections, stale."""
        st = self.opt.state.get(self.tables[0], {})
        self.steps_done = int(float(st["step"])) if len(st) else 0

    def _plane_targets(self):
        """(table index, encoder, table, sign plane, clip counter) for every table whose encoder holds cache buffers of the
        size the table needs: where the kernel leaves the updated tables' planes."""
        out = []
        if self.encoders is not None:
            for k, (p, e) in enumerate(zip(self.tables, self.encoders)):
                bits, cc = getattr(e, "_bits", None), getattr(e, "_clip_count", None)
                if (p.numel() % 8 == 0 and bits is not None and cc is not None and bits.device == p.device
                        and bits.dtype == torch.uint8 and bits.numel() == p.numel() // 8 and cc.device == p.device
                        and cc.numel() == 1 and cc.dtype == torch.int32 and getattr(e, "bitplane", True)):
                    out.append((k, e, p, bits, cc))
        return out

    def clip_counters(self) -> List[torch.Tensor]:
        """The clip counters the next `step` adds to: what a guard's seal zeroes in this class's stead."""
        return [t[4] for t in self._plane_targets()]

    @torch.no_grad()
    def step(self, pieces: Dict[int, List[Piece]], grad_scale: float = 1.0, guard=None) -> None:
        """One Adam update of every table from its gradient pieces (`pieces[id(p)]`, in the order they are to be summed; a
        table's own `.grad`, if autograd left one, goes first and is dropped).  On the current stream: every piece must
        be complete on it.  A table with no piece at all is updated with a zero gradient — like the library's step on a
        `.grad` of zeros (a table always has a gradient in a training step; moments and weight decay move it regardless).
        `grad_scale` (a float32 value): the factor of every table's `.grad` piece — 1 / world for the data-parallel step,
        whose `.grad` is the SUM over the ranks; the other pieces are taken as they are.
        `guard` (a `_step_guard.StepGuard`, sealed for this step with `clip_counters()`): the update goes through
        cnc_table_adam_guarded — skip and bias corrections come from the guard's buffer on the device, the clip counters
        were zeroed by its seal, and `steps_done` only counts the attempt."""
        g = self.group
        grad_scale = float(grad_scale)
        if grad_scale != 1.0 and any(p.grad is None for p in self.tables):
            raise RuntimeError("TableAdam: a gradient scale but a table without `.grad` (the scale belongs to that piece)")
        a = _lib.AdamTables()
        a.n_tables = len(self.tables)
        keep = []
        for k, p in enumerate(self.tables):
            st = self._state(p)
            t = a.table[k]
            t.p, t.m, t.v, t.step, t.n = p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), \
                st["step"].data_ptr(), p.numel()
            row = p.numel() // p.shape[0]
            src: List[Piece] = ([(p.grad, None)] if p.grad is not None else []) + list(pieces.get(id(p), ()))
            if len(src) > 4:
                raise RuntimeError("TableAdam: more than four gradient pieces for one table")
            for j, (gt, rows) in enumerate(src):
                lo, hi = (0, p.numel()) if rows is None else (rows[0] * row, rows[1] * row)
                if gt.dtype != torch.float32 or gt.device != p.device or not gt.is_contiguous() or gt.numel() != hi - lo:
                    raise RuntimeError("TableAdam: a gradient piece must be a contiguous float32 tensor of its range's size")
                t.g[j], t.g_lo[j], t.g_hi[j] = gt.data_ptr(), lo, hi
                keep.append(gt)
            p.grad = None
        # the updated tables' sign planes into the encoders' own cache buffers (kept at their addresses: a recorded graph
        # reads them there), when those exist in the size the table needs
        self._planes_written = []
        counters = []
        for k, e, p, bits, cc in self._plane_targets():
            a.table[k].sign_bits, a.table[k].clip_count = bits.data_ptr(), cc.data_ptr()
            counters.append(cc)
            self._planes_written.append((e, p))
        if counters and guard is None:
            torch._foreach_zero_(counters)
        b1, b2 = g["betas"]
        lr = g["lr"]
        args = (float(lr), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), float(self.steps_done + 1),
                torch.cuda.current_stream(self.tables[0].device).cuda_stream)
        if guard is not None:
            scale = None if grad_scale == 1.0 else (C.c_float * 4)(grad_scale, 1.0, 1.0, 1.0)
            _lib.check(_lib.lib().cnc_table_adam_guarded(C.byref(a), scale, guard.ptr, args[-1]), "cnc_table_adam_guarded")
        elif grad_scale == 1.0:
            _lib.check(_lib.lib().cnc_table_adam(C.byref(a), *args), "cnc_table_adam")
        else:                          # `.grad` is slot 0 of every table (checked above: they all have one)
            scale = (C.c_float * 4)(grad_scale, 1.0, 1.0, 1.0)
            _lib.check(_lib.lib().cnc_table_adam_scaled(C.byref(a), scale, *args), "cnc_table_adam_scaled")
        self.steps_done += 1           # behind the call: a refused step has changed nothing on the device, nor here
        self.last_grad_scale = grad_scale
        # the kernel writes the tables through their addresses: `Tensor._version` does not move, so the copies keyed on it
        # (the encoders' sign bit planes, packed weights) are dropped here as after any optimizer step (cnc_amd._caches)
        _caches.invalidate_all()
        self.mark_planes_current()

    def mark_planes_current(self) -> None:
        """The sign planes the last `step` wrote ARE the planes of the tables as they stand (nothing has written the tables
        since): re-validate the encoders' cache entries.  Called by `step` itself, and by the Trainer once more behind the
        library optimizers' steps — their post-step hook (cnc_amd._caches) drops every cache, it cannot know which
        parameters a step touched."""
        for e, p in self._planes_written:
            e._bits_key = (p.data_ptr(), p._version, tuple(p.shape))
            e._bits_src = (p,)
