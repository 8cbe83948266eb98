"""The reproducible mode: every floating-point sum of a training step in an order that depends on the inputs, the
shapes, the device and the build only — not on scheduling, streams, other work on the GPU or the run.

Off by default.  Under the mode
  * the encoder's backward is the ordered one (`cnc_amd.ordered_backward`, cnc_grid_encode_backward_ordered),
  * the context heads' backward is cnc_ctx_mlp_backward_ordered (backends/context_backend.py),
  * the field's gradient chain sums its bias gradients in the ordered form (cnc_field_backward_chain_ordered, field.py),
  * a Trainer built with `TrainConfig.reproducible` runs the one-thread, one-stream schedule (trainer.py).

`reproducible_enabled(explicit)` resolves, in this order: the explicit argument, the process-wide mode
(`reproducible(True)`), CNC_REPRODUCIBLE=1 (read per call), torch.are_deterministic_algorithms_enabled().
"""
from __future__ import annotations

import os

_MODE = None            # process-wide: None = not set, else bool

# calls per route of the entry points that have an ordered form, for tests and tools to read (the encoder's are in
# backends.gridencoder_backend.ROUTE_CALLS)
ROUTE_CALLS = {"ctx_ordered": 0, "ctx_default": 0, "field_ordered": 0, "field_default": 0}


class reproducible:
    """Process-wide switch of the reproducible mode, as a plain setter — `reproducible(True)` — or a context manager
    that restores the previous state on exit; `reproducible(None)` clears it.  Process-wide and not thread-local for the
    reason `ordered_backward` is: backward kernels run on autograd's device thread."""

    def __init__(self, enabled=True):
        global _MODE
        self._prev = _MODE
        _MODE = None if enabled is None else bool(enabled)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _MODE
        _MODE = self._prev
        return False


def explicitly_enabled():
    """The mode was asked for by name: the process-wide switch or CNC_REPRODUCIBLE=1 (not torch's switch: callers that
    had their own answer to that one keep it)."""
    if _MODE is not None:
        return _MODE
    return os.environ.get("CNC_REPRODUCIBLE") == "1"


def reproducible_enabled(explicit=None):
    if explicit is not None:
        return bool(explicit)
    if _MODE is not None:
        return _MODE
    if os.environ.get("CNC_REPRODUCIBLE") == "1":
        return True
    import torch
    return torch.are_deterministic_algorithms_enabled()
