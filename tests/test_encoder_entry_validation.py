"""CPU-only: the host-side checks of the six hash-grid encoder entry points, pinned by their return codes.

Every call here is refused, or trivially accepted (N = 0, L = 0), BEFORE any launch.  Each non-null pointer is one fake,
16-byte-aligned address the host never dereferences, so the test skips itself wherever a GPU is visible: with a device
present, a regression in the ORDER of the checks would launch a kernel on that address.  The expected values were
recorded from the entries as they stood before they shared one validator; -1 = CNC_ERR_INVALID_VALUE,
-2 = CNC_ERR_UNSUPPORTED.  The workspace sizes are pinned the same way.
"""
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host-side check order only: must never reach a device")

P = 0x7F0000001000          # the one fake address
GIB = 1 << 30
INVALID, UNSUPPORTED = -1, -2

# base call: N = 64, D = 3, F = 8, L = 2, flags 0, level-major layout
_TENSORS = dict(grad=P, inputs=P, embeddings=P, offsets=P, resolutions=P, grad_embeddings=P)
_SHAPE = dict(N=64, D=3, F=8, L=2)
_BACKWARD = dict(_TENSORS, **_SHAPE, Rb=0, dy_dx=None, grad_inputs=None, binary_vxl=None, min_level_id=None, flags=0,
                 ste_clip_count=None, occ_sat=None, vertex_bits=None, vertex_bit_offsets=None, grad_ld=0, grad_col=0,
                 stream=None)
_ORDERED = dict(_BACKWARD, workspace=P, workspace_bytes=GIB)
_BINNED = dict(_TENSORS, **_SHAPE, flags=0, ste_clip_count=None, grad_ld=0, grad_col=0, n_binned=2, level_rows=1 << 16,
               workspace=P, workspace_bytes=GIB, stream=None)
_OVERLAPPED = dict(_BINNED, plan=None)
_FORWARD = dict(inputs=P, embeddings=P, offsets=P, resolutions=P, outputs=P, **_SHAPE, Rb=0, PV=0.0, dy_dx=None,
                binary_vxl=None, min_level_id=None, flags=0, occ_sat=None, vertex_bits=None, vertex_bit_offsets=None,
                out_ld=0, out_col=0, stream=None)
_FORWARD_BITS = dict(inputs=P, bits=P, offsets=P, resolutions=P, outputs=P, **_SHAPE, Rb=0, binary_vxl=None,
                     min_level_id=None, occ_sat=None, vertex_bits=None, vertex_bit_offsets=None, out_ld=0, out_col=0,
                     stream=None)

# positional order of include/cnc_hip.h
_ORDER = {
    "cnc_grid_encode_backward": "grad inputs embeddings offsets resolutions grad_embeddings N D F L Rb dy_dx grad_inputs "
                                "binary_vxl min_level_id flags ste_clip_count occ_sat vertex_bits vertex_bit_offsets "
                                "grad_ld grad_col stream",
    "cnc_grid_encode_backward_ordered": "grad inputs embeddings offsets resolutions grad_embeddings N D F L Rb dy_dx "
                                        "grad_inputs binary_vxl min_level_id flags ste_clip_count occ_sat vertex_bits "
                                        "vertex_bit_offsets grad_ld grad_col workspace workspace_bytes stream",
    "cnc_grid_encode_backward_binned": "grad inputs embeddings offsets resolutions grad_embeddings N D F L flags "
                                       "ste_clip_count grad_ld grad_col n_binned level_rows workspace workspace_bytes stream",
    "cnc_grid_encode_backward_overlapped": "plan grad inputs embeddings offsets resolutions grad_embeddings N D F L flags "
                                           "ste_clip_count grad_ld grad_col n_binned level_rows workspace workspace_bytes "
                                           "stream",
    "cnc_grid_encode_forward": "inputs embeddings offsets resolutions outputs N D F L Rb PV dy_dx binary_vxl min_level_id "
                               "flags occ_sat vertex_bits vertex_bit_offsets out_ld out_col stream",
    "cnc_grid_encode_forward_bits": "inputs bits offsets resolutions outputs N D F L Rb binary_vxl min_level_id occ_sat "
                                    "vertex_bits vertex_bit_offsets out_ld out_col stream",
}
_BASE = {
    "cnc_grid_encode_backward": _BACKWARD, "cnc_grid_encode_backward_ordered": _ORDERED,
    "cnc_grid_encode_backward_binned": _BINNED, "cnc_grid_encode_backward_overlapped": _OVERLAPPED,
    "cnc_grid_encode_forward": _FORWARD, "cnc_grid_encode_forward_bits": _FORWARD_BITS,
}

CASES = {
    "cnc_grid_encode_backward": [
        ("dy_dx without grad_inputs", dict(dy_dx=P), INVALID),
        ("grad_inputs without dy_dx", dict(grad_inputs=P), INVALID),
        ("null grad", dict(grad=None), INVALID),
        ("N=0", dict(N=0), 0),
        ("L=0", dict(L=0), 0),
        ("N=0 with null grad", dict(N=0, grad=None), 0),
        ("grad_ld=8 grad_col=4", dict(grad_ld=8, grad_col=4), INVALID),
        ("grad_col=4 with grad_ld=0", dict(grad_col=4), INVALID),
        ("grad_ld=18", dict(grad_ld=18), INVALID),
        ("F=3", dict(F=3), INVALID),
        ("D=4", dict(D=4), INVALID),
        ("D=0", dict(D=0), INVALID),
    ],
    "cnc_grid_encode_backward_binned": [
        ("n_binned=3 > L", dict(n_binned=3), INVALID),
        ("D=2, all levels binned", dict(D=2), UNSUPPORTED),
        ("F=16, all levels binned", dict(F=16), UNSUPPORTED),
        ("null workspace", dict(workspace=None), INVALID),
        ("workspace at address+4", dict(workspace=P + 4), INVALID),
        ("workspace_bytes=1024", dict(workspace_bytes=1024), INVALID),
        ("level_rows=0", dict(level_rows=0), INVALID),
        ("level_rows=2^20+257", dict(level_rows=(1 << 20) + 257), INVALID),
        ("grad_col=4 with grad_ld=0", dict(grad_col=4), INVALID),
        ("N=0", dict(N=0), 0),
        ("null grad", dict(grad=None), INVALID),
    ],
    "cnc_grid_encode_backward_overlapped": [
        ("n_binned=3 > L", dict(n_binned=3), INVALID),
        ("null workspace", dict(workspace=None), INVALID),
        ("N=0", dict(N=0), 0),
    ],
    "cnc_grid_encode_backward_ordered": [
        ("null workspace", dict(workspace=None), INVALID),
        ("F=3", dict(F=3), INVALID),
        ("dy_dx alone", dict(dy_dx=P), INVALID),
    ],
    "cnc_grid_encode_forward": [
        ("null outputs", dict(outputs=None), INVALID),
        ("out_ld=8 out_col=4", dict(out_ld=8, out_col=4), INVALID),
        ("D=4", dict(D=4), INVALID),
        ("F=3", dict(F=3), INVALID),
        ("N=0", dict(N=0), 0),
    ],
    "cnc_grid_encode_forward_bits": [
        ("null bits", dict(bits=None), INVALID),
        ("F=3", dict(F=3), INVALID),
        ("D=4", dict(D=4), INVALID),
        ("out_ld=8 out_col=4", dict(out_ld=8, out_col=4), INVALID),
        ("N=0", dict(N=0), 0),
    ],
}


@pytest.fixture(scope="module")
def L():
    from cnc_amd import _lib, build
    build.build_all()
    return _lib.lib()


@pytest.mark.parametrize("entry,case,change,expected",
                         [(e, c[0], c[1], c[2]) for e, cases in CASES.items() for c in cases],
                         ids=[f"{e[len('cnc_grid_encode_'):]}-{c[0]}" for e, cases in CASES.items() for c in cases])
def test_entry_return_code(L, entry, case, change, expected):
    assert set(change) <= set(_BASE[entry])
    args = dict(_BASE[entry], **change)
    assert getattr(L, entry)(*[args[name] for name in _ORDER[entry].split()]) == expected


# (N, n_binned, level_rows) -> bytes, read from the entries before the scratch split was shared
WORKSPACES = [
    ((1, 1, 1), 1552, 3840),
    ((65536, 1, 65536), 33820672, 33837056),
    ((1046496, 6, 524288), 3227713536, 3227975680),
    ((2 ** 24 - 1, 6, 2 ** 20), 51565166592, 51569360896),
]


@pytest.mark.parametrize("shape,binned,overlapped", WORKSPACES, ids=[str(w[0]) for w in WORKSPACES])
def test_workspace_sizes(L, shape, binned, overlapped):
    assert L.cnc_grid_encode_backward_binned_workspace(*shape) == binned
    assert L.cnc_grid_encode_backward_overlapped_workspace(*shape) == overlapped


def test_ordered_workspace_of_no_points(L):
    assert L.cnc_grid_encode_backward_ordered_workspace(0, 3, 10) == 0      # before any runtime call
