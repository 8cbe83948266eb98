"""The lattice of models the fused field kernels admit (`FusedFieldForward.supported`, `_chain_ok`: cnc_amd/field.py), as
data, and the references its tests hold the kernels to — test infrastructure, no GPU needed.

A composition is (F, H, L3, L2, tables): F features per level, H neurons, L3 levels of the 3-D grid and L2 levels of each
of the three plane grids, their resolutions prefixes of two fixed ladders.  The first layer's input row of such a model is
[3-D units | xy | xz | yz units (F columns each) | x (3) | sin, cos (60) | 0 up to roundup32(K0)], K0 = F units + 63,
units = L3 + 3 L2.  The two-wave kernel (csrc/field_fused2.hip) works on that row in 32-column chunks, a wave on a
16-column half of a chunk, a thread on an 8-column window; what a half holds decides the code it runs (`window_kinds`).
The lattice puts the encoders' boundaries and the tail's start U = F units at every residue of a chunk, the chain's
column blocks at their extremes, and K0 up to 575.

`reference_features` builds the rows with none of the code under test: oracle.grid_encode_forward (the CPU oracle,
gridencoder.cu:114-316) on the binarised tables, float32 coordinates, float64 NumPy sinusoids."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

LADDER_3D = (5, 6, 8, 9, 11, 14, 17, 20, 24, 29, 34, 40, 47, 55, 64, 75,
             # continued for the one composition with more 3-D levels than the ladder above has: the 67-unit fallback
             88, 104, 122)
LADDER_2D = (6, 10, 14, 18, 22, 26, 34, 42, 50, 66, 82, 98, 130, 162, 194, 258)
N_FREQS = 10
MAX_UNITS = 64                       # kMaxUnits, csrc/field_fused2.hip
PLANE_DIMS = ((0, 1, 2), (0, 1), (0, 2), (1, 2))          # xyz | xy | xz | yz (ngp.py:631-642)

# kind: "fused" (every fused kernel must run), or the fallback it must take without raising
Entry = namedtuple("Entry", "name F H L3 L2 tables kind")


def _e(F, H, L3, L2, tables="mixed", kind="fused", tag=""):
    name = f"f{F}_h{H}_{L3}x3d_{L2}x2d" + ("" if tables == "mixed" else "_" + tables) + ("_" + tag if tag else "")
    return Entry(name, F, H, L3, L2, tables, kind)


# ---- residue sweep at H = 160: units = L3 + 3 L2 takes every residue mod 32 / F; L3 odd and even, L2 in {1, 2, 3, 5} ----
_SWEEP_F2 = [(13, 1), (2, 5), (9, 3), (4, 5), (5, 5), (2, 1), (3, 1), (4, 1),            # units % 16 = 0 .. 7
             (15, 3), (3, 2), (11, 5), (2, 3), (6, 2), (7, 2), (8, 2), (6, 3)]           # 8 .. 15
_SWEEP_F4 = [(5, 1), (3, 2), (4, 2), (4, 5), (3, 3), (6, 5), (11, 1), (6, 3)]            # units % 8 = 0 .. 7
_SWEEP_F8 = [(9, 1), (3, 2), (5, 3), (4, 5)]                                             # units % 4 = 0 .. 3
# ---- reduced sweep at H = 64 ----
_SWEEP_F2_H64 = [(3, 1), (2, 3), (7, 2), (5, 5)]                                          # units % 16 = 6, 11, 13, 4
_SWEEP_F4_H64 = [(1, 2), (4, 2), (6, 1), (3, 3)]                                          # units % 8 = 7, 2, 1, 4

LATTICE = (
    [_e(2, 160, a, b) for a, b in _SWEEP_F2] + [_e(4, 160, a, b) for a, b in _SWEEP_F4]
    + [_e(8, 160, a, b) for a, b in _SWEEP_F8]
    + [_e(2, 64, a, b) for a, b in _SWEEP_F2_H64] + [_e(4, 64, a, b) for a, b in _SWEEP_F4_H64]
    + [
        # ---- extremes ----
        _e(2, 160, 1, 1), _e(4, 160, 1, 1), _e(8, 160, 1, 1),           # the fewest units (n_enc 8, 16, 32)
        _e(8, 160, 16, 16),                                             # 64 units: K0 = 575, the unit table full
        _e(2, 160, 16, 16),                                             # 64 units at F = 2: every 16-column half one encoder
        _e(8, 160, 13, 9),                                              # 40 units: K0 = 383
        _e(8, 160, 5, 2, tables="dense"),
        _e(2, 64, 4, 2, tables="hashed"),
        # the chain's column blocks: n_enc = 100, 164, 184, 188, 192 (8, 12, 112 are (1, 1) and (3, 1) at F = 2, (5, 3) at F = 8)
        _e(4, 160, 10, 5), _e(4, 160, 14, 9), _e(8, 160, 8, 5), _e(4, 160, 11, 12), _e(8, 160, 12, 4),
        # ---- fallbacks that must not raise ----
        _e(2, 160, 19, 16, kind="units"),                               # 67 units: the op chain
        _e(8, 64, 3, 2, kind="shape"),                                  # geo 79 does not fit H = 64: the op chain
        _e(4, 160, 7, 14, kind="chain"),                                # n_enc = 196: fused forward, library gradient pass
    ])
assert len({e.name for e in LATTICE}) == len(LATTICE)
BY_NAME = {e.name: e for e in LATTICE}
FUSED = [e.name for e in LATTICE if e.kind == "fused"]
FALLBACKS = [e.name for e in LATTICE if e.kind != "fused"]


def units_of(e):
    return e.L3 + 3 * e.L2


def n_enc_of(e):
    return e.F * units_of(e)


def k0_of(e):
    return n_enc_of(e) + 3 + 6 * N_FREQS


def roundup32(k):
    return (k + 31) // 32 * 32


def forward_fused(e):
    """`FusedFieldForward.supported` restated for a lattice entry: the shapes, and the unit table's 64 rows."""
    geo = min(127, max(15, e.F * 10 - 1))
    return e.F in (2, 4, 8) and e.H in (64, 160) and roundup32(17 + geo) <= e.H and units_of(e) <= MAX_UNITS


def chain_capable(e):
    """`_chain_ok`'s shape conditions: the chain writes dX in at most twelve 16-column blocks, four columns at a time."""
    return forward_fused(e) and n_enc_of(e) % 4 == 0 and n_enc_of(e) <= 192


CHAIN = [e.name for e in LATTICE if e.kind == "fused" and chain_capable(e)]


def _log2_tables(L3, L2, tables):
    r3, r2 = LADDER_3D[:L3], LADDER_2D[:L2]
    if tables == "mixed":               # the low levels dense (R^3 <= 2^10: R <= 10; R^2 <= 2^9: R <= 22), the rest hashed
        return 10, 9
    if tables == "dense":               # the smallest tables that hold the finest level whole
        return int(np.ceil(np.log2(max(r3) ** 3))), int(np.ceil(np.log2(max(r2) ** 2)))
    if tables == "hashed":              # smaller than the coarsest level: 5^3 = 125 > 2^6, 6^2 = 36 > 2^5
        return 6, 5
    raise ValueError(tables)


def composition(F, H, L3, L2, tables="mixed"):
    """Constructor arguments of NGPRadianceField_mygrid_2D3D for a lattice point."""
    t3, t2 = _log2_tables(L3, L2, tables)
    return dict(n_features_per_level=F, n_neurons=H, resolutions_list=LADDER_3D[:L3], log2_hashmap_size=t3,
                resolutions_list_2D=LADDER_2D[:L2], log2_hashmap_size_2D=t2)


def kwargs_of(e):
    return composition(e.F, e.H, e.L3, e.L2, e.tables)


def window_kinds(e):
    """What the 16-column halves of the feature row's 32-column chunks hold, decided as k_field_fused16w2 decides it
    (csrc/field_fused2.hip, the fill of layer 1) from the first and the last unit of the half: the set of
    "3d" (all 3-D units), "plane" (2-D units of one plane), "planes" (2-D units of several planes), "tail" (raw
    coordinates / sinusoids / padding only), "mixed" (anything else: the general window fill)."""
    enc_of = [0] * e.L3 + [1] * e.L2 + [2] * e.L2 + [3] * e.L2
    n_units, kinds = len(enc_of), set()
    for col0 in range(0, roundup32(k0_of(e)), 16):
        u_first, u_last = col0 // e.F, (col0 + 15) // e.F
        if u_first >= n_units:
            kinds.add("tail")
        elif u_last < n_units:
            e_first, e_last = enc_of[u_first], enc_of[u_last]
            if e_last == 0:
                kinds.add("3d")
            elif e_first != 0:
                kinds.add("plane" if e_first == e_last else "planes")
            else:
                kinds.add("mixed")
        else:
            kinds.add("mixed")
    return kinds


def straddling_pairs(e, window=8):
    """Number of (sin, cos) column pairs of the tail, three columns apart, that lie in different `window`-column windows."""
    U = n_enc_of(e)
    return sum(1 for k in range(N_FREQS) for a in range(3)
               if (U + 3 + 6 * k + a) // window != (U + 6 + 6 * k + a) // window)


def chain_blocks(e):
    """(16-column blocks of dX the chain's stage 0 writes, whether the last one is partial)."""
    n = n_enc_of(e)
    return (n + 15) // 16, n % 16 != 0


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def field_params(f):
    """What `reference_features` needs of a field module (host or device): per encoder (table, offsets, resolutions) as
    NumPy arrays, F, and the sinusoids' frequencies."""
    mb = f.mlp_base
    encs = [(e.params.detach().cpu().numpy(), e.offsets_list.cpu().numpy().astype(np.int32),
             e.resolutions_list.cpu().numpy().astype(np.int32)) for e in mb._encoders()]
    return dict(encoders=encs, F=int(mb.encoding_xyz.n_features),
                freqs=mb._freqs.detach().cpu().numpy().astype(np.float32))


def encoder_columns(params, x_unit, encode):
    """[N, F units] float32: `encode(x [N, D], signs, offsets, resolutions) -> [L, N, F]` once per encoder on its
    coordinate pair and its BINARISED table (STE_binary, ngp.py:24-39: +1 where the entry is >= 0), in feature-row order."""
    x_unit = np.ascontiguousarray(x_unit, np.float32)
    n, parts = x_unit.shape[0], []
    for (table, offs, res), dims in zip(params["encoders"], PLANE_DIMS):
        signs = np.where(table >= 0, 1.0, -1.0).astype(np.float32)
        out = encode(np.ascontiguousarray(x_unit[:, dims]), signs, offs, res)                 # [L, N, F]
        parts.append(np.transpose(np.asarray(out, np.float32), (1, 0, 2)).reshape(n, -1))
    return np.concatenate(parts, axis=1)


def reference_features(params, x_unit, oracle=None):
    """The first layer's input rows [N, roundup32(K0)] (float64 holding: float32 encoder features and coordinates exactly,
    float64 sin / cos of the FLOAT32 product x * freq — the kernels multiply in float32 —, zeros behind K0)."""
    if oracle is None:
        import oracle as oracle_
        oracle = oracle_
    x_unit = np.ascontiguousarray(x_unit, np.float32)
    enc = encoder_columns(params, x_unit,
                          lambda x, s, o, r: oracle.grid_encode_forward(x, s, o, r, threads=8))
    cols = [enc.astype(np.float64), x_unit.astype(np.float64)]
    for fr in params["freqs"]:
        arg = (x_unit * np.float32(fr)).astype(np.float64)
        cols += [np.sin(arg), np.cos(arg)]
    feat = np.concatenate(cols, axis=1)
    k0 = feat.shape[1]
    assert k0 == enc.shape[1] + 3 + 6 * len(params["freqs"])
    return np.concatenate([feat, np.zeros((feat.shape[0], roundup32(k0) - k0))], axis=1)


def table_gradients64(params, x_unit, dX64, oracle):
    """Float64 gradients of the four tables from the float64 gradient dX [N, n_enc] of the encoder columns:
    oracle.grid_encode_backward (gridencoder.cu:411-584, the STE mask of ngp.py:24-39 on the real-valued table) on dX sliced
    per encoder, its float64 accumulators."""
    x_unit = np.ascontiguousarray(x_unit, np.float32)
    n, F, col, out = x_unit.shape[0], params["F"], 0, []
    for (table, offs, res), dims in zip(params["encoders"], PLANE_DIMS):
        L = len(res)
        g = dX64[:, col:col + L * F].reshape(n, L, F).transpose(1, 0, 2).astype(np.float32)       # [L, N, F]
        _, acc = oracle.grid_encode_backward(np.ascontiguousarray(g), np.ascontiguousarray(x_unit[:, dims]), table, offs, res,
                                             ste_binary=True, want_acc64=True)
        out.append(acc)
        col += L * F
    assert col == dX64.shape[1]
    return out


def boundary_points(e, aabb_min=-1.5, aabb_ext=3.0):
    """World positions whose unit-cube coordinates lie on cell boundaries (x (R - 2) + 0.5 an integer) of the coarsest and
    the finest level of the 3-D grid and of the planes: floor() and the corner weights 0 / 1 at their edge."""
    pts = []
    for R in (LADDER_3D[0], LADDER_3D[e.L3 - 1], LADDER_2D[0], LADDER_2D[e.L2 - 1]):
        for k in (0, 1, (R - 2) // 2, R - 3):
            u = (k + 0.5) / (R - 2)
            pts.append([u, u, u])
            pts.append([u, 0.37, (R - 3 - k + 0.5) / (R - 2)])
    u = np.asarray(pts, np.float64)
    return (u * aabb_ext + aabb_min).astype(np.float32)
