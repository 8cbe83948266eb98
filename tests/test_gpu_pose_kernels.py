"""GPU: the two pose kernels (cnc_amd/csrc/pose.hip) through the C ABI, bit for bit against the float32 modes of their
twins (tests/pose_twin.py, which tests/test_pose_twin.py holds to finite differences and to their float64 modes), run
under every sentinel fill (tests/guarded.py, in the style of tests/test_gpu_footprint_rays.py), twice.

cnc_camera_pose_apply: C in {1, 3, 7} and {11, 64, 65, 200} (one thread per camera in blocks of 64: a full block, a second
block of one camera, four blocks); per camera a delta of zero, a rotation under the series' switch, at it, of
|omega| = 0.3 and up to pi, with and without a translation; zero delta gives the base table's bits (-0 entries included).

cnc_ray_pose_grad: rays of 0, 1, 64 and 65 samples among others, n_rays in {1, 64, 65, 1000} (one chunk of the fold less
than full, full, plus one; four chunks), C in {1, 3, 7}, one camera without rays, one camera holding all rays; C in
{11, 64, 65, 200} at n_rays in {65, 1000}: k_pose_fold_chunks' 64 threads stride over the cameras from C = 65 on, and
k_pose_fold_cameras' C * 6 elements need a second 64-lane block from C = 11 on; camera ids outside [0, C).  The
samples of a ray do not follow those of the ray before: there are holes before, between and behind the rays, and they
hold the fill — 0xFF reads as NaN, so a kernel that touched a hole would show it.

Measured on the MI355X at C >= 11: both kernels equal their float32 twins bit for bit; the float32 fold's distance from
its float64 mode is at most 0.020 of the (n_rays + 70) 2^-24 bound (n_rays = 65, C = 200), 0.0033 at n_rays = 1000."""
import numpy as np
import pytest
import torch

import pose_twin as P
from guarded import FILLS, Guarded, same_bits, under_fills, moved_with_fill
from test_pose_twin import _table

pytestmark = pytest.mark.gpu
f32, i64 = np.float32, np.int64


def _deltas(rng, C):
    d = np.zeros((C, 6), f32)
    kinds = [0.0, 1e-5, float(np.sqrt(P.SERIES_BELOW)), 0.3, 3.1, 2.0 ** -12.5, 1.0]
    for c in range(C):
        th = kinds[c % len(kinds)]
        w = rng.normal(size=3)
        d[c, :3] = (w / np.linalg.norm(w) * th).astype(f32)
        if c % 2 == 1 or C == 1:
            d[c, 3:] = (rng.normal(size=3) * 0.1).astype(f32)
    return d


# k_camera_pose_apply: one thread per camera, 64 per block — 64 fills the first block, 65 opens a second, 200 needs four
@pytest.mark.parametrize("C", [1, 3, 7, 11, 64, 65, 200])
def test_pose_apply_is_the_twin_bit_for_bit(cuda, C):
    from cnc_amd import _lib
    rng = np.random.default_rng(C)
    if C >= 7:                                               # every branch of the kernel is taken at this count
        t2 = (_deltas(np.random.default_rng(0), C)[:, :3].astype(np.float64) ** 2).sum(axis=1)
        assert (t2 == 0).any() and ((t2 > 0) & (t2 < P.SERIES_BELOW * 0.99)).any() and (t2 > 1.0).any()
        assert (t2[64:] == 0).any() == (C > 70) and (t2[64:] > 4.0).any() == (C > 67)      # ... in the later blocks too
    clean = _table(rng, C).astype(f32)
    signed = clean.copy()                                    # -0 in a rotation and in a translation entry: zero delta keeps them
    signed[0, 5] = -0.0
    signed[C - 1, 15] = -0.0
    for base, delta in ((clean, _deltas(rng, C)), (signed, np.zeros((C, 6), f32)),
                        (clean, np.roll(_deltas(rng, max(C, 7)), 2, axis=0)[:C])):
        def build(fill):
            return dict(base=Guarded(base, cuda, fill=fill), delta=Guarded(delta, cuda, fill=fill),
                        out=Guarded.empty((C, P.CAMERA_ROW), f32, cuda, fill=fill))

        def run(b):
            assert _lib.lib().cnc_camera_pose_apply(b["base"].ptr, b["delta"].ptr, C, b["out"].ptr, _lib.stream(cuda)) == 0

        res = under_fills(build, run)
        assert moved_with_fill(res) == []
        got = res[FILLS[0]]["out"]
        assert same_bits(got, under_fills(build, run, fills=(0xA5,))[0xA5]["out"]), "two runs differ"
        want = P.pose_apply(base, delta, f32)
        assert same_bits(got, want), np.abs(got.astype(np.float64) - want).max()
        if not delta.any():
            assert same_bits(got, base), "zero delta must leave the table's bits"
        else:
            # sanity of what was tested: the rotations stayed rotations, the other fields are copies
            keep = np.ones(P.CAMERA_ROW, bool)
            keep[4:16] = False
            assert same_bits(got[:, keep], base[:, keep])
            R = got[:, 4:16].reshape(C, 3, 4)[:, :, :3].astype(np.float64)
            assert np.abs(np.einsum("cij,ckj->cik", R, R) - np.eye(3)).max() <= 1e-5


def test_pose_apply_through_the_wrapper_and_its_checks(cuda):
    from cnc_amd.poses import CameraPoseRefiner, pose_apply
    rng = np.random.default_rng(3)
    base = torch.from_numpy(_table(rng, 4).astype(f32)).to(cuda)
    ref = CameraPoseRefiner(4, cuda)
    assert ref.delta.shape == (4, 6) and not ref.delta.any() and ref.delta.requires_grad
    assert torch.equal(ref.apply(base), base)
    with torch.no_grad():
        ref.delta[2, :3] = torch.tensor([0.1, -0.2, 0.05])
        ref.delta[2, 3:] = torch.tensor([0.3, 0.0, -0.1])
    out = ref.apply(base)
    want = P.pose_apply(base.cpu().numpy(), ref.delta.detach().cpu().numpy(), f32)
    assert same_bits(out, want)
    poses = ref.poses(base[:, 4:16].reshape(4, 3, 4))
    assert poses.shape == (4, 4, 4) and same_bits(poses[:, :3].reshape(4, 12), want[:, 4:16])
    assert torch.equal(poses[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], device=cuda).expand(4, 4))
    with pytest.raises(RuntimeError):
        pose_apply(base, ref.delta.data, out=base)
    with pytest.raises(RuntimeError, match="CUDA"):
        pose_apply(base.cpu(), ref.delta.data)


def _rays(rng, n_rays, C, ids_kind):
    """A ray table with holes, the fixed counts 0, 1, 64, 65 first.  -> dict of host arrays + `hole` (bool per sample)."""
    counts = rng.integers(0, 12, size=n_rays)
    counts[:4] = [0, 1, 64, 65][:min(4, n_rays)] if n_rays >= 4 else [65][:n_rays]
    gaps = rng.integers(0, 3, size=n_rays)
    gaps[0] = 2
    starts = np.cumsum(gaps + np.concatenate([[0], counts[:-1]]))
    n = int(starts[-1] + counts[-1]) + 3
    hole = np.ones(n, bool)
    for s, c in zip(starts, counts):
        hole[s:s + c] = False
    t0 = rng.uniform(0.5, 4.0, size=n).astype(f32)
    t1 = (t0 + rng.uniform(0.01, 0.1, size=n).astype(f32)).astype(f32)
    g_x = (rng.normal(size=(n, 3)) * np.exp(rng.normal(size=(n, 1)) * 2)).astype(f32)
    d = rng.normal(size=(n_rays, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    if ids_kind == "all_in_one":
        ids = np.full(n_rays, C - 1, i64)
    else:                                                    # camera 0 without rays (when there is another one)
        ids = rng.integers(min(1, C - 1), C, size=n_rays).astype(i64)
    if ids_kind == "some_outside":                           # below 0 and at or above C: clamped to the first / last camera
        for k, bad in zip(range(3, n_rays, max(1, n_rays // 9)), [-1, C, -(2 ** 40), C + 5, 2 ** 31, -7, 2 ** 62, C, -1]):
            ids[k] = bad
    return dict(g_x=g_x, t0=t0, t1=t1, starts=starts.astype(i64), counts=counts.astype(i64), d=d, ids=ids, hole=hole, n=n)


def _sums_of_abs_terms(v, C):
    """[C, 6]: per entry of G the sum of the absolute values of every term that enters it, in float64."""
    m = (v["t0"].astype(np.float64) + v["t1"].astype(np.float64)) * 0.5
    A, ids = np.zeros((C, 6)), np.clip(v["ids"], 0, C - 1)
    for r, (s, c) in enumerate(zip(v["starts"], v["counts"])):
        ag = np.abs(v["g_x"][s:s + c]).astype(np.float64)
        So, Sd = ag.sum(axis=0), (m[s:s + c, None] * ag).sum(axis=0)
        d = np.abs(v["d"][r]).astype(np.float64)
        A[ids[r], :3] += [d[1] * Sd[2] + d[2] * Sd[1], d[2] * Sd[0] + d[0] * Sd[2], d[0] * Sd[1] + d[1] * Sd[0]]
        A[ids[r], 3:] += So
    return A


def _poison(a, hole, fill):
    a = a.copy()
    a.reshape(a.shape[0], -1).view(np.uint8)[hole] = fill
    return a


# k_pose_fold_chunks: 64 threads, `c += 64` over the cameras — a second round from C = 65.  k_pose_fold_cameras: one lane
# per (camera, component), 64 per block — C = 11 is the first C with C * 6 > 64; 64, 65 and 200 give 6, 7 and 19 blocks.
FOLD_SIZES = [(n_rays, C) for C in (1, 3, 7) for n_rays in (1, 64, 65, 1000)] + \
             [(n_rays, C) for C in (11, 64, 65, 200) for n_rays in (65, 1000)]


@pytest.mark.parametrize("ids_kind", ["one_without", "all_in_one"])
@pytest.mark.parametrize("n_rays,C", FOLD_SIZES)
def test_ray_pose_grad_is_the_twin_bit_for_bit(cuda, n_rays, C, ids_kind):
    _check_ray_pose_grad(cuda, n_rays, C, ids_kind)


@pytest.mark.parametrize("n_rays,C", [(65, 3), (1000, 65)])
def test_ray_pose_grad_clamps_camera_ids_outside_the_table(cuda, n_rays, C):
    """A few cam_ids below 0 and at or above C (up to 2^62): the kernel clamps them to camera 0 / C - 1 as cnc_camera_rays
    does, and so does the twin; same references and bounds as above."""
    _check_ray_pose_grad(cuda, n_rays, C, "some_outside")


def _check_ray_pose_grad(cuda, n_rays, C, ids_kind):
    from cnc_amd import _lib
    L = _lib.lib()
    v = _rays(np.random.default_rng(n_rays * 10 + C), n_rays, C, ids_kind)
    nbytes = int(L.cnc_ray_pose_grad_workspace(n_rays, C))
    assert nbytes == 4 * 6 * (n_rays + (n_rays + 255) // 256 * C)

    def build(fill):
        return dict(g_x=Guarded(_poison(v["g_x"], v["hole"], fill), cuda, fill=fill),
                    t0=Guarded(_poison(v["t0"], v["hole"], fill), cuda, fill=fill),
                    t1=Guarded(_poison(v["t1"], v["hole"], fill), cuda, fill=fill),
                    starts=Guarded(v["starts"], cuda, fill=fill), counts=Guarded(v["counts"], cuda, fill=fill),
                    d=Guarded(v["d"], cuda, fill=fill), ids=Guarded(v["ids"], cuda, fill=fill),
                    ws=Guarded.empty((nbytes // 4,), f32, cuda, fill=fill).scratch(),
                    G=Guarded.empty((C, 6), f32, cuda, fill=fill))

    def run(b):
        rc = L.cnc_ray_pose_grad(b["g_x"].ptr, b["t0"].ptr, b["t1"].ptr, v["n"], b["starts"].ptr, b["counts"].ptr, b["d"].ptr,
                                 b["ids"].ptr, n_rays, C, b["ws"].ptr, nbytes, b["G"].ptr, _lib.stream(cuda))
        assert rc == 0

    res = under_fills(build, run)
    assert moved_with_fill(res) == [], "G depends on bytes outside the rays' samples"
    got = res[FILLS[0]]["G"]
    assert same_bits(got, under_fills(build, run, fills=(0xA5,))[0xA5]["G"]), "two runs differ"
    want = P.ray_pose_grad(v["g_x"], v["t0"], v["t1"], v["starts"], v["counts"], v["d"], v["ids"], C, f32)
    assert same_bits(got, want), np.abs(got.astype(np.float64) - want).max()
    if ids_kind == "all_in_one":
        assert np.all(got[:C - 1] == 0) and not np.signbit(got[:C - 1]).any() and np.all(got[C - 1] != 0)
    elif C > 1 and ids_kind == "one_without":
        assert np.all(got[0] == 0) and not np.signbit(got[0]).any(), "a camera without rays must get exact zeros"
    if ids_kind == "some_outside":
        assert (v["ids"] < 0).sum() >= 2 and (v["ids"] >= C).sum() >= 2
    idle = np.setdiff1d(np.arange(C), np.clip(v["ids"], 0, C - 1))
    assert np.all(got[idle] == 0) and not np.signbit(got[idle]).any(), "a camera without rays must get exact zeros"
    # the float32 fold's distance from its float64 mode, within the n - 1 roundings of its longest chain
    G64 = P.ray_pose_grad(v["g_x"], v["t0"], v["t1"], v["starts"], v["counts"], v["d"], v["ids"], C, np.float64)
    A64 = _sums_of_abs_terms(v, C)
    print(f"RAY POSE GRAD n_rays={n_rays} C={C} {ids_kind}: float32 against float64 "
          f"{float((np.abs(got - G64) / np.maximum(A64, 1e-30)).max()):.3e} of the sums of |terms|, "
          f"{float((np.abs(got - G64) / np.maximum((n_rays + 70) * 2.0 ** -24 * A64, 1e-300)).max()):.3g} of the bound")
    assert np.all(np.abs(got - G64) <= (n_rays + 70) * 2.0 ** -24 * A64)


def test_ray_pose_grad_wrapper_and_empty_calls(cuda):
    from cnc_amd.poses import ray_pose_grad
    v = _rays(np.random.default_rng(5), 300, 3, "one_without")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    G = ray_pose_grad(t(v["g_x"]), t(v["t0"]), t(v["t1"]), t(v["starts"]), t(v["counts"]), t(v["d"]), t(v["ids"]), 3)
    want = P.ray_pose_grad(v["g_x"], v["t0"], v["t1"], v["starts"], v["counts"], v["d"], v["ids"], 3, f32)
    assert same_bits(G, want)
    # no rays at all: every camera gets exact zeros
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=cuda)
    G0 = ray_pose_grad(z(0, 3), z(0), z(0), z(0, dt=torch.int64), z(0, dt=torch.int64), z(0, 3), z(0, dt=torch.int64), 3,
                       out=torch.full((3, 6), 7.0, device=cuda))
    assert torch.equal(G0, z(3, 6))
    with pytest.raises(RuntimeError):
        ray_pose_grad(t(v["g_x"]), t(v["t0"]), t(v["t1"]), t(v["starts"]).int(), t(v["counts"]), t(v["d"]), t(v["ids"]), 3)
