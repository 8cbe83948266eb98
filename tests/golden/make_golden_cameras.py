"""Golden numbers for the camera twin (tests/camera_twin.py), from the reference's own pure-torch helpers in
nerfacc/cameras.py: `_opencv_lens_undistortion`, `_opencv_lens_distortion` and `_opencv_lens_distortion_fisheye` (build
container only; the module is loaded with `nerfacc.cuda` stubbed, none of the three needs the native extension).

    python tests/golden/make_golden_cameras.py <root of the reference checkout>      # writes cameras.npz

Stored: seeded inputs — 4096 ideal points with |x| <= 1, |y| <= 0.75, pushed through the float64 forward model of the
twin and rounded to float32, so that a true inverse exists — and, per coefficient set, what the reference returned in
float32 (`undist_i`: 10 iterations at eps 1e-6; `dist_i`: the forward model on the float32 ideal points) with `ref_err`,
the largest absolute deviation of `undist_i` from the float64 twin on the same float32 inputs.  The fisheye fixture
(|x| <= 1.5, |y| <= 1.0, two coefficient sets) with the reference's forward model in float64, and the thin-prism
(layout 12) inputs, which have no reference.  Data only, nothing of the reference's source."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import camera_twin as T  # noqa: E402

N = 4096
SEED = 20
# k1 k2 p1 p2 k3 k4 k5 k6, zero-padded: the sets {k1}, {k1, k2}, {k1, k2, p1, p2}, all eight
SETS = [[-0.15], [-0.28, 0.07], [-0.28, 0.07, 2e-4, -1e-4], [0.12, -0.05, 5e-4, -3e-4, 0.01, 0.05, -0.02, 0.004]]
FISHEYE_SETS = [[-0.02, 0.003, -5e-4, 1e-4], [0.05, -0.01, 0.002, -3e-4]]
# k1..k6 p1 p2 s1..s4
PRISM = [0.12, -0.05, 0.01, 0.05, -0.02, 0.004, 5e-4, -3e-4, 1e-4, -2e-4, 3e-4, -1e-4]
EPS, ITERS = 1e-6, 10


def load_reference(ref_root):
    pkg = types.ModuleType("nerfacc")
    pkg.__path__ = [os.path.join(ref_root, "nerfacc")]
    stub = types.ModuleType("nerfacc.cuda")
    pkg.cuda = stub
    sys.modules["nerfacc"], sys.modules["nerfacc.cuda"] = pkg, stub
    spec = importlib.util.spec_from_file_location("nerfacc.cameras", os.path.join(ref_root, "nerfacc", "cameras.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["nerfacc.cameras"] = mod
    spec.loader.exec_module(mod)
    return mod


def main(ref_root):
    ref = load_reference(ref_root)
    rng = np.random.default_rng(SEED)
    ideal = np.stack([rng.uniform(-1.0, 1.0, N), rng.uniform(-0.75, 0.75, N)], -1)
    fish_ideal = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.0, 1.0, N)], -1)
    out = {"ideal": ideal, "fish_ideal": fish_ideal, "eps": np.float64(EPS), "iters": np.int64(ITERS),
           "n_sets": np.int64(len(SETS)), "n_fish": np.int64(len(FISHEYE_SETS))}
    worst = 0.0
    for i, coeffs in enumerate(SETS):
        p8 = np.zeros(8, np.float32)
        p8[:len(coeffs)] = coeffs
        uv = T.distort(ideal, p8.astype(np.float64)).astype(np.float32)
        got = ref._opencv_lens_undistortion(torch.from_numpy(uv), torch.from_numpy(p8[:len(coeffs)].copy()), EPS, ITERS)
        assert got.dtype == torch.float32
        want = T.undistort_newton(uv, p8, EPS, ITERS, np.float64)
        err = float(np.abs(got.numpy().astype(np.float64) - want).max())
        back = float(np.abs(want - ideal).max())          # the float32 rounding of uv moves the inverse by a few 1e-8
        worst = max(worst, err)
        dist = ref._opencv_lens_distortion(torch.from_numpy(ideal.astype(np.float32)), torch.from_numpy(p8))
        out.update({f"n_coeffs_{i}": np.int64(len(coeffs)), f"params_{i}": p8, f"uv_{i}": uv, f"undist_{i}": got.numpy(),
                    f"dist_{i}": dist.numpy(), f"ref_err_{i}": np.float64(err)})
        print(f"set {i}: reference float32 vs float64 twin {err:.3e} ({err * 2 ** 24:.2f} x 2^-24), "
              f"float64 inverse vs ideal {back:.3e}")
        exact = T.undistort_newton(T.distort(ideal, p8.astype(np.float64)), p8, 1e-14, 30, np.float64)
        print(f"        float64 inverse of the unrounded image vs ideal {np.abs(exact - ideal).max():.1e}")
    out["ref_err"] = np.float64(worst)
    for i, coeffs in enumerate(FISHEYE_SETS):
        k = np.asarray(coeffs, np.float32)
        uv = T.distort_fisheye(fish_ideal, k.astype(np.float64)).astype(np.float32)
        dist = ref._opencv_lens_distortion_fisheye(torch.from_numpy(fish_ideal), torch.from_numpy(k.astype(np.float64)))
        assert dist.dtype == torch.float64
        out.update({f"fish_params_{i}": k, f"fish_uv_{i}": uv, f"fish_dist_{i}": dist.numpy()})
    p12 = np.asarray(PRISM, np.float32)
    out.update(prism_params=p12, prism_uv=T.distort12(ideal, p12.astype(np.float64)).astype(np.float32))
    path = os.path.join(HERE, "cameras.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "ref_err", worst)


if __name__ == "__main__":
    main(sys.argv[1])
