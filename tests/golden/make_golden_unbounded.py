"""Golden vectors for the UNBOUNDED radiance field (`unbounded=True`: contract_to_unisphere, ngp.py:337-361,515-516),
produced like field_toy{,_sh16}.npz: the reference's own `NGPRadianceField_mygrid_2D3D` run on CPU through the oracle
stand-ins of make_golden_field.py (build container only).

    python tests/golden/make_golden_unbounded.py          # writes field_unbounded_toy.npz

Cases `f8` and `f2` of FIELD_CASES, 512 positions of the unbounded tests' shared point set (tests/contract_twin.py:
uniform in 1.2 x the box, normal x 10 extents, normal x 1e4, the exact cases) in an asymmetric box, both conventions of
the direction encoding's output precision (keys `sh32_...`: the float32 stand-in, `sh16_...`: tiny-cuda-nn's half
output).  Stored: the seeds the inputs are regenerated from, the state dict's key names and shapes, and the numbers the
reference returned — no positions, no parameters, nothing of the reference's source.  (`sh16_...`: outputs, loss and the
head's gradients; `sh32_...`: every gradient.)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import contract_twin as T  # noqa: E402
from make_golden_field import FIELD_CASES, _SHStub, fill_state, import_reference  # noqa: E402

N, POINT_SEED, INPUT_SEED, STATE_SEED = 512, 31, 37, 17


def inputs(n=N):
    """(positions, directions, rgb weights, density weights) — the same function lives in the GPU test."""
    pos = T.points(n, seed=POINT_SEED)
    rng = np.random.default_rng(INPUT_SEED)
    dirs = rng.normal(size=(n, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
    return pos, dirs, rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 1)).astype(np.float32)


def main():
    ngp = import_reference()[0]
    out = {"n": np.int64(N), "point_seed": np.int64(POINT_SEED), "input_seed": np.int64(INPUT_SEED),
           "state_seed": np.int64(STATE_SEED), "aabb": T.BOX.copy()}
    pos, dirs, w_rgb, w_sig = inputs()
    for tag, dtype in (("sh32", None), ("sh16", torch.float16)):
        _SHStub.output_dtype = dtype
        for name, kw in FIELD_CASES.items():
            torch.manual_seed(3)
            f = ngp.NGPRadianceField_mygrid_2D3D(aabb=torch.from_numpy(T.BOX.copy()), unbounded=True, ste_binary=True,
                                                 ste_multistep=False, add_noise=False, Q=10, **kw)
            assert f.unbounded
            sd = f.state_dict()
            out[f"{name}_keys"] = np.array(list(sd.keys()))
            out[f"{name}_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
            f.load_state_dict(fill_state(sd, seed=STATE_SEED), strict=True)
            x, v = torch.from_numpy(pos), torch.from_numpy(dirs)
            density = f.query_density(x)
            rgb, sigma = f(x, v)
            loss = (rgb * torch.from_numpy(w_rgb)).sum() + (sigma * torch.from_numpy(w_sig)).sum()
            f.zero_grad()
            loss.backward()
            p = f"{tag}_{name}"
            out.update({f"{p}_density": density.detach().numpy(), f"{p}_rgb": rgb.detach().numpy(),
                        f"{p}_sigma": sigma.detach().numpy(), f"{p}_loss": np.float64(loss.item())})
            for k, q in f.named_parameters():
                # the half-precision run keeps the head's gradients only (where the harmonics enter, and what tells the two
                # conventions apart): the fixture stays under the size limit for committed files
                if tag == "sh32" or k.startswith("mlp_head."):
                    out[f"{p}_grad_{k}"] = q.grad.numpy().copy()
            print(p, "loss", loss.item(), "density max", float(density.max()), "zero densities", int((density == 0).sum()))
    _SHStub.output_dtype = None
    path = os.path.join(HERE, "field_unbounded_toy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
