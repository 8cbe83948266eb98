"""Golden numbers for the proposal-network twin (tests/propnet_twin.py), from the reference's own pure-torch helpers in
nerfacc/estimators/prop_net.py: `_outer` (its independent measure of the outer weights), `_transform_stot` and
`get_proposal_requires_grad_fn` (build container only; none of them needs the reference's native extension).

    python tests/golden/make_golden_propnet.py <root of the reference checkout>      # writes propnet_outer.npz

Stored: the seeds and shapes the inputs are regenerated from (propnet_twin.histograms, and `transform_inputs` below)
and the numbers the reference returned: `_outer` in float64 on seeded histograms with ties and clamped ends,
`_transform_stot` in float64 for both spacings, the schedule's booleans for steps 0..2499.  No inputs, nothing of the
reference's source."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import propnet_twin as P  # noqa: E402

# (seed, n_rays, key edges, query edges)
OUTER_CASES = [(1, 8, 2, 2), (2, 8, 3, 17), (3, 10, 33, 17), (4, 10, 65, 65), (5, 10, 33, 130), (6, 6, 600, 65)]
SCHEDULES = [(5.0, 1000), (2.0, 10)]
N_STEPS = 2500
TRANSFORM_SEED, TRANSFORM_N = 9, 256
RANGES = [(1.0, 10.0), (0.05, 1000.0), (2.0, 6.0)]


def transform_inputs():
    """s in [0, 1], both ends included (float64)."""
    s = np.random.default_rng(TRANSFORM_SEED).uniform(0.0, 1.0, TRANSFORM_N)
    s[0], s[-1] = 0.0, 1.0
    return s


def main(ref_root):
    sys.path.insert(0, ref_root)
    from nerfacc.estimators.prop_net import _outer, _transform_stot, get_proposal_requires_grad_fn
    out = {"outer_cases": np.asarray(OUTER_CASES, np.int64), "n_steps": np.int64(N_STEPS),
           "schedules": np.asarray(SCHEDULES, np.float64), "transform_seed": np.int64(TRANSFORM_SEED),
           "transform_n": np.int64(TRANSFORM_N), "ranges": np.asarray(RANGES, np.float64)}
    for i, (seed, n_rays, n_key, n_query) in enumerate(OUTER_CASES):
        key, cdf, q = (torch.from_numpy(x) for x in P.histograms(seed, n_rays, n_key, n_query))
        got = _outer(q[:, :-1], q[:, 1:], key[:, :-1], key[:, 1:], torch.diff(cdf, dim=-1))
        assert got.dtype == torch.float64 and got.shape == (n_rays, n_query - 1)
        out[f"outer_{i}"] = got.numpy()
    s = torch.from_numpy(transform_inputs())
    for j, (t_min, t_max) in enumerate(RANGES):
        lo, hi = torch.tensor(t_min, dtype=torch.float64), torch.tensor(t_max, dtype=torch.float64)
        for kind in ("uniform", "lindisp"):
            out[f"stot_{kind}_{j}"] = _transform_stot(kind, s, lo, hi).numpy()
    for j, (target, num_steps) in enumerate(SCHEDULES):
        fn = get_proposal_requires_grad_fn(target, int(num_steps))
        out[f"schedule_{j}"] = np.packbits(np.asarray([fn(step) for step in range(N_STEPS)], bool))
    path = os.path.join(HERE, "propnet_outer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
