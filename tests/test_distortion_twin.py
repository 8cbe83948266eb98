"""CPU: the distortion loss's NumPy twin (tests/distortion_twin.py) against itself — the float32 recurrences within the
derived bound of the float64 definition, the prefix-difference form far outside it on the offset case — and
`cnc_amd.nerfacc.losses.distortion` on CPU tensors against the twin: float32 within the bound, float64 at 1e-12, packed
and batched, gradcheck, the documented edge cases, the Trainer's option and its command-line flag."""
import numpy as np
import pytest
import torch

import distortion_twin as T

f32, f64 = np.float32, np.float64


def _contiguous(rng, S, lo=0.0, hi=4.0):
    edges = np.sort(rng.uniform(lo, hi, S + 1)).astype(f32)
    return edges[:-1].copy(), edges[1:].copy()


def _lindisp(S, near=0.05, far=1000.0):
    edges = (1.0 / np.linspace(1.0 / near, 1.0 / far, S + 1)).astype(f32)
    return edges[:-1].copy(), edges[1:].copy()


def _cases():
    rng = np.random.default_rng(5)
    out = {}
    for name, S, make in (("S33", 33, _contiguous), ("S64", 64, _contiguous), ("S1000", 1000, _contiguous)):
        out[name] = (rng.uniform(0, 1, S).astype(f32) ** 3,) + make(rng, S)
    out["S40_gaps"] = (rng.uniform(0, 0.1, 40).astype(f32),) + T.gapped_intervals(rng, 40)
    out["S256_lindisp"] = (rng.uniform(0, 0.02, 256).astype(f32),) + _lindisp(256)
    out["offset"] = T.offset_case(rng)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_recurrences_within_the_bound_of_the_definition(name):
    w, t0, t1 = CASES[name]
    S = w.size
    loss64, grad64 = T.direct64(w, t0, t1)
    loss32, grad32 = T.recurrence32(w, t0, t1)
    print(name, "loss", T.worst(loss32, loss64), "grad", T.worst(grad32, grad64), "bound", T.bound(S))
    assert loss64 > 0
    assert T.within(loss32, loss64, S) and T.within(grad32, grad64, S)


def test_prefix_difference_form_fails_the_offset_case():
    w, t0, t1 = CASES["offset"]
    loss64, _ = T.direct64(w, t0, t1)
    print("prefix-difference form:", T.worst(T.prefix_difference32(w, t0, t1), loss64), "bound", T.bound(w.size))
    assert not T.within(T.prefix_difference32(w, t0, t1), loss64, w.size)


def _pack(names, empty_at=()):
    """The named cases as one flattened call, with empty rays at the given positions."""
    rays = [CASES[n] for n in names]
    for at in empty_at:
        rays.insert(at, (np.zeros(0, f32),) * 3)
    cnts = np.array([r[0].size for r in rays], np.int64)
    starts = np.cumsum(cnts) - cnts
    cat = lambda k: np.concatenate([r[k] for r in rays]).astype(f32)      # noqa: E731
    return rays, cat(0), cat(1), cat(2), starts, cnts


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("how", ["packed_info", "ray_indices"])
def test_packed_cpu_tensors_against_the_twin(dtype, how):
    from cnc_amd.nerfacc.losses import distortion
    rays, w, t0, t1, starts, cnts = _pack(["S33", "S40_gaps", "offset", "S256_lindisp", "S64"], empty_at=(0, 3, 7))
    rng = np.random.default_rng(8)
    up = rng.normal(size=len(rays))
    up[1], up[2] = 0.0, -1.5
    wt = torch.tensor(w, dtype=dtype, requires_grad=True)
    kw = dict(packed_info=torch.from_numpy(np.stack([starts, cnts], -1))) if how == "packed_info" else \
        dict(ray_indices=torch.from_numpy(np.repeat(np.arange(len(rays)), cnts)), n_rays=len(rays))
    loss = distortion(wt, torch.tensor(t0, dtype=dtype), torch.tensor(t1, dtype=dtype), **kw)
    assert loss.shape == (len(rays),) and loss.dtype == dtype
    (loss * torch.tensor(up, dtype=dtype)).sum().backward()
    got_l, got_g = loss.detach().numpy(), wt.grad.numpy()
    for r, (rw, r0, r1) in enumerate(rays):
        want_l, want_g = T.direct64(rw, r0, r1)
        want_g = want_g * f64(up[r].astype(np.float32 if dtype == torch.float32 else f64))
        seg = slice(starts[r], starts[r] + cnts[r])
        if dtype == torch.float64:
            assert abs(got_l[r] - want_l) <= 1e-12 * abs(want_l)
            assert np.all(np.abs(got_g[seg] - want_g) <= 1e-12 * np.abs(want_g))
        else:
            assert T.within(got_l[r], want_l, cnts[r]), (r, T.worst(got_l[r], want_l))
            assert T.within(got_g[seg], want_g, cnts[r]), (r, T.worst(got_g[seg], want_g))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_batched_cpu_tensors_against_the_twin(dtype):
    from cnc_amd.nerfacc.losses import distortion
    rng = np.random.default_rng(9)
    S, lead = 40, (3, 5)
    rows = [(rng.uniform(0, 0.2, S).astype(f32),) + T.gapped_intervals(rng, S) for _ in range(15)]
    stack = lambda k: torch.tensor(np.stack([r[k] for r in rows]).reshape(*lead, S), dtype=dtype)     # noqa: E731
    wt = stack(0).requires_grad_(True)
    loss = distortion(wt, stack(1), stack(2))
    assert loss.shape == lead and loss.dtype == dtype
    loss.sum().backward()
    tol = 1e-12 if dtype == torch.float64 else T.bound(S)
    for r, (rw, r0, r1) in enumerate(rows):
        want_l, want_g = T.direct64(rw, r0, r1)
        assert abs(loss.detach().reshape(-1)[r].item() - want_l) <= tol * abs(want_l)
        assert np.all(np.abs(wt.grad.reshape(-1, S)[r].numpy() - want_g) <= tol * np.abs(want_g))


def test_gradcheck_on_the_float64_route():
    from cnc_amd.nerfacc.losses import distortion
    rng = np.random.default_rng(10)
    t0, t1 = (torch.tensor(x, dtype=torch.float64) for x in T.gapped_intervals(rng, 9))
    w = torch.tensor(rng.uniform(0.1, 1, 9), dtype=torch.float64, requires_grad=True)
    info = torch.tensor([[0, 4], [4, 0], [4, 5]])
    assert torch.autograd.gradcheck(lambda x: distortion(x, t0, t1, packed_info=info), (w,))
    wb = torch.tensor(rng.uniform(0.1, 1, (3, 3)), dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: distortion(x, t0.view(3, 3), t1.view(3, 3)), (wb,))


def test_no_gradient_to_t():
    from cnc_amd.nerfacc.losses import distortion
    t0 = torch.tensor([0.0, 1.0, 2.5], requires_grad=True)
    t1 = torch.tensor([0.5, 2.0, 3.0], requires_grad=True)
    w = torch.tensor([0.2, 0.3, 0.1], requires_grad=True)
    distortion(w[None], t0[None], t1[None]).sum().backward()
    assert t0.grad is None and t1.grad is None and w.grad is not None


def test_documented_edge_cases():
    from cnc_amd.nerfacc.losses import distortion
    # an empty ray gives 0; a ray of one sample gives w^2 d / 3
    w = torch.tensor([0.5, 0.25, 0.75], dtype=torch.float64, requires_grad=True)
    t0 = torch.tensor([1.0, 3.0, 4.0], dtype=torch.float64)
    t1 = torch.tensor([2.0, 3.5, 6.0], dtype=torch.float64)
    loss = distortion(w, t0, t1, packed_info=torch.tensor([[0, 0], [0, 1], [1, 0], [1, 2], [3, 0]]))
    pair = 2 * 0.25 * 0.75 * (5.0 - 3.25) + (0.25 ** 2 * 0.5 + 0.75 ** 2 * 2.0) / 3.0
    assert loss.tolist() == pytest.approx([0.0, 0.5 ** 2 * 1.0 / 3.0, 0.0, pair, 0.0], rel=1e-15)
    assert loss[0].item() == 0.0 and loss[2].item() == 0.0
    # no samples at all
    none = torch.zeros(0)
    assert distortion(none, none, none, ray_indices=torch.zeros(0, dtype=torch.int64), n_rays=4).tolist() == [0.0] * 4
    assert distortion(torch.zeros(2, 0), torch.zeros(2, 0), torch.zeros(2, 0)).tolist() == [0.0, 0.0]
    # all-zero weights: loss and gradient are exact zeros
    wz = torch.zeros(2, 7, requires_grad=True)
    edges = torch.arange(8.0)
    lz = distortion(wz, edges[:-1].expand(2, 7), edges[1:].expand(2, 7))
    lz.sum().backward()
    assert lz.tolist() == [0.0, 0.0] and not wz.grad.any()
    # the docstring's example
    ex = distortion(torch.tensor([.5, .5]), torch.tensor([0., 2.]), torch.tensor([1., 3.]),
                    ray_indices=torch.tensor([0, 0]), n_rays=1)
    assert ex.tolist() == pytest.approx([2 * .25 * 2.0 + .5 / 3.0], rel=1e-6)


def test_trainer_option_and_flag():
    from cnc_amd.train import build_parser, make_config_and_data
    from cnc_amd.trainer import TrainConfig
    assert TrainConfig().distortion_weight == 0.0
    ap = build_parser()
    assert ap.parse_args([]).distortion_weight == 0.0
    args = ap.parse_args(["--distortion-weight", "0.01", "--dataset", "procedural"])
    assert args.distortion_weight == 0.01
    _, cfg, _ = make_config_and_data(args, torch.device("cpu"))
    assert cfg.distortion_weight == 0.01


def test_render_helpers_take_with_samples_keyword_only():
    import inspect
    from cnc_amd import render
    for fn in (render.render_image_with_occgrid, render.render_image_with_propnet):
        p = inspect.signature(fn).parameters["with_samples"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
