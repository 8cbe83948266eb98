"""CPU-only tests of the host-side logic (no kernels): table construction, the nerfacc Python layer
against the reference (golden vectors from tests/golden/make_golden.py), the range coder, and the
context-model tables."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_gridencoder_tables_match_reference_class():
    """Offsets / resolutions / parameter shape of GridEncoder == the reference class (ngp.py:197-223)."""
    from cnc_amd.gridencoder import GridEncoder
    g = np.load(os.path.join(GOLD, "gridencoder_glue.npz"))
    cfgs = [dict(num_dim=3, n_features=4, resolutions_list=(6, 9, 14, 20, 31, 44), log2_hashmap_size=10),
            dict(num_dim=2, n_features=8, resolutions_list=(10, 18, 34, 66), log2_hashmap_size=9),
            dict(num_dim=3, n_features=2, resolutions_list=(6, 9, 14), log2_hashmap_size=12)]
    for k, cfg in enumerate(cfgs):
        enc = GridEncoder(**cfg)
        assert enc.offsets_list.dtype == torch.int32
        assert np.array_equal(enc.offsets_list.numpy(), g[f"g{k}_offsets"])
        assert np.array_equal(enc.resolutions_list.numpy(), g[f"g{k}_res"])
        assert tuple(enc.params.shape) == g[f"g{k}_params"].shape
        assert enc.params.abs().max() <= 1e-4


def test_reference_composition_table_sizes():
    """SURVEY §8 header: 4,003,896 3-D rows, 345,616 rows per plane, 6,120,776 for the 16L bench grid."""
    from cnc_amd import synthetic
    assert synthetic.level_offsets(synthetic.RES_3D_REF, 19, 3).tolist() == [
        0, 5832, 19656, 55600, 140784, 346168, 858168, 1382456, 1906744, 2431032, 2955320, 3479608, 4003896]
    assert synthetic.level_offsets(synthetic.RES_2D_REF, 17, 2).tolist() == [0, 16904, 83472, 214544, 345616]
    assert int(synthetic.level_offsets(synthetic.RES_16L, 19, 3)[-1]) == 6120776


def test_ste_binary_known_answers():
    from cnc_amd.gridencoder import STE_binary
    g = np.load(os.path.join(GOLD, "gridencoder_glue.npz"))
    v = torch.tensor(g["ste_in"], requires_grad=True)
    s = STE_binary.apply(v)
    s.backward(torch.arange(1.0, 10.0))
    assert np.array_equal(s.detach().numpy(), g["ste_out"])
    assert np.array_equal(v.grad.numpy(), g["ste_grad"])


def test_occ_grid_update_matches_reference():
    """OccGridEstimator._update on CPU with the reference's seed reproduces its occs / binaries."""
    from cnc_amd.nerfacc import OccGridEstimator
    g = np.load(os.path.join(GOLD, "occ_grid.npz"))
    est = OccGridEstimator([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], resolution=16, levels=1)
    est.train()
    occ_fn = lambda x: torch.exp(-4.0 * (x ** 2).sum(-1, keepdim=True)) * 0.05
    torch.manual_seed(123)
    for step in (0, 16, 256, 272):
        est._update(step=step, occ_eval_fn=occ_fn, occ_thre=0.01, ema_decay=0.95, warmup_steps=256)
        assert np.array_equal(est.occs.numpy(), g[f"occs_{step}"])
        assert np.array_equal(est.binaries.numpy(), g[f"bin_{step}"])
    est.eval()
    with pytest.raises(RuntimeError):
        est.update_every_n_steps(0, occ_fn)


def test_ray_aabb_torch_twin_and_enlarge():
    from cnc_amd.nerfacc.estimators.occ_grid import OccGridEstimator
    from cnc_amd.nerfacc.grid import _ray_aabb_intersect
    g = np.load(os.path.join(GOLD, "ray_aabb.npz"))
    for k in range(3):
        near, far, miss = (float(v) for v in g[f"nfm_{k}"])
        t0, t1, h = _ray_aabb_intersect(torch.from_numpy(g["rays_o"]), torch.from_numpy(g["rays_d"]),
                                        torch.from_numpy(g["aabbs"]), near, far, miss)
        assert np.array_equal(h.numpy(), g[f"hit_{k}"])
        assert np.array_equal(t0.numpy(), g[f"t0_{k}"]) and np.array_equal(t1.numpy(), g[f"t1_{k}"])
    # nested levels: level k covers the region of interest scaled by 2^k about its centre (occ_grid.py:64-70)
    est = OccGridEstimator([-1.5, -1.0, -0.5, 1.5, 2.0, 2.5], resolution=4, levels=3)
    assert est.aabbs[0].tolist() == [-1.5, -1.0, -0.5, 1.5, 2.0, 2.5]
    assert est.aabbs[1].tolist() == [-3.0, -2.5, -2.0, 3.0, 3.5, 4.0]
    assert est.aabbs[2].tolist() == [-6.0, -5.5, -5.0, 6.0, 6.5, 7.0]


def test_batched_volrend_and_scans_cpu():
    """Batched (non-packed) branches run on plain torch, like the reference."""
    import cnc_amd.nerfacc as n
    x = torch.tensor([[1., 2., 3.], [4., 5., 6.]])
    assert n.inclusive_sum(x).tolist() == [[1, 3, 6], [4, 9, 15]]
    assert n.exclusive_sum(x).tolist() == [[0, 1, 3], [0, 4, 9]]
    assert n.exclusive_prod(x).tolist() == [[1, 1, 2], [1, 4, 20]]
    alphas = torch.tensor([[0.4, 0.8, 0.1]])
    w, tr = n.render_weight_from_alpha(alphas)
    assert torch.allclose(tr, torch.tensor([[1.0, 0.6, 0.12]])) and torch.allclose(w, torch.tensor([[0.4, 0.48, 0.012]]))
    vis = n.render_visibility_from_alpha(alphas, early_stop_eps=0.3, alpha_thre=0.2)
    assert vis.tolist() == [[True, True, False]]
    acc = n.accumulate_along_rays(w, torch.ones(1, 3, 2))
    assert torch.allclose(acc, w.sum(-1, keepdim=True).expand(1, 2))
    assert n.pack_info(torch.tensor([0, 0, 1, 1, 1, 2, 2, 2, 2]), 3).tolist() == [[0, 2], [2, 3], [5, 4]]
    assert n.pack_info(torch.tensor([], dtype=torch.long), 2).tolist() == [[0, 0], [0, 0]]


def test_product_range_coder_equals_oracle_bytes(oracle, tmp_path):
    """libcnc_codec.so emits exactly the oracle's byte stream and decodes it back."""
    from cnc_amd.context import decoder, encoder
    rng = np.random.default_rng(5)
    for n in (1, 7, 4096, 200001):
        p = rng.uniform(1e-6, 1 - 1e-6, size=n).astype(np.float32)
        if n > 100:
            p[:50] = 1e-6
            p[50:100] = 1 - 1e-6
        x = np.where(rng.uniform(size=n) < p, 1.0, -1.0).astype(np.float32)
        f = str(tmp_path / f"s{n}.b")
        bits = encoder(torch.from_numpy(x), torch.from_numpy(p), f)
        stream = open(f, "rb").read()
        assert bits == 8 * len(stream)
        assert stream == oracle.rc_encode(p, ((x + 1) // 2).astype(np.int16))
        back = decoder(torch.from_numpy(p), f)
        assert back.dtype == torch.float32 and np.array_equal(back.numpy(), x)
    with pytest.raises(AssertionError):
        encoder(torch.ones(1), torch.full((1,), 0.5), "x.bin")


def test_get_grid_index_twin(oracle):
    from cnc_amd.context import get_grid_index
    g = np.load(os.path.join(GOLD, "grid_index.npz"))
    for k in range(int(g["n_cases"])):
        D, R, hs = int(g[f"c{k}_D"]), int(g[f"c{k}_R"]), int(g[f"c{k}_hs"])
        got = get_grid_index(hs, R, torch.from_numpy(g[f"c{k}_pos"].astype(np.int64)))
        assert np.array_equal(got.numpy(), g[f"c{k}_rows"])


def test_context_model_tables_toy():
    """Vertex-by-slot tables: every vertex appears once, grouped by the slot the kernel hash sends it
    to; counts/cumsums consistent; sample allocation sums to ~sample_num."""
    from cnc_amd.context import CNC_context_models, get_grid_index
    torch.manual_seed(0)
    res = [6, 9, 14, 20, 31, 44]
    m = CNC_context_models(resolutions_list=res, resolutions_list_2D=[10, 18, 34, 66], log2_hashmap_size=10,
                           log2_hashmap_size_2D=9, n_features=4, sample_num=500, Pg_level=6, Pg_level_2D=4,
                           Rb=8, skip_levels_3D=(0, 1, 2), skip_levels_2D=(0,), device="cpu",
                           dimension_wise_resolution=34)
    assert m.offsets_list.tolist() == [0, 216, 952, 1976, 3000, 4024, 5048]
    assert m.n_levels_thresh == 2 and float(m.resolution_thresh) == 9.0
    for n, R in enumerate(res):
        pos = m.pos_grid_sorted_list[n]
        assert pos.shape == (R ** 3, 3) and pos.dtype == torch.int16
        hs = int(m.offsets_list[n + 1] - m.offsets_list[n])
        slots = get_grid_index(hs, R, pos.long())
        nslots = int(m.hashparams_num_levels[n])
        cnt = m.unique_count_list[n, :nslots]
        cum = m.unique_count_cumsum_list[n, :nslots + 1]
        assert int(cnt.sum()) == R ** 3 and int(cum[-1]) == R ** 3
        assert torch.equal(cum[1:] - cum[:-1], cnt)
        # vertices of slot k occupy pos[cum[k]:cum[k+1]] and all hash to unique_value[k]
        expect = torch.repeat_interleave(m.unique_value_list[n], cnt)
        assert torch.equal(slots, expect)
        assert torch.unique(pos.long() @ torch.tensor([R * R, R, 1])).numel() == R ** 3
    assert abs(int(m.sample_num_levels.sum()) - 500) <= 3
    assert m.ttl_sample_num_valid_levels == int(m.sample_num_levels[3:].sum())
    # occupied-cell vertex lattice for the dimension-wise context
    bv = torch.zeros(1, 8, 8, 8, dtype=torch.bool)
    bv[0, 2, 3, 1] = True
    c = m.get_idx_coords2(bv)
    t = (34 - 2) // 8
    assert c.shape == ((t + 2) ** 3, 3)
    assert c.min(0).values.tolist() == [2 * t, 3 * t, 1 * t] and c.max(0).values.tolist() == [3 * t + 1, 4 * t + 1, 2 * t + 1]
    assert c.dtype == torch.int32
    # the candidate lattice was built for resolution 34 (factor 4): another resolution has no meaning here and is
    # refused rather than answered differently by the two branches
    with pytest.raises(ValueError, match="does not match the lattice"):
        m.get_idx_coords2(bv, resolution=18)


def test_nerf_synthetic_loader_on_a_fabricated_scene(tmp_path):
    """PIL-based SubjectLoader: ray formula (OpenGL camera, nerf_synthetic.py:200-223), white
    compositing at test time, random rays in training."""
    import json
    from PIL import Image
    from cnc_amd.datasets import SubjectLoader
    root = tmp_path / "nerf_synthetic" / "lego"
    (root / "train").mkdir(parents=True)
    H = W = 8
    frames = []
    rng = np.random.default_rng(0)
    for i in range(3):
        rgba = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
        Image.fromarray(rgba, "RGBA").save(root / "train" / f"r_{i}.png")
        c2w = np.eye(4)
        c2w[:3, 3] = [0.0, 0.0, 4.0 + i]
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": c2w.tolist()})
    for split in ("train", "test"):
        json.dump({"camera_angle_x": 0.6911, "frames": frames}, open(root / f"transforms_{split}.json", "w"))
    ds = SubjectLoader("lego", str(tmp_path / "nerf_synthetic"), "train", num_rays=64)
    assert len(ds) == 3 and ds.training
    d = ds[0]
    assert d["pixels"].shape == (64, 3) and d["rays"].origins.shape == (64, 3)
    assert torch.allclose(d["rays"].viewdirs.norm(dim=-1), torch.ones(64), atol=1e-6)
    ds.update_num_rays(10)
    assert ds[1]["pixels"].shape == (10, 3)
    te = SubjectLoader("lego", str(tmp_path / "nerf_synthetic"), "test")
    t0 = te[0]
    assert t0["pixels"].shape == (H, W, 3) and t0["rays"].viewdirs.shape == (H, W, 3)
    focal = 0.5 * W / np.tan(0.5 * 0.6911)
    # centre-most pixel (x=4, y=4): camera dir ((4-4+.5)/f, -(4-4+.5)/f, -1), identity rotation
    want = np.array([0.5 / focal, -0.5 / focal, -1.0]); want /= np.linalg.norm(want)
    assert np.allclose(t0["rays"].viewdirs[4, 4].numpy(), want, atol=1e-6)
    assert torch.equal(t0["rays"].origins[0, 0], torch.tensor([0.0, 0.0, 4.0]))
    img = np.asarray(Image.open(root / "train" / "r_0.png"), np.float32) / 255.0
    assert np.allclose(t0["pixels"].numpy(), img[..., :3] * img[..., 3:] + (1 - img[..., 3:]), atol=1e-6)


def test_plan_binned_levels_host_only():
    """The level plan of the binned backward is made from HOST lists (no device reads): finest levels
    with resolution >= 400 and >= 2^16 rows, as a suffix of the level list."""
    from cnc_amd.backends.gridencoder_backend import plan_binned_levels
    from cnc_amd.synthetic import RES_16L, RES_3D_REF, level_offsets
    off16 = level_offsets(RES_16L, 19, 3)
    assert plan_binned_levels(RES_16L, off16, 3, 8, 1 << 20) == (6, 1 << 19)
    assert plan_binned_levels(RES_16L, off16, 3, 8, 1 << 20, min_resolution=1000) == (3, 1 << 19)
    assert plan_binned_levels(RES_16L, off16, 3, 8, 1 << 15) is None          # too few points to pay
    assert plan_binned_levels(RES_16L, off16, 3, 16, 1 << 20) is None         # F = 16: atomic kernel only
    assert plan_binned_levels(RES_16L, off16, 2, 8, 1 << 20) is None          # planes stay on atomics
    off12 = level_offsets(RES_3D_REF, 19, 3)
    n, rows = plan_binned_levels(RES_3D_REF, off12, 3, 8, 1 << 18, min_work=0)
    assert rows == 1 << 19 and n == sum(1 for r in RES_3D_REF if r >= 400) == 1
    # samples x binned levels below 1.5 M: the bin pass would be a handful of blocks, the atomic kernel takes the call
    assert plan_binned_levels(RES_3D_REF, off12, 3, 8, 1 << 18) is None and plan_binned_levels(RES_3D_REF, off12, 3, 8, 1 << 20) is None
    assert plan_binned_levels(RES_16L, off16, 3, 8, 1 << 17) is None and plan_binned_levels(RES_16L, off16, 3, 8, 1 << 18) == (6, 1 << 19)
    # a coarse level after a fine one breaks the suffix
    assert plan_binned_levels([600, 20], [0, 1 << 19, (1 << 19) + 8000], 3, 8, 1 << 20) is None


def test_mark_invisible_cells_matches_reference():
    """tests/golden/render.npz: the reference's OccGridEstimator.mark_invisible_cells on seeded cameras."""
    from cnc_amd.nerfacc import OccGridEstimator
    g = np.load(os.path.join(GOLD, "render.npz"))
    est = OccGridEstimator(roi_aabb=[-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], resolution=12, levels=2)
    W, H = (int(v) for v in g["mic_WH"])
    est.mark_invisible_cells(torch.from_numpy(g["mic_K"]), torch.from_numpy(g["mic_c2w"]), W, H,
                             near_plane=float(g["mic_near"]), chunk=500)
    assert np.array_equal(est.occs.numpy(), g["mic_occs"])
    assert (est.occs < 0).any() and (est.occs == 0).any()
    # cells marked invisible are never picked for an update
    assert all((est.occs[k * est.cells_per_lvl + idx] >= 0).all() for k, idx in enumerate(est._get_all_cells()))


def test_rendering_generic_route_on_cpu_matches_reference():
    """`rendering` / `render_weight_from_density` on CPU tensors (batched layout and flattened-with-
    ray_indices layout) against the reference's outputs in tests/golden/render.npz."""
    import cnc_amd.nerfacc as n
    g = np.load(os.path.join(GOLD, "render.npz"))
    t0, t1, sg, rgb = (torch.from_numpy(g[k]) for k in ("t_starts", "t_ends", "sigmas", "rgbs"))
    R, M = sg.shape
    w, tr, al = n.render_weight_from_density(t0, t1, sg)                      # batched
    assert torch.allclose(w, torch.from_numpy(g["plain_weights"]), rtol=1e-6, atol=1e-9)
    ri = torch.arange(R).repeat_interleave(M)
    w2, tr2, al2 = n.render_weight_from_density(t0.reshape(-1), t1.reshape(-1), sg.reshape(-1), ray_indices=ri, n_rays=R)
    assert torch.allclose(w2.view(R, M), torch.from_numpy(g["plain_weights"]), rtol=1e-6, atol=1e-9)
    col, op, dep, extras = n.rendering(t0.reshape(-1), t1.reshape(-1), ri, n_rays=R,
                                       rgb_sigma_fn=lambda a, b, c: (rgb.reshape(-1, 3), sg.reshape(-1), None),
                                       render_bkgd=torch.from_numpy(g["bkgd"]))
    assert torch.allclose(col, torch.from_numpy(g["plain_colors_bkgd"]), rtol=1e-5, atol=1e-6)
    assert torch.allclose(op, torch.from_numpy(g["plain_opacity"]), rtol=1e-5, atol=1e-6)
    assert torch.allclose(dep, torch.from_numpy(g["plain_depth"]), rtol=1e-5, atol=1e-6)
    assert set(extras) == {"weights", "alphas", "trans", "sigmas", "rgbs", "positions"}


def test_context_table_disk_cache_roundtrip(tmp_path):
    """the per-level sorted vertex tables come back from the on-disk cache identical to a
    fresh build (same seed -> same shuffle of the dense levels, which is applied after loading); a corrupt
    file is a cache miss."""
    from cnc_amd.context import CNC_context_models
    kw = dict(resolutions_list=[6, 9, 14, 20, 31], resolutions_list_2D=[10, 18, 34], log2_hashmap_size=10,
              log2_hashmap_size_2D=9, n_features=2, sample_num=300, Pg_level=5, Pg_level_2D=3, Rb=8,
              skip_levels_3D=(0, 1), skip_levels_2D=(0,), device="cpu", dimension_wise_resolution=18)
    torch.manual_seed(3)
    fresh = CNC_context_models(**kw)
    torch.manual_seed(3)
    first = CNC_context_models(**kw, table_cache_dir=str(tmp_path))          # builds + writes
    files = sorted(os.listdir(tmp_path))
    assert len(files) == 5 and all(f.startswith("ctx_level_R") and f.endswith(".pt") for f in files)
    (tmp_path / files[0]).write_bytes(b"not a table")                           # corrupt one level
    torch.manual_seed(3)
    cached = CNC_context_models(**kw, table_cache_dir=str(tmp_path))         # 4 hits, 1 rebuild
    for m in (first, cached):
        for a, b in zip(fresh.pos_grid_sorted_list, m.pos_grid_sorted_list):
            assert torch.equal(a, b)
        for a, b in zip(fresh.unique_value_list, m.unique_value_list):
            assert torch.equal(a, b)
        assert torch.equal(fresh.unique_count_cumsum_list, m.unique_count_cumsum_list)
        assert torch.equal(fresh.unique_count_list, m.unique_count_list)
    assert os.path.getsize(tmp_path / files[0]) > 100                            # rewritten


def test_tanks_loader_on_a_fabricated_scene(tmp_path):
    """SubjectLoader_Tanks (NSVF layout): OpenCV camera (y down, +z forward), file-name split, bbox -> aabb * 1.2
    and the step-size rule (tanks.py:135-137)."""
    from PIL import Image
    from cnc_amd.datasets import SubjectLoader_Tanks
    root = tmp_path / "TanksAndTemple" / "Barn"
    (root / "rgb").mkdir(parents=True)
    (root / "pose").mkdir()
    H, W = 6, 10
    rng = np.random.default_rng(1)
    for name in ("0_a", "0_b", "1_a"):
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), "RGB").save(root / "rgb" / f"{name}.png")
        c2w = np.eye(4)
        c2w[:3, 3] = [0.5, -0.25, -3.0]
        np.savetxt(root / "pose" / f"{name}.txt", c2w)
    np.savetxt(root / "intrinsics.txt", np.array([[20.0, 0, W / 2, 0], [0, 20.0, H / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))
    np.savetxt(root / "bbox.txt", np.array([[-1.0, -2.0, -0.5, 1.0, 2.0, 0.5, 0.2]]))
    tr = SubjectLoader_Tanks("Barn", str(tmp_path / "TanksAndTemple"), "train", num_rays=32)
    te = SubjectLoader_Tanks("Barn", str(tmp_path / "TanksAndTemple"), "test")
    assert len(tr) == 2 and len(te) == 1 and tr.training and not te.training
    assert torch.allclose(tr.aabb, torch.tensor([-1.2, -2.4, -0.6, 1.2, 2.4, 0.6])) and tr.render_step_size == 4e-3
    d = te[0]
    assert d["pixels"].shape == (H, W, 3) and torch.equal(d["color_bkgd"], torch.ones(3))
    # RGB images read as opaque RGBA: the pixel is the image colour
    img = np.asarray(Image.open(root / "rgb" / "1_a.png"), np.float32) / 255.0
    assert np.allclose(d["pixels"].numpy(), img, atol=1e-6)
    want = np.array([(3 - W / 2 + 0.5) / 20.0, (2 - H / 2 + 0.5) / 20.0, 1.0]); want /= np.linalg.norm(want)
    assert np.allclose(d["rays"].viewdirs[2, 3].numpy(), want, atol=1e-6)          # row y=2, column x=3; y points down
    assert torch.equal(d["rays"].origins[0, 0], torch.tensor([0.5, -0.25, -3.0]))
    assert tr[0]["pixels"].shape == (32, 3)


def test_fused_optimizer_step_drops_version_keyed_caches():
    """torch.optim.Adam(fused=True) updates parameters WITHOUT bumping Tensor._version (checked here), the key
    of the encoders' packed sign planes: cnc_amd._caches marks them stale from a global optimizer post-step hook (the
    buffer itself is kept: the next `_bit_plane` repacks into it, its address is a constant of the run)."""
    import torch
    from cnc_amd.gridencoder import GridEncoder
    enc = GridEncoder(num_dim=3, n_features=2, resolutions_list=(4, 8), log2_hashmap_size=8, ste_binary=True)
    enc._bits, enc._bits_key = object(), ("stale",)            # pretend a plane was packed
    opt = torch.optim.Adam(enc.parameters(), lr=1e-2, fused=True)
    v0 = enc.params._version
    enc.params.grad = torch.ones_like(enc.params)
    opt.step()
    if enc.params._version != v0:
        pytest.skip("this torch bumps _version in the fused optimizer")
    assert enc._bits_key is None and enc._bits is not None


def test_bench_refuses_a_world_that_contradicts_gpus():
    """`bench.py --gpus N` under a launcher that started a different number of ranks must stop, not report a line
    whose n_gpus is wrong; and without a GPU it must stop too (no CPU fallback in the measured path)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr
    import torch
    if not torch.cuda.is_available():
        env.pop("WORLD_SIZE")
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")], env=env, capture_output=True, text=True)
        assert r.returncode != 0 and "needs an MI355X" in r.stderr


def test_bench_options_for_the_full_run_and_the_output_dump():
    """`--full` (everything outside the timed region) and `--dump-outputs DIR` are offered; a dump without a timed step
    to take it from is refused before any work."""
    import os, subprocess, sys
    bench = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
    r = subprocess.run([sys.executable, bench, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
    r = subprocess.run([sys.executable, bench, "--steps", "0", "--dump-outputs", "unused"], capture_output=True, text=True)
    assert r.returncode != 0 and "at least one timed step" in r.stderr


def test_per_rank_sampling_streams_of_the_real_scene_loaders(tmp_path):
    """Data parallelism: `LoaderDataset.seed_sampling(seed + 1000 * rank)` gives every rank its own stream of images /
    pixels / backgrounds (without it all ranks would draw the same batch from the identically seeded global
    generators and the all-reduce would average N copies of one gradient), reproducibly, and leaves the global
    generators — which the replica-identical draws use — untouched."""
    import json
    from PIL import Image
    from cnc_amd.datasets import SubjectLoader
    from cnc_amd.trainer import LoaderDataset
    root = tmp_path / "nerf_synthetic" / "lego"
    (root / "train").mkdir(parents=True)
    rng = np.random.default_rng(0)
    frames = []
    for i in range(5):
        Image.fromarray(rng.integers(0, 256, size=(16, 16, 4), dtype=np.uint8), "RGBA").save(root / "train" / f"r_{i}.png")
        c2w = np.eye(4)
        c2w[:3, 3] = [0.1 * i, 0.0, 4.0]
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": c2w.tolist()})
    for split in ("train", "test"):
        json.dump({"camera_angle_x": 0.6911, "frames": frames}, open(root / f"transforms_{split}.json", "w"))

    def dataset(rank):
        tr = SubjectLoader("lego", str(tmp_path / "nerf_synthetic"), "train", num_rays=32, color_bkgd_aug="random")
        te = SubjectLoader("lego", str(tmp_path / "nerf_synthetic"), "test")
        ds = LoaderDataset(tr, te)
        if rank is not None:
            ds.seed_sampling(42 + 1000 * rank)
        return ds

    torch.manual_seed(7)
    state = torch.get_rng_state()
    a0, a1, b0 = dataset(0), dataset(1), dataset(0)
    fa0, fa1, fb0 = a0.fetch(), a1.fetch(), b0.fetch()
    assert torch.equal(torch.get_rng_state(), state)                       # the global generator was not consumed
    assert torch.equal(fa0["pixels"], fb0["pixels"]) and torch.equal(fa0["rays"].origins, fb0["rays"].origins)
    assert torch.equal(fa0["color_bkgd"], fb0["color_bkgd"])               # same rank, same stream
    assert not torch.equal(fa0["pixels"], fa1["pixels"])                   # another rank, another batch
    assert not torch.equal(fa0["color_bkgd"], fa1["color_bkgd"])
    # without a per-rank seed the loaders follow the global generators, as the single-GPU reference does
    torch.manual_seed(7)
    g0 = dataset(None).fetch()
    torch.manual_seed(7)
    g1 = dataset(None).fetch()
    assert torch.equal(g0["pixels"], g1["pixels"])


def test_field_row_buckets_and_vertex_set_host_logic():
    """Host-side pieces of the round-3 training step that need no GPU: (i) the row count the field's GEMMs run at —
    a multiple of 2^(floor(log2 n) - 5) at or above n, n itself below `row_bucket_min`, never more than ~3 % above n, and
    only a handful of distinct values over the range a run's sample counts take; (ii) the vertex set of the vote plan
    from shifted ORs equals the reference's candidates-then-unique construction (utils_bpp_acc.py:498-512)."""
    from cnc_amd.field import NGPRadianceField_mygrid_2D3D
    f = NGPRadianceField_mygrid_2D3D(aabb=[-1.5] * 3 + [1.5] * 3, n_features_per_level=2, n_neurons=32,
                                     resolutions_list=(6, 9), log2_hashmap_size=8, resolutions_list_2D=(10,),
                                     log2_hashmap_size_2D=8)
    f.row_bucket_min = 4096
    assert f._bucket_rows(100) == 100 and f._bucket_rows(4095) == 4095
    assert f._bucket_rows(4096) == 4096 and f._bucket_rows(4097) == 4096 + 128
    for n in (5000, 65537, 258446, 270000, 1500000):
        b = f._bucket_rows(n)
        g = 1 << (n.bit_length() - 6)
        assert b >= n and b % g == 0 and b - n < g and b <= n * 1.032
    assert len({f._bucket_rows(n) for n in range(240000, 280000, 37)}) <= 11
    # (ii)
    torch.manual_seed(0)
    for Rb, t in ((8, 4), (6, 1), (5, 3)):
        res = Rb * t + 2
        occ = torch.rand(Rb, Rb, Rb) < 0.15
        ar = torch.arange(-1, t + 1)
        base = torch.stack(torch.meshgrid(ar, ar, ar, indexing="ij"), -1).unsqueeze(0)
        cells = torch.stack(torch.meshgrid(*[torch.arange(Rb)] * 3, indexing="ij"), -1).view(-1, 1, 1, 1, 3)
        coords = (cells[occ.reshape(-1)] * t + base).view(-1, 3) + 1
        lin = torch.unique(coords[..., 0] * res * res + coords[..., 1] * res + coords[..., 2], dim=0)
        want = torch.stack([lin // (res * res), (lin // res) % res, lin % res], -1)
        m = occ
        for axis in range(3):
            up = m.repeat_interleave(t, dim=axis)
            n = up.shape[axis]
            shape = list(up.shape)
            shape[axis] = n + 2
            out = torch.zeros(shape, dtype=torch.bool)
            for sft in range(3):
                out.narrow(axis, sft, n).logical_or_(up)
            m = out
        assert torch.equal(torch.nonzero(m), want)


def test_gradient_sink_bookkeeping_on_cpu():
    """cnc_amd._gradsink without a GPU: buffers are handed out by tensor identity, only inside an `activate` scope of
    the calling thread; `flush` adds what was accumulated to `.grad` (or assigns it), skips what nobody touched, and
    the arena it hands out is not aliased by the gradient it leaves behind."""
    import threading

    from cnc_amd import _gradsink as gs
    torch.manual_seed(0)
    t1, t2 = torch.nn.Parameter(torch.randn(40, 8)), torch.nn.Parameter(torch.randn(16, 8))
    w, b = torch.nn.Parameter(torch.randn(4, 9)), torch.nn.Parameter(torch.randn(4))
    other = torch.nn.Parameter(torch.randn(40, 8))
    sink = gs.GradSink([t1, t2], [w, b])
    assert gs.current() is None
    with gs.activate(sink):
        assert gs.current() is sink
        seen = []
        th = threading.Thread(target=lambda: seen.append(gs.current()))     # another thread: no sink
        th.start(); th.join()
        assert seen == [None]
        with gs.activate(None):
            assert gs.current() is None
        assert gs.current() is sink
    assert gs.current() is None
    sink.zero()
    assert sink.table(other) is None and sink.table(t1.detach()[:10]) is None       # not one of its tables / wrong shape
    v1 = sink.table(t1)
    v1 += 2.0                                                 # what an encoder backward's atomics would do
    v1 += 1.0
    slots = sink.small_slot([w, b, None])
    assert slots[2] is None and slots[0].numel() == 36 and slots[1].numel() == 4
    assert sink.small_slot([w, other]) is None                # a parameter the sink does not hold: caller falls back
    for r in range(gs.REPLICAS):                              # workgroups spread their atomics over the replicas
        sink.replicas[r, :36] += float(r)
    t1.grad = torch.ones_like(t1)
    sink.flush()
    assert torch.equal(t1.grad, torch.full_like(t1, 4.0))     # 1 (autograd's) + 3 (the sink's)
    assert t2.grad is None                                    # untouched table: nothing assigned, nothing added
    assert torch.equal(w.grad, torch.full_like(w, float(sum(range(gs.REPLICAS))))) and torch.equal(b.grad, torch.zeros(4))
    t1.grad = None
    sink.flush()                                              # `.grad` was None: it gets a COPY of the arena's view
    kept = t1.grad.clone()
    sink.zero()
    assert torch.equal(t1.grad, kept) and float(kept.abs().max()) == 3.0
    sink.flush()                                              # nothing used since zero(): a no-op
    assert torch.equal(t1.grad, kept)
    bucket = {id(t1): torch.zeros_like(t1)}
    sink.table(t1).add_(5.0)
    sink.flush(grads_of=lambda p: bucket.get(id(p)))          # data-parallel form: add into the bucket's views
    assert torch.equal(bucket[id(t1)], torch.full_like(t1, 5.0)) and torch.equal(t1.grad, kept)


def test_fused_field_shape_table_on_cpu():
    """Which configurations `FusedFieldForward` takes (the kernel's shape table, include/cnc_hip.h) and which fall
    back to the chain — decided on the host, no GPU needed."""
    from cnc_amd.field import FusedFieldForward, NGPRadianceField_mygrid_2D3D
    base = dict(aabb=[-1.5] * 3 + [1.5] * 3, resolutions_list=(6, 9, 14), log2_hashmap_size=8,
                resolutions_list_2D=(10, 18), log2_hashmap_size_2D=8)
    ok = lambda **kw: FusedFieldForward.supported(NGPRadianceField_mygrid_2D3D(**base, **kw))
    assert ok(n_features_per_level=8, n_neurons=160) and ok(n_features_per_level=4, n_neurons=160)
    assert ok(n_features_per_level=2, n_neurons=64) and ok(n_features_per_level=4, n_neurons=64)
    assert not ok(n_features_per_level=8, n_neurons=64)        # geo 79: the head input does not fit 64 columns
    assert not ok(n_features_per_level=2, n_neurons=128)       # hidden width outside {64, 160}
    assert not ok(n_features_per_level=1, n_neurons=64)        # F outside {2, 4, 8}
    assert not ok(n_features_per_level=8, n_neurons=160, unbounded=True)
    assert not ok(n_features_per_level=8, n_neurons=160, fused_ste=False)
    f = NGPRadianceField_mygrid_2D3D(**base, n_features_per_level=8, n_neurons=160)
    assert f.sh_fp16_round and f.fused_field and f.fused_field_precision == "f16x3"
    x = torch.rand(5, 3)
    assert f._fused_forward(x) is None                          # host tensors, gradients on: the chain
    with torch.no_grad():
        assert f._fused_forward(x) is None                      # host tensors: still the chain (no CPU fallback of a kernel)


def test_procedural_dataset_fetch_reads_prerendered_views():
    """SyntheticBallDataset.fetch indexes training views rendered once (as the reference's loader indexes its images,
    nerf_synthetic.py:164-239): the pixels are exactly what shading the fetched rays gives, and the random draws
    (view, x, y, background) are consumed in the same order as before."""
    from cnc_amd.trainer import SyntheticBallDataset
    ds = SyntheticBallDataset(image_size=24, n_train_views=5, device="cpu", seed=3)
    ref = SyntheticBallDataset(image_size=24, n_train_views=5, device="cpu", seed=3)
    for n in (7, 300):
        got = ds.fetch(n)
        img = torch.randint(0, 5, (n,), generator=ref.gen)
        x = torch.randint(0, 24, (n,), generator=ref.gen).float()
        y = torch.randint(0, 24, (n,), generator=ref.gen).float()
        o, d = ref._rays(ref.train_c2w[img], x, y)
        rgb, alpha = ref._shade(o, d)
        bk = torch.rand(3, generator=ref.gen)
        assert torch.equal(got["rays"].origins, o) and torch.equal(got["rays"].viewdirs, d)
        assert torch.equal(got["color_bkgd"], bk)
        assert torch.equal(got["pixels"], rgb * alpha + bk * (1 - alpha))
    assert ds._images.shape == (5, 24, 24, 4) and 0.02 < float(ds._images[..., 3].mean()) < 0.5
