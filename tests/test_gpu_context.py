"""cnc_amd.context.CNC_context_models (HIP kernels) vs golden vectors produced by the REFERENCE's
own class on CPU (tests/golden/make_golden_context.py): same tables, entropy estimate and gradients
within fp32 tolerance, same set of coded rows, decode == the reference's decode bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "context_toy.npz")
TOY = dict(res3=[6, 9, 14, 20, 26, 34], res2=[10, 18, 34, 66], T3=10, T2=9, F=4, Rb=8, fine=34,
           sample_num=400, max_pts=20000)


@pytest.fixture(scope="module")
def setup(cuda):
    from cnc_amd.context import CNC_context_models
    from cnc_amd.gridencoder import GridEncoder
    g = np.load(GOLD)
    c = TOY
    torch.manual_seed(11)     # same CPU draws (randperm of dense levels, utils_rand) as the golden run
    m = CNC_context_models(num_dim=3, resolutions_list=c["res3"], resolutions_list_2D=c["res2"],
                           log2_hashmap_size=c["T3"], log2_hashmap_size_2D=c["T2"], n_features=c["F"],
                           sample_num=c["sample_num"], max_context_layer_num=3, ste_binary=True,
                           Pg_level=6, Pg_level_2D=4, Rb=c["Rb"], step_update=16, skip_levels_3D=[0, 1, 2],
                           skip_levels_2D=[0], device=cuda, dimension_wise_resolution=c["fine"])
    m.MAX_POINTS_NUM_TO_OOM = c["max_pts"]
    m.rand_like = lambda t: torch.rand(t.shape).to(t.device)     # replay the reference's CPU stream
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd_")}
    m.load_state_dict(sd, strict=True)
    encs = {}
    for name, D, res, T in (("xyz", 3, c["res3"], c["T3"]), ("xy", 2, c["res2"], c["T2"]),
                            ("xz", 2, c["res2"], c["T2"]), ("yz", 2, c["res2"], c["T2"])):
        e = GridEncoder(num_dim=D, n_features=c["F"], resolutions_list=res, log2_hashmap_size=T, ste_binary=True).to(cuda)
        with torch.no_grad():
            e.params.copy_(torch.from_numpy(g[f"params_{name}"]))
        encs[name] = e
    binary = torch.from_numpy(g["binary_vxl"]).to(cuda)
    return g, m, encs, binary


def test_tables_equal_reference(setup):
    g, m, encs, binary = setup
    assert np.array_equal(m.utils_rand.cpu().numpy(), g["utils_rand"])
    assert np.array_equal(m.unique_count_list.cpu().numpy(), g["unique_count_list"])
    assert np.array_equal(m.sample_num_levels.cpu().numpy(), g["sample_num_levels"])
    for n in range(6):
        assert np.array_equal(m.unique_value_list[n].cpu().numpy(), g[f"uv_{n}"]), n
        # the order of the vertices INSIDE one hash slot is whatever torch.sort leaves (unstable
        # sort in the reference): compare slot by slot as sets
        cnt = g["unique_count_list"][n][: len(g[f"uv_{n}"])]
        slot = np.repeat(np.arange(len(cnt)), cnt)
        def canon(pos):
            key = (pos[:, 0].astype(np.int64) * 4096 + pos[:, 1]) * 4096 + pos[:, 2]
            return pos[np.lexsort((key, slot))]
        assert np.array_equal(canon(m.pos_grid_sorted_list[n].cpu().numpy()), canon(g[f"pos_{n}"])), n


def test_training_pass_matches_reference(setup):
    g, m, encs, binary = setup
    for step, seed in ((0, 77), (1, 78)):
        torch.manual_seed(seed)
        for e in encs.values():
            e.zero_grad()
        m.zero_grad()
        bpp, mb = m.forward_binary_vxl_mixPg_3D2D(encs["xyz"], encs["xy"], encs["xz"], encs["yz"], binary, step=step)
        bpp.backward()
        want = float(g[f"fwd{step}_bpp"])
        assert abs(bpp.item() - want) <= 1e-4 * abs(want), (step, bpp.item(), want)
        assert abs(mb - float(g[f"fwd{step}_mb"])) <= 1e-4 * float(g[f"fwd{step}_mb"])
        for name, e in encs.items():
            ref = g[f"fwd{step}_grad_{name}"]
            got = e.params.grad.cpu().numpy()
            scale = np.abs(ref).max()
            assert np.abs(got - ref).max() <= 2e-4 * scale, (step, name, np.abs(got - ref).max(), scale)
            assert np.array_equal(got == 0, ref == 0) or (np.abs(got[(got == 0) != (ref == 0)]).max() < 1e-9 * scale)
        for key, w in (("ctx3d_w0", m.context_model_3D[0].weight), ("ctx2d_w0", m.context_model_2D[0][0].weight)):
            ref = g[f"fwd{step}_grad_{key}"]
            assert np.abs(w.grad.cpu().numpy() - ref).max() <= 2e-4 * np.abs(ref).max()


def test_encode_decode_matches_reference(setup, tmp_path):
    g, m, encs, binary = setup
    prefix = str(tmp_path / "b")
    with torch.no_grad():
        Pgs, est_mb, coded_mb = m.encode_binary_vxl_mixPg_3D2D(encs["xyz"], encs["xy"], encs["xz"], encs["yz"],
                                                               binary, filename_prefix=prefix)
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith(".b"))
    assert files == list(g["enc_files"])                                  # same levels / chunking
    sizes = np.array([os.path.getsize(tmp_path / f) for f in files], np.int64)
    ref_sizes = g["enc_sizes"]
    assert abs(int(sizes.sum()) - int(ref_sizes.sum())) <= 0.005 * ref_sizes.sum()   # north-star: +-0.5 %
    assert np.abs(sizes - ref_sizes).max() <= 2                              # per file: rounding of p only
    assert abs(est_mb - float(g["enc_est_mb"])) <= 1e-4 * float(g["enc_est_mb"])
    assert list(Pgs.keys()) == list(g["pg_keys"])
    assert np.allclose([float(v) for v in Pgs.values()], g["pg_vals"], rtol=0, atol=1e-7)
    recs = [torch.ones_like(encs[n].params.data) for n in ("xyz", "xy", "xz", "yz")]
    out = m.decode_binary_vxl_mixPg_3D2D(encs["xyz"], encs["xy"], encs["xz"], encs["yz"], *recs, binary, Pgs,
                                         filename_prefix=prefix)
    for name, t in zip(("xyz", "xy", "xz", "yz"), out):
        got = t.cpu().numpy().astype(np.int8)
        assert np.array_equal(got, g[f"dec_{name}"]), name               # incl. which rows were never coded
        q = np.where(g[f"params_{name}"] >= 0, 1, -1)
        coded = ~(got == 1).all(axis=1) | (q == 1).all(axis=1)
        assert np.array_equal(got[coded], q[coded])


def test_fused_ste_equals_unfused(setup):
    """GridEncoder(fused_ste=True) (sign inside the gather, mask inside the scatter) == the
    reference's op-by-op STE_binary dataflow."""
    from cnc_amd.gridencoder import GridEncoder
    g, m, encs, binary = setup
    c = TOY
    a = GridEncoder(3, c["F"], c["res3"], c["T3"], ste_binary=True, fused_ste=True).to(binary.device)
    b = GridEncoder(3, c["F"], c["res3"], c["T3"], ste_binary=True, fused_ste=False).to(binary.device)
    with torch.no_grad():
        a.params.copy_(torch.from_numpy(g["params_xyz"]))
        b.params.copy_(a.params)
    x = torch.rand(5000, 3, device=binary.device)
    w = torch.randn(5000, c["F"] * 6, device=binary.device)
    ya, yb = a(x), b(x)
    assert torch.equal(ya, yb)
    (ya * w).sum().backward()
    (yb * w).sum().backward()
    # two atomic scatters of the same terms in different orders
    assert (a.params.grad - b.params.grad).abs().max() <= 1e-5 * b.params.grad.abs().max()
    # same untouched entries; a touched entry may cancel to exactly 0 in one summation order only
    differ = (a.params.grad == 0) != (b.params.grad == 0)
    assert (a.params.grad[differ].abs().max() if differ.any() else 0) <= 1e-9 * b.params.grad.abs().max()
    assert (b.params.grad[differ].abs().max() if differ.any() else 0) <= 1e-9 * b.params.grad.abs().max()


def test_fused_segment_reduction_equals_packed_dataflow(setup):
    """fused_segments=True (one segmented-reduction kernel) vs the reference's pack -> multiply -> sum."""
    g, m, encs, binary = setup
    res = {}
    for fused in (True, False):
        m.fused_segments = fused
        torch.manual_seed(5)
        for e in encs.values():
            e.zero_grad()
        m.zero_grad()
        bpp, _ = m.forward_binary_vxl_mixPg_3D2D(encs["xyz"], encs["xy"], encs["xz"], encs["yz"], binary, step=0)
        bpp.backward()
        res[fused] = (bpp.item(), encs["xyz"].params.grad.clone(), m.context_model_3D[0].weight.grad.clone())
    m.fused_segments = True
    assert abs(res[True][0] - res[False][0]) <= 1e-5 * abs(res[False][0])
    for a, b in zip(res[True][1:], res[False][1:]):
        assert (a - b).abs().max() <= 1e-4 * b.abs().max()


def test_vertex_set_fast_path_equals_the_candidate_lattice_branch(setup):
    """get_idx_coords2: the shifted-OR construction (fused_segments, GPU) and the reference's candidates-then-unique
    expression (utils_bpp_acc.py:498-512) return the same sorted vertex set in the same dtype; a resolution the
    candidate lattice was not built for is refused by both."""
    g, m, encs, binary = setup
    out = {}
    for fused in (True, False):
        m.fused_segments = fused
        out[fused] = m.get_idx_coords2(binary)
    m.fused_segments = True
    assert out[True].dtype == out[False].dtype == torch.int32
    assert out[True].shape[0] > 0 and torch.equal(out[True], out[False])
    other = m.dimension_wise_resolution + m.binary_vxl_len          # factor t + 1
    for fused in (True, False):
        m.fused_segments = fused
        with pytest.raises(ValueError, match="does not match the lattice"):
            m.get_idx_coords2(binary, resolution=other)
    m.fused_segments = True


def test_plane_ring_vertices_kernel_equals_the_tensor_expression(setup, cuda):
    """`fetch_2D_batches` (utils_bpp_acc.py:431-456) as one kernel against the reference's tensor expression: same
    table rows, same positions bit for bit, every 2-D level of the toy model (dense and hashed) on its three planes;
    then the slot lists built from them; then the row formula alone at the full-size levels (R up to 1026, T = 2^17)."""
    from cnc_amd.backends import context_backend as ck
    from cnc_amd.context import get_grid_index
    g, m, encs, binary = setup
    for axis in ("xy", "xz", "yz"):
        plane = m._project(binary, axis)
        for n in range(m.n_levels_2D):
            got = {}
            for fused in (True, False):
                m.fused_segments = fused
                got[fused] = (m.fetch_2D_batches(plane, n), m._sorted_slots_2D(plane, n))
            m.fused_segments = True
            (ri, pi), si = got[True]
            (rt, pt), st = got[False]
            assert ri.dtype == torch.int32 and ri.shape[0] > 0
            assert torch.equal(ri.long(), rt) and torch.equal(pi, pt), (axis, n)
            for a, b in zip(si, st):
                assert a.dtype == b.dtype and torch.equal(a, b), (axis, n)
    gen = torch.Generator(device=cuda).manual_seed(4)
    for R, T, hs in ((130, 1, 130 * 130), (258, 2, 258 * 258), (514, 4, 2 ** 17), (1026, 8, 2 ** 17), (1026, 8, 100003)):
        cells = torch.randint(0, 128, (3000, 2), device=cuda, generator=gen)
        rows, pts = ck.plane_ring_vertices(cells, T, R, hs)
        ar = torch.arange(T + 2, device=cuda)
        ring = torch.stack(torch.meshgrid(ar, ar, indexing="ij"), dim=-1).view(1, T + 2, T + 2, 2)
        v = (cells.view(-1, 1, 1, 2) * T + ring).view(-1, 2)
        assert torch.equal(rows.long(), get_grid_index(hs, R, v)), (R, hs)
        assert torch.equal(pts, (v - 0.5) / float(R - 2)), (R, hs)
        assert int(rows.max()) < hs and int(rows.min()) >= 0
    rows, pts = ck.plane_ring_vertices(torch.zeros((0, 2), dtype=torch.long, device=cuda), 4, 514, 2 ** 17)
    assert rows.shape == (0,) and pts.shape == (0, 2)


def test_plane_batched_levels_equal_the_level_by_level_pass(setup):
    """The coded levels of a plane evaluated together (one encoder call over levels [0, max n), the heads on row ranges
    of one matrix through `ContextHeads`, one per-slot mean) against one pass per level: the same rate to fp32 summation
    order, the same gradients into the plane tables, the finest 3-D level (votes), every 2-D head and the level
    frequencies behind Pg."""
    g, m, encs, binary = setup
    assert m._plane_batch_ok(encs["xy"].params)
    res = {}
    for batched in (True, False):
        m.plane_batched = batched
        torch.manual_seed(5)
        for e in encs.values():
            e.zero_grad()
        m.zero_grad()
        bpp, _ = m.forward_binary_vxl_mixPg_3D2D(encs["xyz"], encs["xy"], encs["xz"], encs["yz"], binary, step=0)
        bpp.backward()
        res[batched] = [bpp.detach().clone()] + [encs[k].params.grad.clone() for k in ("xyz", "xy", "xz", "yz")] + \
                       [p.grad.clone() for p in m.context_model_2D.parameters()]
    m.plane_batched = True
    # the plane records from ONE composite-key sort (refresh path) against per-level sorts concatenated
    binary_2D = [m._project(binary, a) for a in ("xy", "xz", "yz")]
    assert m._refresh_plane_cats(binary_2D)
    one_sort = [dict(c) for c in m._plane_cat]
    m.batched_inputs_list, m._plane_cat = m._slot_lists_2D(binary_2D), [None, None, None]
    Pg_all, bits_all = m.level_stats(m.get_STE_params(encs["xy"]), m._off2_host)
    for k, name in enumerate(("xy", "xz", "yz")):
        with torch.no_grad():
            m._plane_bits(k, encs[name], m.get_STE_params(encs[name]), Pg_all, bits_all, binary_2D[k], None if not m.use_dimension_wise
                          else torch.zeros(m.dimension_wise_resolution ** 2, m.n_features, device=binary.device), False)
        for key in ("pts", "order", "rows", "cum"):
            assert one_sort[k][key].dtype == m._plane_cat[k][key].dtype, (k, key)
            assert torch.equal(one_sort[k][key], m._plane_cat[k][key]), (k, key)
        assert one_sort[k]["segs"] == m._plane_cat[k]["segs"]
    assert abs(float(res[True][0]) - float(res[False][0])) <= 2e-6 * abs(float(res[False][0]))
    for a, b in zip(res[True][1:], res[False][1:]):
        assert float(b.abs().max()) > 0
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max())


@pytest.mark.parametrize("Rb,t,log2T", [(8, 4, 10), (8, 1, 12), (16, 2, 19), (128, 4, 19)])
def test_vote_plan_from_the_occupancy_grid_equals_the_plan_from_the_vertex_list(cuda, Rb, t, log2T):
    """`VotePlan.from_occupancy` (vertex volume -> per-pixel counts -> rows written in pixel-major order, one sort by
    table row of packed vertices) against `VotePlan(get_idx_coords2 list)` (three stable sorts by pixel, one by row):
    the same rows per pixel in the same order, the same segments, the same vertices per table row in the same order —
    toy sizes, a dense finest level (R^3 < T), occupancy touching the border (skipped vertices), and the full size."""
    from cnc_amd.backends import gridencoder_backend as be
    g = torch.Generator(device=cuda).manual_seed(Rb * 10 + t)
    if Rb == 128:
        from cnc_amd.synthetic import ball_binaries
        occ = ball_binaries(128, device=cuda)[0].bool()
    else:
        occ = torch.rand(Rb, Rb, Rb, device=cuda, generator=g) < 0.15
        occ[0, 0, :] = True                                  # cells on the box: vertices cnt_np_embed skips
        occ[-1, :, -1] = True
    R, hs = Rb * t + 2, 2 ** log2T
    m = occ
    for axis in range(3):                                    # get_idx_coords2's construction (context.py)
        up = m.repeat_interleave(t, dim=axis)
        n = up.shape[axis]
        shape = list(up.shape)
        shape[axis] = n + 2
        out = torch.zeros(shape, dtype=torch.bool, device=cuda)
        for sft in range(3):
            out.narrow(axis, sft, n).logical_or_(up)
        m = out
    verts = torch.nonzero(m).to(torch.int16).contiguous()
    a = be.VotePlan(verts, R, hs)
    b = be.VotePlan.from_occupancy(occ, t, R, hs)
    n = int(b.pixel_seg[0][-1])
    assert n > 0 and n == int(a.pixel_seg[0][-1])
    for k in range(3):
        assert torch.equal(a.pixel_seg[k], b.pixel_seg[k]), k
        assert torch.equal(a.rows_by_pixel[k][:n], b.rows_by_pixel[k]), k
        assert torch.equal(a.pixels_by_row[k][:n], b.pixels_by_row[k]), k
    assert torch.equal(a.row_seg, b.row_seg)
    # and the kernels that consume the two forms: counts and the three-plane backward
    F = 8
    emb = torch.where(torch.rand(min(hs, R ** 3), F, device=cuda, generator=g) < 0.5, 1.0, -1.0)
    for axis in range(3):
        oa = torch.empty(R - 2, R - 2, F, 2, device=cuda)
        ob = torch.empty_like(oa)
        be.cnt_np_embed_planned(a, emb, oa, F, axis)
        be.cnt_np_embed_planned(b, emb, ob, F, axis)
        assert torch.equal(oa, ob)
    gs = [torch.randn(R - 2, R - 2, F, 2, device=cuda, generator=g) for _ in range(3)]
    ga, gb = torch.empty_like(emb), torch.empty_like(emb)
    be.cnt_np_embed_planned_backward3(a, emb, gs, ga, F)
    be.cnt_np_embed_planned_backward3(b, emb, gs, gb, F)
    assert torch.equal(ga, gb) and float(ga.abs().max()) > 0


def test_planned_votes_equal_atomic_votes(setup):
    """planned_votes=True (vertex list sorted once per refresh, segmented gathers) vs the atomic
    cnt_np_embed kernels: same entropy estimate, same gradients into the finest 3-D level and planes."""
    g, m, encs, binary = setup
    res = {}
    for planned in (True, False):
        m.planned_votes = planned
        torch.manual_seed(5)
        for e in encs.values():
            e.zero_grad()
        m.zero_grad()
        bpp, _ = m.forward_binary_vxl_mixPg_3D2D(encs["xyz"], encs["xy"], encs["xz"], encs["yz"], binary, step=0)
        bpp.backward()
        assert (m.vote_plan is not None) == planned
        res[planned] = (bpp.item(), encs["xyz"].params.grad.clone(), encs["xy"].params.grad.clone(),
                        next(m.context_model_2D[1].parameters()).grad.clone())
    m.planned_votes = True
    assert res[True][0] == res[False][0]        # the votes are integer counts: the forward is identical
    for a, b in zip(res[True][1:], res[False][1:]):
        assert (a - b).abs().max() <= 1e-5 * b.abs().max()


def test_vote_tables_node_equals_the_op_chain(setup):
    """`_vote_tables3` (counts -> fraction -> channel 0 -> ring of zeros as one kernel per plane, and one back) against
    `_cnt_np_embed_planned3` followed by the reference's op chain (`_ring_of_zeros`, utils_bpp_acc.py:515-526): same
    float operations, so the three tables and the gradient of the finest 3-D level are bit-equal."""
    from cnc_amd.context import _cnt_np_embed_planned3, _vote_tables3
    g, m, encs, binary = setup
    m.planned_votes = True
    m.forward_binary_vxl_mixPg_3D2D(encs["xyz"], encs["xy"], encs["xz"], encs["yz"], binary, step=0)   # builds the plan
    plan = m.vote_plan
    assert plan is not None
    fine = encs["xyz"].params.detach()[m._off3_host[-2]:m._off3_host[-1]]
    fine = torch.where(fine >= 0, torch.ones_like(fine), -torch.ones_like(fine))
    ws = [torch.randn(plan.resolution ** 2, fine.shape[1], device=fine.device) for _ in range(3)]
    out = {}
    for name in ("node", "chain"):
        x = fine.clone().requires_grad_(True)
        if name == "node":
            tabs = _vote_tables3.apply(plan, x)
        else:
            tabs = [m._ring_of_zeros(f) for f in _cnt_np_embed_planned3.apply(plan, x)]
        sum((t * w).sum() for t, w in zip(tabs, ws)).backward()
        out[name] = ([t.detach() for t in tabs], x.grad)
    for a, b in zip(out["node"][0], out["chain"][0]):
        assert a.shape == b.shape and torch.equal(a, b)
        assert float(a.max()) > 0 and float(a.min()) == 0.0
    assert torch.equal(out["node"][1], out["chain"][1]) and float(out["node"][1].abs().max()) > 0


SEGMENT_ATOL = {0: 1e-4, 1: 1e-5, 2: 1e-5}          # cnc_segment_weighted_sum per mode, against float64 sums


def test_segment_weighted_sum_kernel(cuda):
    from cnc_amd.backends import pack_and_align as pa
    rng = np.random.default_rng(0)
    cnt = rng.integers(0, 30, size=500).astype(np.int64)
    cnt[3] = 288
    T = int(cnt.sum())
    cum = torch.as_tensor(np.concatenate([[0], np.cumsum(cnt)]), device=cuda)
    for F in (1, 8):
        v = torch.randn(T, F, device=cuda)
        w = torch.rand(T, device=cuda) + 0.1
        ref = torch.zeros(500, F, device=cuda, dtype=torch.float64)
        slot = torch.repeat_interleave(torch.arange(500, device=cuda), torch.as_tensor(cnt, device=cuda))
        ref.index_add_(0, slot, (v * w[:, None]).double())
        wsum = torch.zeros(500, device=cuda, dtype=torch.float64).index_add_(0, slot, w.double())
        got0 = pa.segment_weighted_sum(v, w, cum, 0)
        assert torch.allclose(got0.double(), ref, atol=SEGMENT_ATOL[0])
        got1 = pa.segment_weighted_sum(v, w, cum, 1)
        nz = torch.as_tensor(cnt, device=cuda) > 0
        assert torch.allclose(got1[nz].double(), (ref / wsum[:, None])[nz], atol=SEGMENT_ATOL[1])
        got2 = pa.segment_weighted_sum(v, None, cum, 2)
        plain = torch.zeros(500, F, device=cuda, dtype=torch.float64).index_add_(0, slot, v.double())
        assert torch.allclose(got2[nz].double(), (plain / torch.as_tensor(cnt, device=cuda)[:, None])[nz], atol=SEGMENT_ATOL[2])


@pytest.mark.parametrize("F,sample_num", [(2, 200000), (8, 150000)])
def test_full_size_encode_decode_roundtrip(cuda, tmp_path, F, sample_num):
    """BASELINE configs[2] sizes (12x3-D T=2^19 + 3x4 planes T=2^17; F=8 / sample_num=150000 is the
    configuration BASELINE.json names, F=2 / 200000 the reference script's default): encode -> wipe ->
    decode reproduces every coded row; the 3-D chunking is the reference's (21 files); coded size
    within 2 % of the entropy estimate + per-file termination overhead."""
    from cnc_amd import synthetic
    from cnc_amd.context import CNC_context_models
    from cnc_amd.gridencoder import GridEncoder
    torch.manual_seed(3)
    m = CNC_context_models(num_dim=3, resolutions_list=synthetic.RES_3D_REF, resolutions_list_2D=synthetic.RES_2D_REF,
                           log2_hashmap_size=19, log2_hashmap_size_2D=17, n_features=F, sample_num=sample_num,
                           ste_binary=True, Pg_level=12, Pg_level_2D=4, Rb=128, skip_levels_3D=[0, 1, 2],
                           skip_levels_2D=[0], device=cuda)
    encs = [GridEncoder(3, F, synthetic.RES_3D_REF, 19, ste_binary=True).to(cuda)] + \
           [GridEncoder(2, F, synthetic.RES_2D_REF, 17, ste_binary=True).to(cuda) for _ in range(3)]
    with torch.no_grad():
        for e in encs:       # spatially smooth signs so the context models have something to predict
            e.params.copy_(torch.sin(torch.arange(e.params.shape[0], device=cuda).float()[:, None] * 0.01
                                     + torch.arange(F, device=cuda).float()) + 0.3 * torch.randn_like(e.params))
    binaries = synthetic.ball_binaries(128, radius=0.9, device=cuda)
    prefix = str(tmp_path / "b")
    with torch.no_grad():
        Pgs, est_MB, coded_MB = m.encode_binary_vxl_mixPg_3D2D(*encs, binaries, filename_prefix=prefix)
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith(".b"))
    assert len([f for f in files if "_3D" in f]) == 21 and len(files) == 33
    assert coded_MB <= est_MB * 1.02 + 33 * 8 / 1024 / 1024
    recs = [torch.ones_like(e.params.data) for e in encs]
    out = m.decode_binary_vxl_mixPg_3D2D(*encs, *recs, binaries, Pgs, filename_prefix=prefix)
    for e, dec in zip(encs, out):
        q = torch.where(e.params.data >= 0, 1.0, -1.0)
        coded = ~(dec == 1).all(dim=1)
        assert torch.equal(dec[coded], q[coded])
        assert coded.float().mean() > 0.2


def test_configs2_training_pass_forward_backward(cuda):
    """configs[2] (F=8, sample_num=150000, 12x3-D T=2^19 + 3x4 planes T=2^17): one training pass of
    `forward_binary_vxl_mixPg_3D2D` + backward.  Size-independent properties: the estimate is a finite,
    positive bit rate,
    the same seed gives the same value (the window draw is the only randomness), gradients reach the four
    tables and the context MLPs, are finite, and vanish on rows of levels that are never coded (3-D
    levels 0-2 and plane level 0 are skipped)."""
    from cnc_amd import synthetic
    from cnc_amd.context import CNC_context_models
    from cnc_amd.gridencoder import GridEncoder
    F = 8
    torch.manual_seed(5)
    m = CNC_context_models(num_dim=3, resolutions_list=synthetic.RES_3D_REF, resolutions_list_2D=synthetic.RES_2D_REF,
                           log2_hashmap_size=19, log2_hashmap_size_2D=17, n_features=F, sample_num=150000,
                           max_context_layer_num=3, ste_binary=True, Pg_level=12, Pg_level_2D=4, Rb=128,
                           step_update=16, skip_levels_3D=[0, 1, 2], skip_levels_2D=[0], device=cuda)
    encs = [GridEncoder(3, F, synthetic.RES_3D_REF, 19, ste_binary=True).to(cuda)] + \
           [GridEncoder(2, F, synthetic.RES_2D_REF, 17, ste_binary=True).to(cuda) for _ in range(3)]
    binaries = synthetic.ball_binaries(128, radius=1.0, device=cuda)
    vals = []
    for rep in range(2):
        torch.manual_seed(77)
        for p in [q for e in encs for q in e.parameters()] + list(m.parameters()):
            p.grad = None
        bpp, mb = m.forward_binary_vxl_mixPg_3D2D(*encs, binaries, step=0)
        bpp.backward()
        vals.append(float(bpp.detach()))
    assert vals[0] == vals[1]
    # an untrained context MLP can be confidently wrong: several bits per binary parameter is legitimate
    assert 0.3 < vals[0] < 32 and 0 < mb < 200 and np.isfinite(mb)
    g3 = encs[0].params.grad
    assert torch.isfinite(g3).all() and float(g3.abs().max()) > 0
    off = encs[0].offsets_list
    assert float(g3[int(off[3]):].abs().max()) > 0
    for e in encs[1:]:
        assert torch.isfinite(e.params.grad).all() and float(e.params.grad.abs().max()) > 0
    ctx_grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert ctx_grads and all(torch.isfinite(g).all() for g in ctx_grads)
    assert any(float(g.abs().max()) > 0 for g in ctx_grads)


def test_a_refresh_with_an_unchanged_occupancy_keeps_the_plan(setup):
    """Everything a refresh rebuilds is a function of the occupancy grid: when the estimator hands over a NEW tensor with the
    SAME cells at a refresh step, the structures are kept (and the pass returns what a full rebuild returns); a flipped
    cell rebuilds them."""
    g, m, encs, binary = setup

    def run(step, occ, skip):
        m.skip_unchanged_refresh = skip
        torch.manual_seed(5)
        bpp, _ = m.forward_binary_vxl_mixPg_3D2D(encs["xyz"], encs["xy"], encs["xz"], encs["yz"], occ, step=step)
        return float(bpp)

    base = run(0, binary, True)                                   # builds
    before = dict(m.refresh_stats)
    same = run(16, binary.clone(), True)                          # a fresh tensor, equal cells: kept
    assert m.refresh_stats["skipped"] == before["skipped"] + 1 and m.refresh_stats["refreshes"] == before["refreshes"] + 1
    plan = m.vote_plan
    rebuilt = run(32, binary.clone(), False)                      # forced rebuild
    assert m.vote_plan is not plan
    assert same == rebuilt == base
    flipped = binary.clone()
    idx = torch.nonzero(flipped.reshape(-1) == 0)[:3, 0]
    flipped.view(-1)[idx] = 1
    plan = m.vote_plan
    run(48, flipped, True)
    assert m.vote_plan is not plan and m.refresh_stats["skipped"] == before["skipped"] + 1
    # a cell that appears BEHIND others in all three projections: the 3-D structures are rebuilt, the planes' are kept —
    # and the pass returns what a full rebuild returns
    occ3 = binary.reshape(binary.shape[-3:]).bool()
    hidden = (~occ3) & occ3.any(2)[:, :, None] & occ3.any(1)[:, None, :] & occ3.any(0)[None, :, :]
    assert bool(hidden.any())
    deeper = binary.clone()
    deeper.view(-1)[torch.nonzero(hidden.reshape(-1))[:2, 0]] = 1
    run(64, binary.clone(), False)                                # planes built from `binary`'s projections
    held = lambda: [c["rows"] for c in m._plane_cat] if m._plane_cat[0] is not None else [m.batched_inputs_list]
    cats, plan, kept = held(), m.vote_plan, m.refresh_stats.get("planes_kept", 0)
    got = run(80, deeper, True)
    assert m.vote_plan is not plan and m.refresh_stats.get("planes_kept", 0) == kept + 1
    assert all(a is b for a, b in zip(cats, held()))
    want = run(96, deeper.clone(), False)
    assert got == want
    m.skip_unchanged_refresh = True
    run(0, binary, True)                                          # leave the module fixture as the other tests expect it
