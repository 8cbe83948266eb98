"""The field's glue kernels and the two streaming kernels (cnc_amd/csrc/field_glue.hip) through the C ABI, against
tests/glue_twin.py: cnc_field_prepare, cnc_field_sinusoid, cnc_field_post, cnc_field_post_backward,
cnc_relu_backward_bias, cnc_ste_binary_forward / _backward.

Everything the kernels compute with +, -, *, /, comparisons and the half round trip is compared BIT FOR BIT with the
float32 twin (the kernel's header promises the op chain's operations in the op chain's order; the library is built
with contraction off).  Outputs lie in sentinel-filled, over-long buffers (tests/guarded.py): columns and rows a call
does not own must keep the sentinel.

Two library functions remain, `expf` and `sincosf`.  Their bounds can be neither derived nor taken from the project:
each was measured ONCE on an MI355X as the largest error, in ulp of the float32 result, against the float64 function
of the same float32 argument over this module's inputs, and the assertion is twice that figure (inputs not drawn):
    expf      (density, normal results)       measured 0.834 ulp (EXPF_ULP)     -> asserted 1.668
    expf      (density, subnormal results)    measured 0.234 ulp (EXPF_SUB_ULP) -> asserted 0.468
    sincosf   (sin and cos, |x f| <= 615)     measured 1.535 ulp (SINCOS_ULP)   -> asserted 3.07
All are below the 4 ulp above which a different function would have to be suspected.  The module prints what it
measures (pytest -s).  Whether sincosf returns sinf's and cosf's values is compared with torch.sin / torch.cos of
the same tensor on the device and printed, not asserted: on the MI355X all 2,100,030 sines and all cosines were equal
(profiles/adam_glue_matrix.md).

The bias gradient's column sums are held to c 2^-24 sum|g| of the float64 sums, c from the summation depth: a lane
adds its ceil(rows_per_block / R) rows one by one, then one lane per column adds the R lane sums; each addition
rounds by at most 2^-24 of a partial sum, itself at most the block's sum|g|, and the blocks' bounds add up to the
column's.  The test adds the partials in float64, so they contribute nothing: c = ceil(rows_per_block / R) + R + 1
(the 1 for the second-order terms), at most 260 (C = 4: R = 256) — a worst-case bound, no statistics."""
import numpy as np
import pytest
import torch

import glue_twin as G
from guarded import Guarded, sentinel

pytestmark = pytest.mark.gpu

f32, f64, u32 = np.float32, np.float64, np.uint32
INVALID = -1
EXPF_ULP = 0.834              # measured on an MI355X over this module's inputs (see the docstring); asserted twice
EXPF_SUB_ULP = 0.234
SINCOS_ULP = 1.535
N_ROWS = [1, 255, 256, 257, 70001]
AABB = np.array([-1.5, -1.0, -0.5, 1.5, 2.0, 0.75], f32)
SH_FP16 = 1

_MEASURED = {}


def _note(group, r):
    _MEASURED[group] = max(_MEASURED.get(group, 0.0), float(r))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nfield glue, measured: " + ", ".join(f"{k} {v:.4g}" for k, v in sorted(_MEASURED.items())))


def _lib():
    from cnc_amd import _lib as L
    return L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits_equal(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == f32 and got.shape == want.shape
    return (got.view(u32) == want.view(u32)) | (np.isnan(got) & np.isnan(want))


def _assert_bits(got, want, what):
    ok = _bits_equal(got, want)
    if not ok.all():
        i = np.unravel_index(int(np.argmin(ok)), ok.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} differ, first at {i}: got {got[i]!r} want {want[i]!r}")


def _ulp_error(got, ref64):
    """|got - ref| in units of the float32 spacing at ref (finite ref only)."""
    with np.errstate(all="ignore"):
        ref32 = ref64.astype(f32)
        return np.abs(got.astype(f64) - ref64) / np.spacing(np.abs(ref32)).astype(f64)


def _untouched(buf):
    return bool((buf.get().reshape(-1).view(np.uint8) == 0xA5).all())


# ------------------------------------------------------------------------------------------------------------------
# cnc_field_prepare
# ------------------------------------------------------------------------------------------------------------------
def _positions(N, seed):
    rng = np.random.default_rng(seed)
    lo, hi = AABB[:3], AABB[3:]
    pos = (lo + (hi - lo) * rng.uniform(-0.15, 1.15, size=(N, 3))).astype(f32)
    inside = (lo + (hi - lo) * f32(0.5)).astype(f32)
    rows = []
    for a in range(3):
        for v in (lo[a], hi[a], np.nextafter(lo[a], hi[a]), np.nextafter(hi[a], lo[a]), np.nextafter(lo[a], f32(-9)),
                  np.nextafter(hi[a], f32(9)), f32(np.nan)):
            r = inside.copy()
            r[a] = v
            rows.append(r)
    rows = np.asarray(rows, f32)
    k = min(N, len(rows))
    at = rng.permutation(N)[:k]
    pos[at] = rows[(np.arange(k) + N) % len(rows)]          # N = 1 gets one of them, the larger N all 21
    return pos


@pytest.mark.parametrize("N", N_ROWS)
def test_prepare(cuda, N):
    """An asymmetric box; rows with one coordinate exactly on a face (selector 0), one float32 step inside it, one step
    outside, NaN (selector 0).  x_unit and the selector equal the twin's bit for bit (float32 division is correctly
    rounded); rows at and behind N keep the sentinel."""
    pos = _positions(N, N)
    want_x, want_s = G.prepare(pos, AABB)
    P, A = Guarded(pos, cuda), Guarded(AABB, cuda)
    X, S = Guarded.empty((N, 3), f32, cuda), Guarded.empty((N,), np.uint8, cuda)
    assert _lib().cnc_field_prepare(P.ptr, A.ptr, N, X.ptr, S.ptr, _stream()) == 0
    torch.cuda.synchronize()
    _assert_bits(X.get(), want_x, "x_unit")
    assert np.array_equal(S.get(), want_s)
    assert all(b.intact() for b in (P, A, X, S)) and np.array_equal(P.get().view(u32), pos.view(u32))
    if N >= 255:
        lo, hi = AABB[:3], AABB[3:]
        on_face = ((pos == lo) | (pos == hi) | np.isnan(pos)).any(1)
        assert on_face.sum() >= 9 and not want_s[on_face].any()
        just_in = (pos == np.nextafter(lo, hi)).any(1)
        assert just_in.sum() == 3 and want_s[just_in].all()
        assert 0.3 < want_s.mean() < 0.7


# ------------------------------------------------------------------------------------------------------------------
# cnc_field_sinusoid
# ------------------------------------------------------------------------------------------------------------------
def _unit_points(N, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.2, 1.2, size=(N, 3)).astype(f32)
    sp = np.array([0.0, -0.0, 1.0], f32)
    k = min(N, 3)
    x[rng.permutation(N)[:k], rng.integers(0, 3, k)] = sp[(np.arange(k) + N) % 3]
    return x


@pytest.mark.parametrize("n_freqs", [0, 1, 10])
@pytest.mark.parametrize("N", N_ROWS)
def test_sinusoid(cuda, N, n_freqs):
    """[x | sin(2^k x) | cos(2^k x) | zeros] into columns col .. ld of a wider matrix: without padding, with padding, and
    behind col > 0 columns that must keep the sentinel.  The copy of x and the padding zeros are exact; sin and cos are
    held to float64 sin / cos of the float32 product x * f."""
    x = _unit_points(N, 31 * N + n_freqs)
    freqs = (2.0 ** np.arange(max(n_freqs, 1))).astype(f32)
    w = 3 + 6 * n_freqs
    Xd, Fd = Guarded(x, cuda), Guarded(freqs, cuda)
    for ld, col in ((w, 0), ((w + 7) // 8 * 8 + 8, 0), (w + 9, 5)):
        want, exact = G.sinusoid(x, freqs[:n_freqs], ld - col)
        out = Guarded.empty((N, ld), f32, cuda)
        assert _lib().cnc_field_sinusoid(Xd.ptr, Fd.ptr, n_freqs, N, out.ptr, ld, col, _stream()) == 0
        torch.cuda.synchronize()
        got = out.get()
        assert out.intact() and Xd.intact() and Fd.intact()
        assert (got[:, :col].view(u32) == sentinel(u32)).all(), "columns left of col were written"
        got = got[:, col:]
        _assert_bits(got[:, exact], want[:, exact].astype(f32), f"x copy / padding (ld {ld}, col {col})")
        if n_freqs:
            err = _ulp_error(got[:, ~exact], want[:, ~exact])
            _note("sincosf ulp", err.max())
            assert err.max() <= 2 * SINCOS_ULP, (ld, col, float(err.max()))
    if n_freqs == 10 and N == 70001:
        # the kernel's claim that sincosf returns sinf's and cosf's values: the library's own kernels on the same products
        arg = torch.tensor(G.sinusoid_arguments(x, freqs), device=cuda)
        s, c = torch.sin(arg).cpu().numpy(), torch.cos(arg).cpu().numpy()
        mine = out.get()[:, col + 3:col + 3 + 6 * n_freqs].reshape(N, n_freqs, 2, 3)
        _note("sincosf != torch.sin (elements)", (mine[:, :, 0] != s).sum())
        _note("sincosf != torch.cos (elements)", (mine[:, :, 1] != c).sum())
        _note("torch.sin ulp", _ulp_error(s, np.sin(arg.cpu().numpy().astype(f64))).max())


def test_sinusoid_refusals(cuda):
    x, freqs = Guarded(_unit_points(8, 1), cuda), Guarded((2.0 ** np.arange(10)).astype(f32), cuda)
    out = Guarded.empty((8, 64), f32, cuda)
    for n_freqs, ld, col in ((1, 8, 9), (10, 62, 0), (10, 64, 2), (0, 2, 0)):
        assert _lib().cnc_field_sinusoid(x.ptr, freqs.ptr, n_freqs, 8, out.ptr, ld, col, _stream()) == INVALID
    assert _lib().cnc_field_sinusoid(None, freqs.ptr, 1, 8, out.ptr, 16, 0, _stream()) == INVALID
    torch.cuda.synchronize()
    assert _untouched(out) and out.intact()


# ------------------------------------------------------------------------------------------------------------------
# cnc_field_post / cnc_field_post_backward
# ------------------------------------------------------------------------------------------------------------------
B_ROWS = np.array([-100.0, 0.0, 1.0, 16.5, 89.5, np.nan, 100.0, 100.0, np.inf, -np.inf], f32)     # 100: expf overflows
B_SELECT = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1, 1], np.uint8)                                     # inf * 0 = NaN


def _directions(N, rng):
    d = rng.normal(size=(N, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    special = np.concatenate([np.eye(3), -np.eye(3), np.zeros((1, 3)), rng.normal(size=(9, 3)) * 2.5]).astype(f32)
    k = min(N, len(special))
    d[rng.permutation(N)[:k]] = special[(np.arange(k) + N) % len(special)]
    return d


def _base(N, ld_base, rng, rows, select):
    base = rng.normal(size=(N, ld_base)).astype(f32)
    base[:, 0] = rng.uniform(-6, 6, N)
    sel = (rng.uniform(size=N) < 0.7).astype(np.uint8)
    k = min(N, len(rows))
    at = rng.permutation(N)[:k]
    pick = (np.arange(k) + N) % len(rows)
    base[at, 0], sel[at] = rows[pick], select[pick]
    return base, sel


def _ld_options(geo):
    ld_base = [1 + geo, next(v for v in (16, 64, 72) if v > 1 + geo)]
    ld_head = (16 + geo + 3) // 4 * 4
    return ld_base, [ld_head, ld_head + 8]


def _check_density(got, base, sel):
    arg = G.density_argument(base[:, 0])
    with np.errstate(all="ignore"):
        ref64 = np.exp(arg.astype(f64))
        ref32 = ref64.astype(f32)                                   # float32's own overflow (inf) and underflow
        s = np.ones(len(arg), f32) if sel is None else sel.astype(f32)
        want = ref32 * s                                            # inf * 0 = NaN, NaN stays
    special = ~np.isfinite(want) | (s == 0)
    _assert_bits(got[special], want[special], "density where it is 0, inf or NaN")
    tiny = np.finfo(f32).tiny
    for name, rows, bound in (("expf ulp", ~special & (ref32 >= tiny), EXPF_ULP), ("expf ulp (subnormal results)", ~special & (ref32 < tiny), EXPF_SUB_ULP)):
        if rows.any():
            err = _ulp_error(got[rows], ref64[rows]).max()
            _note(name, err)
            assert err <= 2 * bound, (name, float(err))


def _post_cases(N):
    """(ld_base index, ld_head index, selector?, outputs, fp16): the full product for the small N, for N = 70,001 eight
    cases in which every option appears with every other output choice."""
    full = [(b, h, s, o, f) for b in (0, 1) for h in (0, 1) for s in (True, False) for o in ("density", "head", "both") for f in (0, SH_FP16)]
    if N < 1000:
        return full
    return [(0, 0, True, "both", 0), (1, 1, False, "both", SH_FP16), (0, 1, True, "head", SH_FP16), (1, 0, False, "head", 0),
            (0, 0, False, "density", 0), (1, 0, True, "density", 0), (1, 1, True, "both", 0), (0, 1, False, "both", SH_FP16)]


@pytest.mark.parametrize("geo", [1, 12, 15, 63])
@pytest.mark.parametrize("N", N_ROWS)
def test_post(cuda, N, geo):
    """density = expf(b - 1) * selector and head_in = [SH-4 (16) | geo features | zeros] from the base MLP's output: the
    harmonics (unit vectors, the six axes, the zero vector, unnormalised vectors; with and without the half round trip),
    the copied columns and the padding zeros bit for bit; the density against float64 exp of the float32 b - 1, with
    float32's own underflow, overflow and inf * 0 = NaN."""
    rng = np.random.default_rng(1000 * geo + N)
    dirs = _directions(N, rng)
    D = Guarded(dirs, cuda)
    lds_base, lds_head = _ld_options(geo)
    sh = {f: G.sh16(dirs, bool(f)) for f in (0, SH_FP16)}
    made = {}
    for bi, hi, with_sel, outputs, fp16 in _post_cases(N):
        ld_base, ld_head = lds_base[bi], lds_head[hi]
        if bi not in made:
            base, sel = _base(N, ld_base, rng, B_ROWS, B_SELECT)
            made[bi] = (base, sel, Guarded(base, cuda), Guarded(sel, cuda))
        base, sel, Bd, Sd = made[bi]
        den = Guarded.empty((N,), f32, cuda) if outputs != "head" else None
        head = Guarded.empty((N, ld_head), f32, cuda) if outputs != "density" else None
        rc = _lib().cnc_field_post(Bd.ptr, ld_base, geo, Sd.ptr if with_sel else None, D.ptr if head else None, N,
                                   den.ptr if den else None, head.ptr if head else None, ld_head if head else 0, fp16, _stream())
        torch.cuda.synchronize()
        what = f"ld_base {ld_base} ld_head {ld_head} selector {with_sel} {outputs} fp16 {fp16}"
        assert rc == 0, what
        if den:
            assert den.intact(), what
            _check_density(den.get(), base, sel if with_sel else None)
        if head:
            assert head.intact(), what
            want = np.zeros((N, ld_head), f32)
            want[:, :16] = sh[fp16]
            want[:, 16:16 + geo] = base[:, 1:1 + geo]
            _assert_bits(head.get(), want, what + ": head_in")
        assert Bd.intact() and Sd.intact() and D.intact()
    if N >= 255:
        assert not np.array_equal(sh[0], sh[SH_FP16])


def test_post_refusals(cuda):
    N, geo = 8, 12
    rng = np.random.default_rng(3)
    base, sel = _base(N, 16, rng, B_ROWS, B_SELECT)
    Bd, Sd, D = Guarded(base, cuda), Guarded(sel, cuda), Guarded(_directions(N, rng), cuda)
    den, head = Guarded.empty((N,), f32, cuda), Guarded.empty((N, 40), f32, cuda)
    post = _lib().cnc_field_post
    st = _stream()
    assert post(Bd.ptr, 12, geo, Sd.ptr, D.ptr, N, den.ptr, head.ptr, 28, 0, st) == INVALID          # ld_base < 1 + geo
    assert post(Bd.ptr, 16, geo, Sd.ptr, D.ptr, N, None, None, 28, 0, st) == INVALID                 # neither output
    assert post(Bd.ptr, 16, geo, Sd.ptr, None, N, den.ptr, head.ptr, 28, 0, st) == INVALID           # head_in without dirs
    assert post(Bd.ptr, 16, geo, Sd.ptr, D.ptr, N, den.ptr, head.ptr, 30, 0, st) == INVALID          # ld_head % 4
    assert post(Bd.ptr, 16, geo, Sd.ptr, D.ptr, N, den.ptr, head.ptr, 24, 0, st) == INVALID          # ld_head < 16 + geo
    assert post(Bd.ptr, 16, geo, Sd.ptr, D.ptr, N, den.ptr, head.ptr + 4, 28, 0, st) == INVALID      # misaligned head_in
    assert post(None, 16, geo, Sd.ptr, D.ptr, N, den.ptr, head.ptr, 28, 0, st) == INVALID
    back = _lib().cnc_field_post_backward
    gb = Guarded.empty((N, 16), f32, cuda)
    assert back(Bd.ptr, 12, geo, Sd.ptr, den.ptr, head.ptr, 28, N, gb.ptr, st) == INVALID            # ld_base < 1 + geo
    assert back(Bd.ptr, 16, geo, Sd.ptr, den.ptr, head.ptr, 24, N, gb.ptr, st) == INVALID            # ld_head < 16 + geo
    assert back(Bd.ptr, 16, geo, Sd.ptr, den.ptr, head.ptr, 28, N, None, st) == INVALID
    torch.cuda.synchronize()
    assert all(_untouched(b) and b.intact() for b in (den, head, gb))


BWD_ROWS = np.array([15.5, 16.0, 16.5, 41.0, -3.0, 1.0], f32)            # b - 1 = 14.5, 15, 15.5, 40: both sides of the clamp
BWD_SELECT = np.array([1, 1, 1, 1, 1, 0], np.uint8)


@pytest.mark.parametrize("geo", [1, 12, 15, 63])
@pytest.mark.parametrize("N", N_ROWS)
def test_post_backward(cuda, N, geo):
    """d base[:, 0] = (g_density * s) * expf(min(b - 1, 15)), d base[:, 1 + k] = g_head[:, 16 + k], zeros behind: the
    copies and zeros bit for bit, column 0 against float64 within the measured expf error and the product's one
    rounding; g_density NULL, g_head NULL, selector NULL."""
    rng = np.random.default_rng(2000 * geo + N)
    lds_base, lds_head = _ld_options(geo)
    cases = [(b, h, s, gd, gh) for b in (0, 1) for h in (0, 1) for s in (True, False) for gd in (True, False) for gh in (True, False)]
    if N > 1000:
        cases = [(0, 0, True, True, True), (1, 1, False, True, True), (1, 0, True, False, True), (0, 1, True, True, False),
                 (1, 1, False, False, False)]
    made = {}
    for bi, hi, with_sel, with_gd, with_gh in cases:
        ld_base, ld_head = lds_base[bi], lds_head[hi]
        if bi not in made:
            base, sel = _base(N, ld_base, rng, BWD_ROWS, BWD_SELECT)
            made[bi] = (base, sel, Guarded(base, cuda), Guarded(sel, cuda))
        if ("h", hi) not in made:
            gh = rng.normal(size=(N, ld_head)).astype(f32)
            made[("h", hi)] = (gh, Guarded(gh, cuda))
        if "d" not in made:
            gd = (rng.normal(size=N) * 10.0 ** rng.uniform(-3, 2, N)).astype(f32)
            made["d"] = (gd, Guarded(gd, cuda))
        (base, sel, Bd, Sd), (gh, GH), (gd, GD) = made[bi], made[("h", hi)], made["d"]
        out = Guarded.empty((N, ld_base), f32, cuda)
        rc = _lib().cnc_field_post_backward(Bd.ptr, ld_base, geo, Sd.ptr if with_sel else None, GD.ptr if with_gd else None,
                                            GH.ptr if with_gh else None, ld_head, N, out.ptr, _stream())
        torch.cuda.synchronize()
        what = f"ld_base {ld_base} ld_head {ld_head} selector {with_sel} g_density {with_gd} g_head {with_gh}"
        assert rc == 0 and out.intact(), what
        got = out.get()
        want = np.zeros((N, ld_base), f32)
        if with_gh:
            want[:, 1:1 + geo] = gh[:, 16:16 + geo]
        _assert_bits(got[:, 1:], want[:, 1:], what + ": columns 1 ..")
        if not with_gd:
            _assert_bits(got[:, 0], want[:, 0], what + ": column 0 without g_density")
            continue
        s = sel.astype(f32) if with_sel else np.ones(N, f32)
        gs = (gd * s).astype(f64)                                          # the float32 product, exact in either
        ref = gs * np.exp(np.minimum(G.density_argument(base[:, 0]).astype(f64), 15.0))
        # expf within 2 EXPF_ULP ulp = 2 EXPF_ULP 2^-23 relative at most, then one rounded product: 2^-24
        bound = np.abs(ref) * (2 * EXPF_ULP * 2.0 ** -23 + 2.0 ** -24) * (1 + 2.0 ** -20) + np.finfo(f32).smallest_subnormal
        err = np.abs(got[:, 0].astype(f64) - ref)
        _note("post_backward column 0, error / bound", (err / bound).max())
        assert (err <= bound).all(), (what, float((err / bound).max()))
        zero = gs == 0
        assert (got[zero, 0] == 0).all()
    if N >= 255:
        assert (G.density_argument(made[0][0][:, 0]) > 15).sum() >= 2          # rows the clamp acts on


# ------------------------------------------------------------------------------------------------------------------
# cnc_relu_backward_bias
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [4, 12, 64, 80, 96, 160, 252, 256])
@pytest.mark.parametrize("N", [1, 255, 257, 262144, 262145, 640003])
def test_relu_backward_bias(cuda, N, C_):
    """grad_in = where(y > 0, grad_out, 0) bit for bit (y = 0, -0.0 and NaN: 0); exactly
    cnc_relu_backward_bias_partials(N) rows of partial sums, whose float64 column sums lie within c 2^-24 sum|g| of the
    float64 column sums (c: the module docstring).  C = 12, 252 leave idle lanes; above N = 262,144 a block takes more than
    256 rows and the grid stays at 1,024 blocks.  Inputs and reference are made on the device (1.3 GB at the largest)."""
    g = torch.Generator(device=cuda).manual_seed(N * 1000 + C_)
    go = torch.randn(N, C_, device=cuda, generator=g)
    y = torch.randn(N, C_, device=cuda, generator=g)
    flat = y.view(-1)
    k = min(flat.numel(), 12)
    at = torch.randint(0, flat.numel(), (k,), device=cuda, generator=g)
    flat[at] = torch.tensor([0.0, -0.0, float("nan"), float("inf")], device=cuda).repeat(3)[:k]
    P = _lib().cnc_relu_backward_bias_partials(N)
    assert P == min((N + 255) // 256, 1024)
    GO, Y = Guarded.like(go), Guarded.like(y)
    GI, PART = Guarded.empty((N, C_), f32, cuda), Guarded.empty((P, C_), f32, cuda)
    assert _lib().cnc_relu_backward_bias(GO.ptr, Y.ptr, N, C_, GI.ptr, PART.ptr, _stream()) == 0
    torch.cuda.synchronize()
    want = torch.where(y > 0, go, torch.zeros((), device=cuda))
    assert torch.equal(GI.tensor().view(torch.int32), want.view(torch.int32))
    assert all(b.intact() for b in (GO, Y, GI, PART))
    assert torch.equal(GO.tensor(), go) and torch.equal(Y.tensor().view(torch.int32), y.view(torch.int32))
    part = PART.tensor()
    assert not bool((part.view(torch.int32) == int(sentinel(np.int32))).any()), "a partial row was not written"
    rows_per_block = (N + P - 1) // P
    R = 256 // (C_ // 4)
    c = (rows_per_block + R - 1) // R + R + 1
    A = want.abs().double().sum(0)
    err = (part.double().sum(0) - want.double().sum(0)).abs()
    bound = c * 2.0 ** -24 * A
    ok = err <= bound
    _note("bias sums, error / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert bool(ok.all()), float((err / bound.clamp_min(1e-300)).max())


def test_relu_backward_bias_refusals(cuda):
    N = 16
    go, y = (Guarded(np.ones((N, 264), f32), cuda) for _ in range(2))
    gi, part = Guarded.empty((N, 264), f32, cuda), Guarded.empty((4, 264), f32, cuda)
    f = _lib().cnc_relu_backward_bias
    st = _stream()
    for C_ in (6, 0, 260, 258):
        assert f(go.ptr, y.ptr, N, C_, gi.ptr, part.ptr, st) == INVALID, C_
    assert f(go.ptr + 4, y.ptr, N, 8, gi.ptr, part.ptr, st) == INVALID
    assert f(go.ptr, y.ptr + 4, N, 8, gi.ptr, part.ptr, st) == INVALID
    assert f(go.ptr, y.ptr, N, 8, gi.ptr + 4, part.ptr, st) == INVALID
    assert f(go.ptr, y.ptr, N, 8, gi.ptr, None, st) == INVALID
    torch.cuda.synchronize()
    assert _untouched(gi) and _untouched(part) and gi.intact() and part.intact()


# ------------------------------------------------------------------------------------------------------------------
# cnc_ste_binary_forward / _backward
# ------------------------------------------------------------------------------------------------------------------
def _ste_data(n, seed):
    one = f32(1)
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(one, f32(2)), np.nextafter(one, f32(0)), np.nextafter(-one, f32(-2)),
                   np.nextafter(-one, f32(0)), np.inf, -np.inf, np.nan, 1e-40, -1e-40], f32)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, n).astype(f32)
    k = min(n, 4 * sp.size)
    x[rng.permutation(n)[:k]] = sp[(np.arange(k) + n) % sp.size]
    return x


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025])
def test_ste_binary(cuda, n):
    """forward (c >= 0) - (c < 0) of c = clamp(x, -1, 1), backward g * ((x >= -1) & (x <= 1)), on 0, -0.0, +-1, their
    neighbours, +-inf, NaN and a subnormal: bit for bit; n around the float4 width and the 1,024-element block."""
    x = _ste_data(n, n)
    g = (np.random.default_rng(n + 1).normal(size=n) * 3).astype(f32)
    X, GR = Guarded(x, cuda), Guarded(g, cuda)
    out, gin = Guarded.empty((n,), f32, cuda), Guarded.empty((n,), f32, cuda)
    assert _lib().cnc_ste_binary_forward(X.ptr, out.ptr, n, _stream()) == 0
    assert _lib().cnc_ste_binary_backward(X.ptr, GR.ptr, gin.ptr, n, _stream()) == 0
    torch.cuda.synchronize()
    _assert_bits(out.get(), G.ste_forward(x), "forward")
    _assert_bits(gin.get(), G.ste_backward(x, g), "backward")
    assert all(b.intact() for b in (X, GR, out, gin))
    assert np.array_equal(X.get().view(u32), x.view(u32)) and np.array_equal(GR.get().view(u32), g.view(u32))


def test_ste_binary_refusals(cuda):
    x, g = Guarded(_ste_data(64, 0), cuda), Guarded(np.ones(64, f32), cuda)
    out = Guarded.empty((64,), f32, cuda)
    fwd, bwd = _lib().cnc_ste_binary_forward, _lib().cnc_ste_binary_backward
    st = _stream()
    assert fwd(x.ptr + 4, out.ptr, 32, st) == INVALID and fwd(x.ptr, out.ptr + 4, 32, st) == INVALID
    assert fwd(None, out.ptr, 32, st) == INVALID and fwd(x.ptr, None, 32, st) == INVALID
    assert bwd(x.ptr + 4, g.ptr, out.ptr, 32, st) == INVALID and bwd(x.ptr, g.ptr + 4, out.ptr, 32, st) == INVALID
    assert bwd(x.ptr, g.ptr, out.ptr + 4, 32, st) == INVALID and bwd(x.ptr, None, out.ptr, 32, st) == INVALID
    torch.cuda.synchronize()
    assert _untouched(out) and out.intact()
