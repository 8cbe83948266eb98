"""`cnc_amd.dist.fold_entropy_gradients`: the data-parallel step's gradient assembly behind the all-reduce — one path,
parameterised by the parameters whose gradient is not folded into the bucket — against the four bodies the Trainer used to
spell out for {tables through their Adam kernel, through the library} x {entropy gradients returned by autograd, accumulated
into a second bucket}, written out literally below.  No GPU: small CPU parameters, with "tables" first, in the middle and
last among the others, random values, and world = 3 (not a power of two: a stray `* (1 / world)` in place of `/ world`
would show).  Every comparison is bit for bit."""
import pytest
import torch

from cnc_amd.dist import GradBucket, fold_entropy_gradients

SHAPES = [(8, 4), (5,), (3, 7), (6, 4), (1,), (2, 2, 2), (4, 4)]       # tables: 0 (first), 3 (middle), 6 (last)
TABLES = (0, 3, 6)
WORLD = 3


def _setup(seed):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    A, B = GradBucket(params, tail=2), GradBucket(params)
    A.flat.copy_(torch.randn(A.flat.shape, generator=g) * 100.0)
    B.flat.copy_(torch.randn(B.flat.shape, generator=g))
    # what torch.autograd.grad(..., allow_unused=True) returns: one tensor per parameter, None where the loss does not reach
    # (a table among them), one of the tables' not contiguous
    grads = [torch.randn(s, generator=g) for s in SHAPES]
    grads[1] = grads[6] = None
    grads[3] = torch.randn((4, 6), generator=g).t()
    assert not grads[3].is_contiguous() and grads[3].shape == SHAPES[3]
    return params, A, B, grads


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_pieces(got, want):
    assert set(got) == set(want)
    for k in want:
        assert len(got[k]) == len(want[k]) == 1
        (g, rows), (w, wrows) = got[k][0], want[k][0]
        assert rows is None and wrows is None and g.is_contiguous() and torch.equal(_bits(g), _bits(w))


# ---- the four former bodies, as the Trainer had them (A: the ray loss's bucket behind the all-reduce, B: the entropy loss's)
def _kernel_returned(A, tables, ctx_grads, world):
    tids = {id(p) for p in tables}
    runs = A.runs_excluding(tables)
    table_pieces = {}
    for lo, hi in runs:
        A.flat[lo:hi].div_(world)
    pairs = [(v, g) for p, v, g in zip(A.params, A.views, ctx_grads) if g is not None and id(p) not in tids]
    if pairs:
        torch._foreach_add_([v for v, _ in pairs], [g for _, g in pairs])
    for p, g in zip(A.params, ctx_grads):
        if g is not None and id(p) in tids:
            table_pieces[id(p)] = [(g if g.is_contiguous() else g.contiguous(), None)]
    return table_pieces


def _kernel_bucket(A, B, tables, world):
    tids = {id(p) for p in tables}
    runs = A.runs_excluding(tables)
    table_pieces = {}
    for lo, hi in runs:
        A.flat[lo:hi].div_(world)
    for lo, hi in runs:
        A.flat[lo:hi].add_(B.flat[lo:hi])
    for p, v in zip(B.params, B.views):
        if id(p) in tids:
            table_pieces[id(p)] = [(v, None)]
    return table_pieces


def _library_returned(A, ctx_grads, world):
    A.grads.div_(world)
    pairs = [(v, g) for v, g in zip(A.views, ctx_grads) if g is not None]
    torch._foreach_add_([v for v, _ in pairs], [g for _, g in pairs])


def _library_bucket(A, B, world):
    A.grads.div_(world)
    A.grads.add_(B.flat)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("cell", ["kernel, returned", "kernel, bucket", "library, returned", "library, bucket"])
def test_one_path_equals_the_four_former_bodies(cell, seed):
    params, A, B, grads = _setup(seed)
    params_w, A_w, B_w, grads_w = _setup(seed)                       # the same values, for the former body
    assert torch.equal(_bits(A.flat), _bits(A_w.flat)) and torch.equal(_bits(B.flat), _bits(B_w.flat))
    before = A.flat.clone()
    kernel, returned = cell.startswith("kernel"), cell.endswith("returned")
    tables, tables_w = [params[k] for k in TABLES], [params_w[k] for k in TABLES]
    got = fold_entropy_gradients(A, tables if kernel else (), WORLD, grads=grads if returned else None,
                                 other=None if returned else B)
    if kernel and returned:
        want = _kernel_returned(A_w, tables_w, grads_w, WORLD)
    elif kernel:
        want = _kernel_bucket(A_w, B_w, tables_w, WORLD)
    elif returned:
        want, _ = {}, _library_returned(A_w, grads_w, WORLD)
    else:
        want, _ = {}, _library_bucket(A_w, B_w, WORLD)
    assert torch.equal(_bits(A.flat), _bits(A_w.flat))
    assert torch.equal(_bits(B.flat), _bits(B_w.flat))               # the entropy loss's bucket is read, never written
    key = {id(p): id(q) for p, q in zip(params, params_w)}
    _same_pieces({key[k]: v for k, v in got.items()}, want)
    # what the comparison cannot see if both sides shared a mistake: the tail rides untouched, a table the kernel steps keeps
    # the collective's sum, everything else moved, and the pieces are the tables the entropy loss reaches
    assert torch.equal(A.tail, before[A.numel:]) and A.tail.numel() == 2
    o = 0
    for k, p in enumerate(params):
        kept = torch.equal(_bits(A.flat[o:o + p.numel()]), _bits(before[o:o + p.numel()]))
        assert kept == (kernel and k in TABLES), (k, kept)
        o += p.numel()
    reached = [k for k in TABLES if not returned or grads[k] is not None]
    assert sorted(got) == sorted(id(params[k]) for k in reached) if kernel else not got
    if kernel and not returned:
        assert all(got[id(params[k])][0][0].data_ptr() == B.views[k].data_ptr() for k in TABLES)


def test_division_is_a_division():
    """world = 3: `x / 3` and `x * float32(1 / 3)` differ for some of these values, so the test above tells them apart."""
    _, A, _, _ = _setup(0)
    third = float(torch.tensor(1.0) / 3)
    assert not torch.equal(A.grads / 3, A.grads * third)


def test_no_entropy_loss():
    """lmbda = 0: nothing to add, the runs are divided and the tables' entropy pieces are none."""
    params, A, _, _ = _setup(2)
    before = A.flat.clone()
    assert fold_entropy_gradients(A, [params[k] for k in TABLES], WORLD) == {}
    want = before.clone()
    for lo, hi in A.runs_excluding([params[k] for k in TABLES]):
        want[lo:hi] /= WORLD
    assert torch.equal(_bits(A.flat), _bits(want))
