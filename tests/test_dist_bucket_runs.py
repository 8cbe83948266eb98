"""`GradBucket.runs_excluding` (cnc_amd/dist.py): the contiguous runs of the flat gradient buffer that belong to none of a
given parameter list — what the data-parallel step still divides by the world size once the tables' mean is taken inside
their optimizer kernel.  No GPU: tiny CPU parameters.  The runs and the excluded parameters' slices must tile the gradient
part exactly, in order, and never reach the tail slots."""
import pytest
import torch

from cnc_amd.dist import GradBucket

SHAPES = [(3, 4), (5,), (2, 2, 2), (1,), (7,), (4, 3)]          # 12, 5, 8, 1, 7, 12 elements: offsets 0, 12, 17, 25, 26, 33, 45


def _bucket(tail):
    params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    return params, GradBucket(params, tail=tail)


def _slices(bucket):
    out, o = {}, 0
    for p in bucket.params:
        out[id(p)] = (o, o + p.numel())
        o += p.numel()
    return out


CASES = {
    "none": ([], [(0, 45)]),
    "first": ([0], [(12, 45)]),
    "last": ([5], [(0, 33)]),
    "first and last": ([0, 5], [(12, 33)]),
    "adjacent": ([1, 2], [(0, 12), (25, 45)]),
    "adjacent at the front": ([0, 1, 2, 3], [(26, 45)]),
    "interleaved": ([0, 2, 4], [(12, 17), (25, 26), (33, 45)]),
    "interleaved, the other half": ([1, 3, 5], [(0, 12), (17, 25), (26, 33)]),
    "all": ([0, 1, 2, 3, 4, 5], []),
}


@pytest.mark.parametrize("tail", [0, 1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_runs_and_excluded_slices_tile_the_gradients(name, tail):
    which, want = CASES[name]
    params, b = _bucket(tail)
    skip = [params[k] for k in which]
    runs = b.runs_excluding(skip)
    assert runs == want
    assert runs == b.runs_excluding(reversed(skip))                        # the order of the list does not matter
    at = _slices(b)
    pieces = sorted(runs + [at[id(p)] for p in skip])
    joined = [pieces[0]] if pieces else []
    for lo, hi in pieces[1:]:
        assert lo == joined[-1][1], "a gap or an overlap"
        joined[-1] = (joined[-1][0], hi)
    assert joined == [(0, b.numel)] and b.numel == 45
    assert all(0 <= lo < hi <= b.numel for lo, hi in runs)                  # never the tail: flat[numel:]
    assert all(runs[k][1] < runs[k + 1][0] for k in range(len(runs) - 1))   # maximal: neighbours are merged


def test_dividing_the_runs_leaves_the_excluded_and_the_tail_alone():
    """What the Trainer does with the runs: one in-place division each."""
    params, b = _bucket(tail=2)
    b.flat.copy_(torch.arange(1, b.flat.numel() + 1, dtype=torch.float32))
    before = b.flat.clone()
    skip = [params[0], params[2], params[3]]
    for lo, hi in b.runs_excluding(skip):
        b.flat[lo:hi].div_(4)
    at = _slices(b)
    for p, v in zip(b.params, b.views):
        lo, hi = at[id(p)]
        assert v.data_ptr() == b.flat[lo:hi].data_ptr()
        want = before[lo:hi] if any(p is q for q in skip) else before[lo:hi] / 4
        assert torch.equal(b.flat[lo:hi], want)
    assert torch.equal(b.tail, before[b.numel:]) and b.tail.numel() == 2


def test_frozen_and_foreign_parameters():
    """A parameter without requires_grad is not in the bucket (nor in its offsets); one the bucket does not hold is an error."""
    params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    params[1].requires_grad_(False)
    b = GradBucket(params, tail=1)
    assert b.runs_excluding([params[2]]) == [(0, 12), (20, 40)]
    with pytest.raises(ValueError):
        b.runs_excluding([params[1]])
    with pytest.raises(ValueError):
        b.runs_excluding([torch.nn.Parameter(torch.zeros(3))])

