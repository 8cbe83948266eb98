"""`extract_mesh(..., min_component_points=k)`: the lattice's inside set is pruned with the Kuhn neighbourhood
before the surface is cut.  A ready float32 lattice [41, 37, 45] with one large ball and four small blobs; one blob — a
single point — touches the ball only along a mixed-sign diagonal, so it is a component of its own at connectivity 14 (and
would not be at 26); one blob lies against the box, where the cap takes its boundary points out of the inside set.  The
mesh must be bit-equal to the mesh of the lattice the NumPy twin pruned (tests/components_twin.py)."""
import numpy as np
import pytest
import torch

import components_twin as C
import mesh_twin as T
from guarded import same_bits

pytestmark = pytest.mark.gpu

SHAPE = (41, 37, 45)
AABB = [-1.1, -0.9, -1.0, 1.1, 0.9, 1.0]
THRESHOLD = 1.0


def _diagonal_point(ball):
    """The first lattice point outside `ball` that has a ball point among its 26 neighbours and none among its 14."""
    def touched(connectivity):
        out = np.zeros_like(ball)
        for o in C.offsets(connectivity):
            out |= np.roll(ball, o, axis=(0, 1, 2))            # the ball is far from the box: nothing wraps
        return out
    q = np.flatnonzero(touched(26) & ~touched(14) & ~ball)
    assert q.size
    return np.unravel_index(int(q[0]), ball.shape)


def _scene():
    z, y, x = np.indices(SHAPE)
    ball = (z - 20) ** 2 + (y - 18) ** 2 + (x - 22) ** 2 <= 81
    inside = ball.copy()
    q = _diagonal_point(ball)
    inside[q] = True                                            # blob 1: one point, diagonal to the ball
    inside[34:37, 30:32, 5:7] = True                            # blob 2: 12 points
    inside[(z - 6) ** 2 + (y - 6) ** 2 + (x - 38) ** 2 <= 5] = True        # blob 3: 57 points
    inside[0:3, 5:7, 5:7] = True                                # blob 4: against the box, 8 points behind the cap
    rng = np.random.default_rng(17)
    D = np.where(inside, 1.25 + rng.random(SHAPE), 0.75 * rng.random(SHAPE)).astype(np.float32)
    D[3, 30, 40] = np.nan                                       # NaN is outside
    return D, q


@pytest.fixture(scope="module")
def scene(cuda):
    D, q = _scene()
    capped = T.capped(D)
    with np.errstate(invalid="ignore"):
        inside = capped >= THRESHOLD
    labels = C.label_grid(inside, 14)
    sizes = np.sort(C.sizes(labels)[C.sizes(labels) > 0])
    assert sizes.tolist() == [1, 8, 12, 57, int(sizes[-1])] and sizes[-1] > 2000
    assert labels[q] == q[0] * SHAPE[1] * SHAPE[2] + q[1] * SHAPE[2] + q[2]            # on its own at 14 ...
    assert C.n_components(C.label_grid(inside, 26)) == 4                                 # ... and part of the ball at 26
    return D, inside, torch.from_numpy(D).to(cuda)


def _canonical(mesh):
    return T.canonical_faces(mesh.faces.cpu().numpy())


@pytest.mark.parametrize("k,removed", [(1, 0), (2, 1), (9, 2), (13, 3), (58, 4), (10 ** 9, 4)])
def test_pruned_mesh_is_the_mesh_of_the_twins_pruned_lattice(scene, k, removed):
    from cnc_amd.mesh import extract_mesh
    D, inside, dev = scene
    kept, stats = C.prune_small(inside, k, 14)
    assert stats["removed_components"] == removed and stats["components"] == 5
    want_lattice = D.copy()
    want_lattice[inside & ~kept] = 0.0
    want = extract_mesh(torch.from_numpy(want_lattice).to(dev.device), AABB, threshold=THRESHOLD)
    before = dev.clone()
    mesh, lattice = extract_mesh(dev, AABB, threshold=THRESHOLD, min_component_points=k, return_lattice=True)
    assert same_bits(dev, before)                                                        # the caller's lattice is not modified
    assert same_bits(lattice, T.capped(want_lattice))                                    # the returned lattice is the pruned one
    assert same_bits(mesh.vertices, want.vertices) and same_bits(mesh.normals, want.normals)
    assert np.array_equal(_canonical(mesh), _canonical(want))
    V = mesh.vertices.shape[0]
    assert V > 0 and T.is_directed_manifold(mesh.faces.cpu().numpy(), V)                 # still closed
    assert mesh.components().size == 5 - removed
    assert np.array_equal(mesh.components(on_device=True), mesh.components())


def test_zero_is_todays_mesh(scene):
    from cnc_amd.mesh import extract_mesh
    _, _, dev = scene
    plain, plain_lattice = extract_mesh(dev, AABB, threshold=THRESHOLD, return_lattice=True)
    mesh, lattice = extract_mesh(dev, AABB, threshold=THRESHOLD, min_component_points=0, return_lattice=True)
    assert same_bits(mesh.vertices, plain.vertices) and same_bits(mesh.normals, plain.normals) and same_bits(mesh.faces, plain.faces)
    assert same_bits(lattice, plain_lattice) and plain.components().size == 5
    with pytest.raises(ValueError):
        extract_mesh(dev, AABB, threshold=THRESHOLD, min_component_points=-1)


def test_uncapped_boundary_points_count(scene):
    """cap=False: the blob against the box keeps its boundary points (12 instead of 8), so k = 9 no longer removes it."""
    from cnc_amd.mesh import extract_mesh
    D, _, dev = scene
    with np.errstate(invalid="ignore"):
        inside = D >= THRESHOLD
    kept, stats = C.prune_small(inside, 9, 14)
    assert stats["removed_components"] == 1
    want_lattice = D.copy()
    want_lattice[inside & ~kept] = 0.0
    _, lattice = extract_mesh(dev, AABB, threshold=THRESHOLD, cap=False, min_component_points=9, return_lattice=True)
    assert same_bits(lattice, want_lattice)
