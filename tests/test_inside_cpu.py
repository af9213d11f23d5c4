"""The crossing-count definition meshdist.host_crossings (and _HostMesh.crossings / contains over it) on meshes whose inside is known
without it.  The point of every case is the tie rule: lattice-aligned queries send their lines exactly through vertices and edges,
and the parity must still be the inside -- with nothing excluded."""
import numpy as np

from tests import inside_cases as ic
from tests import raycast_cases as rc
from psnerf_amd import meshdist as md


def _inside_open(v, f, points, axis):
    above, below, on = md.host_crossings(v, f, points, axis)
    assert above.dtype == below.dtype == on.dtype == np.int32 and above.shape == below.shape == on.shape == (len(points),)
    return (above & 1) == 1, ((above + below + on) & 1) == 1, (above, below, on)


def test_box_is_half_open():
    """inside == (lo <= p < hi) on all three axes whatever the axis of the line, on faces, edges and corners too; no line is open."""
    points = ic.box_lattice()
    want = ((points >= ic.BOX_LO) & (points < ic.BOX_HI)).all(axis=1)
    on_surface = ((points == ic.BOX_LO) | (points == ic.BOX_HI)).any(axis=1) & ((points >= ic.BOX_LO) & (points <= ic.BOX_HI)).all(axis=1)
    assert int(on_surface.sum()) == 9 ** 3 - 7 ** 3 and 0 < int(want.sum()) == 8 ** 3
    for seed in (0, 1, 2):
        v, f = ic.box(seed)
        for axis in range(3):
            inside, line_open, (above, below, on) = _inside_open(v, f, points, axis)
            assert np.array_equal(inside, want), 'seed %d axis %d: %d points differ' % (seed, axis, int((inside != want).sum()))
            assert not line_open.any()
            assert int((on > 0).sum()) > 0 and above.max() <= 2 and (above + below + on).max() == 2


def _check_lattice(case, axis):
    v, f, field, lattice = case
    inside, line_open, _ = _inside_open(v, f, lattice, axis)
    return inside, line_open, field > 0.0


def test_marching_cubes_sphere_on_its_own_lattice():
    """Every point of the padded lattice is inside exactly where the field is, on all three axes, with zero points excluded.  The case
    rests on one condition, asserted here: no lattice value equals the threshold (then no lattice point lies ON the surface)."""
    v, f, field, lattice = ic.mc_sphere()
    assert not (field == 0.0).any()
    assert len(lattice) == 19 ** 3 and len(v) > 400 and len(f) * len(lattice) <= 2e7
    on_lines = (np.abs(v - np.round(v)) < 1e-12).sum(axis=1)
    assert (on_lines >= 2).all()                                  # every vertex on a lattice line: every query line meets vertices
    for axis in range(3):
        inside, line_open, want = _check_lattice((v, f, field, lattice), axis)
        assert np.array_equal(inside, want), 'axis %d: %d of %d points differ' % (axis, int((inside != want).sum()), len(want))
        assert not line_open.any()
    assert 0 < int(want.sum()) < len(want)


def test_marching_cubes_torus_axes_agree():
    v, f, field, lattice = ic.mc_torus()
    assert not (field == 0.0).any()
    results = [_check_lattice((v, f, field, lattice), axis) for axis in range(3)]
    for axis, (inside, line_open, want) in enumerate(results):
        assert np.array_equal(inside, results[0][0]), 'axis %d disagrees with axis 0' % axis
        assert not line_open.any()
    assert np.array_equal(results[0][0], results[0][2]) and 0 < int(results[0][2].sum())


def test_hemisphere_is_open_and_the_vote_differs():
    v, f = ic.hemisphere(2)
    g = np.random.RandomState(3)
    points = (g.random_sample((3000, 3)) - 0.5) * 2.2
    mesh = md._HostMesh(v, f)
    single = mesh.contains(points, axis=2)
    vote = mesh.contains(points, vote=True)
    line_open = _inside_open(v, f, points, 2)[1]
    assert single.dtype == np.bool_ and vote.dtype == np.bool_
    assert 0 < int(line_open.sum()) < len(points)
    assert int((single != vote).sum()) > 0
    # well under the (jagged) rim, inside the ball: the dome is overhead, and no horizontal line meets it
    below_dome = (np.linalg.norm(points, axis=1) < 0.9) & (points[:, 2] < -0.35)
    assert single[below_dome].all() and not vote[below_dome].any() and int(below_dome.sum()) > 100
    assert np.array_equal(single, mesh.contains(points, axis=2)) and np.array_equal(vote, mesh.contains(points, vote=True))


def test_nested_spheres():
    v, f = ic.nested(2, 0.5)
    r_in = rc.inner_radius(*rc.icosphere(2))
    g = np.random.RandomState(4)
    points = (g.random_sample((4000, 3)) - 0.5) * 2.4
    r = np.linalg.norm(points, axis=1)
    inside, line_open, (above, below, on) = _inside_open(v, f, points, 2)
    core, shell, outer = r < 0.5 * r_in, (r > 0.5) & (r < r_in), r > 1.0
    assert min(int(core.sum()), int(shell.sum()), int(outer.sum())) > 50
    assert not inside[core].any() and inside[shell].all() and not inside[outer].any() and not line_open.any()
    assert (above[core] == 2).all() and (below[core] == 2).all() and above.max() == 4 and (above[shell] % 2 == 1).all()
    centre = md.host_crossings(v, f, np.array([[0.01, 0.02, -0.03]]), 2)
    assert (int(centre[0][0]), int(centre[1][0]), int(centre[2][0])) == (2, 2, 0)


def test_non_finite_points_give_zeros():
    v, f = rc.icosphere(1)
    points = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3, [0.01, 0.02, 0.03]])
    for axis in range(3):
        above, below, on = md.host_crossings(v, f, points, axis)
        assert not above[:4].any() and not below[:4].any() and not on[:4].any()
        assert (above[4], below[4], on[4]) == (1, 1, 0)


def test_awkward_meshes_run():
    """A single triangle, degenerate triangles, a flat bounding box, two oversize triangles: the query runs, counts are small
    non-negative integers (no NaN has anywhere to escape to), and the degenerate rows are never counted."""
    g = np.random.RandomState(6)
    for name, (v, f) in rc.awkward_meshes().items():
        lo, hi = v.min(0), v.max(0)
        points = np.concatenate([lo + g.random_sample((300, 3)) * (hi - lo), v[f[:100, 0]], v[f[:100]].mean(axis=1)])
        for axis in range(3):
            above, below, on = md.host_crossings(v, f, points, axis)
            assert above.min() >= 0 and below.min() >= 0 and on.min() >= 0 and (above + below + on).max() <= len(f), name
            if name == 'degenerate triangles':
                rest = md.host_crossings(v, f[rc.N_REPEATED:], points, axis)
                assert all(np.array_equal(a, b) for a, b in zip((above, below, on), rest)), name
    v, f = rc.awkward_meshes()['a single triangle']
    centroid = v.mean(axis=0)
    for axis in range(3):
        p = np.stack([centroid, centroid, centroid])
        p[0, axis] -= 1.0
        p[2, axis] += 1.0
        above, below, on = md.host_crossings(v, f, p, axis)
        assert list(above + 2 * below) in ([1, 0, 2], [1, 1, 2], [1, 2, 2]) and list(above + below + on) == [1, 1, 1]
    with np.testing.assert_raises(ValueError):
        md.host_crossings(v, f, p, 3)
    with np.testing.assert_raises(ValueError):
        md.host_crossings(v, f[:0], p, 2)


def test_volume_of_a_closed_mesh():
    """icosphere(3): the share of 20 000 uniform points found inside, times the box's volume, against the exact enclosed volume; the
    gap may be 5 binomial standard deviations (derived in inside_cases.five_sigma)."""
    v, f = rc.icosphere(3)
    n = 20000
    lo, hi = v.min(0) - 0.05, v.max(0) + 0.05
    box = float(np.prod(hi - lo))
    exact = ic.volume(v, f)
    assert 4.0 < exact < 4.0 * np.pi / 3.0
    points = lo + np.random.RandomState(8).random_sample((n, 3)) * (hi - lo)
    mesh = md._HostMesh(v, f)
    allowed = ic.five_sigma(exact / box, n, box)
    found = float(mesh.contains(points).sum()) / n * box
    print('volume %.5f, exact %.5f, allowed gap %.5f' % (found, exact, allowed))
    assert abs(found - exact) <= allowed
