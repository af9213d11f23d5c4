"""The meshes of tests/test_meshclean_*.py, built once per process and read-only: marching-cubes surfaces of the fields of
tests/mesh_fields.py at threshold 0 (host path) and a hand-made ribbon.  CASES holds what was counted for each on the host."""
import functools

import numpy as np

from tests import mesh_fields as mf

CASES = {
    'ribbon': dict(vertices=4112, faces=4103, classes=9),
    'sphere_rod_torus': dict(vertices=11410, faces=22816, classes=2, largest=[14656, 8160]),
    'checker16': dict(vertices=7808, faces=16532, classes=39, largest=[16212, 16, 16]),
    'checker16_shuffled': dict(vertices=7808, faces=16532, classes=39, largest=[16212, 16, 16]),
    'checker32': dict(vertices=55672, faces=118664, classes=272),
}


def ribbon():
    """The diameter case: a strip of 4096 triangles (i, i + 1, i + 2) whose 4098 vertex ids are shuffled, so that its graph diameter
    is ~2048 and the smallest index sits somewhere in the middle; then 3 unreferenced vertices, a second strip of 5 triangles on
    7 vertices, 4 unreferenced vertices; a duplicated face and a face with a repeated index at the end."""
    g = np.random.RandomState(0)
    perm = g.permutation(4098)
    i = np.arange(4096)
    strip = perm[np.stack([i, i + 1, i + 2], axis=1)]
    j = np.arange(5)
    second = 4101 + np.stack([j, j + 1, j + 2], axis=1)
    faces = np.concatenate([strip, second, strip[1000:1001], np.array([[4103, 4103, 4106]])]).astype(np.int64)
    vertices = g.rand(4112, 3)
    return vertices, faces


def _shuffled(v, f, seed):
    """The same mesh with its vertex ids permuted and its faces in another order: the smallest index of a component is then not the
    first one met."""
    g = np.random.RandomState(seed)
    new_id = g.permutation(len(v))
    out_v = np.empty_like(v)
    out_v[new_id] = v
    return out_v, new_id[f][g.permutation(len(f))]


@functools.lru_cache(maxsize=None)
def case(name):
    from psnerf_amd.stage1.extracting import host_marching_cubes
    if name == 'ribbon':
        v, f = ribbon()
    elif name == 'checker16_shuffled':
        v, f = _shuffled(*case('checker16'), seed=5)
    else:
        field = {'sphere_rod_torus': lambda: mf.sphere_rod_torus(64), 'checker16': lambda: mf.checker(16),
                 'checker32': lambda: mf.checker(32, seed=1)}[name]()
        v, f = host_marching_cubes(field, 0.0)
    v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
    v.flags.writeable = f.flags.writeable = False
    return v, f
