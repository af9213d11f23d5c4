"""What the mesh modules share (psnerf_amd/meshcore.py), without a GPU: the forms a mesh is unpacked from, the host validator's
errors under every caller's prefix, the cross product on numpy arrays and CPU tensors, and the writer / reader round trip."""
import types

import numpy as np
import pytest
import torch

from psnerf_amd import meshbake, meshclean, meshcore as core, meshdist, meshsimplify

TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)


def test_mesh_parts_takes_every_form():
    n = np.ones((4, 3), dtype=np.float32)
    for mesh, normals in ((core.Mesh(TET_V, TET_F), None), (core.Mesh(TET_V, TET_F, n), n),
                          (types.SimpleNamespace(vertices=TET_V, faces=TET_F), None),
                          (types.SimpleNamespace(vertices=TET_V, faces=TET_F, vertex_normals=n), n),
                          ((TET_V, TET_F), None), ([TET_V, TET_F], None), ((TET_V, TET_F, n), n), ((TET_V, TET_F, None), None)):
        v, f, vn = core.mesh_parts(mesh)
        assert np.array_equal(v, TET_V) and np.array_equal(f, TET_F) and (vn is None if normals is None else np.array_equal(vn, normals))
    v, f, _ = core.mesh_parts((torch.from_numpy(TET_V), TET_F.tolist()))          # handed on as they are
    assert torch.is_tensor(v) and isinstance(f, list)


def test_host_mesh_returns_contiguous_arrays_and_keeps_or_widens_the_normals():
    n32 = np.arange(12, dtype=np.float32).reshape(4, 3)
    v, f, n = core.host_mesh(TET_V.astype(np.float32)[:, ::-1], TET_F.astype(np.int32).T.copy().T, n32)
    assert v.dtype == np.float64 and f.dtype == np.int64 and v.flags.c_contiguous and f.flags.c_contiguous
    assert np.array_equal(v, TET_V[:, ::-1]) and np.array_equal(f, TET_F)
    assert n.dtype == np.float32 and n.tobytes() == n32.tobytes()                                 # bits untouched
    wide = core.host_mesh(TET_V, TET_F, n32, widen_normals=True)[2]
    assert wide.dtype == np.float64 and np.array_equal(wide, n32)
    assert core.host_mesh(TET_V, TET_F)[2] is None


def test_host_mesh_accepts_no_faces_and_no_vertices():
    v, f, _ = core.host_mesh(TET_V, np.zeros((0, 3), dtype=np.int64))
    assert v.shape == (4, 3) and f.shape == (0, 3) and f.dtype == np.int64
    n_v, f, _ = core.host_mesh(None, [], n_vertices=0)
    assert n_v == 0 and f.shape == (0, 3)
    n_v, f, _ = core.host_mesh(None, TET_F, n_vertices=4)
    assert n_v == 4 and np.array_equal(f, TET_F)
    with pytest.raises(ValueError, match=r'^mesh: -1 vertices'):
        core.host_mesh(None, [], n_vertices=-1)
    with pytest.raises(ValueError, match='refers to vertex 0 of 0'):
        core.host_mesh(None, [[0, 0, 0]], n_vertices=0)


@pytest.mark.parametrize('prefix', ['mesh', 'atlas'])
def test_host_mesh_errors_carry_the_prefix(prefix):
    low, high = TET_F.copy(), TET_F.copy()
    low[2, 1], high[1, 2] = -1, 4
    with pytest.raises(ValueError, match=r'^%s: a face refers to vertex -1 of 4' % prefix):
        core.host_mesh(TET_V, low, prefix=prefix)
    with pytest.raises(ValueError, match=r'^%s: a face refers to vertex 4 of 4' % prefix):
        core.host_mesh(TET_V, high, prefix=prefix)
    with pytest.raises(ValueError, match=r'^%s: a face refers to vertex 4 of 4' % prefix):
        core.host_mesh(None, high, n_vertices=4, prefix=prefix)
    with pytest.raises(ValueError, match=r'^%s: 3 normals for 4 vertices' % prefix):
        core.host_mesh(TET_V, TET_F, np.zeros((3, 3)), prefix=prefix)
    for bad in (np.nan, np.inf):
        broken = TET_V.copy()
        broken[3, 1] = bad
        assert core.host_mesh(broken, TET_F, prefix=prefix)[0].tobytes() == broken.tobytes()      # not asked for: no error
        with pytest.raises(ValueError, match=r'^%s: a vertex coordinate is not finite' % prefix):
            core.host_mesh(broken, TET_F, prefix=prefix, finite=True)
        with pytest.raises(ValueError, match=r'^simplify: a vertex coordinate is not finite'):
            core.host_mesh(broken, TET_F, prefix=prefix, finite='simplify')


def test_every_caller_keeps_its_prefix_and_raises_value_error():
    high = TET_F.copy()
    high[0, 0] = 7
    broken = TET_V.copy()
    broken[0, 0] = np.nan
    atlas = meshbake.Atlas(16, 4)
    calls = {'mesh: a face refers to vertex 7 of 4': [lambda: meshclean.host_clean(TET_V, high),
                                                      lambda: meshclean.host_components(high, 4),
                                                      lambda: meshclean.clean_mesh((TET_V, high)),
                                                      lambda: meshdist.host_face_areas(TET_V, high),
                                                      lambda: meshdist._HostMesh(TET_V, high),
                                                      lambda: meshsimplify.host_simplify(TET_V, high, resolution=2)],
             'mesh: 3 normals for 4 vertices': [lambda: meshclean.host_clean(TET_V, TET_F, np.zeros((3, 3)))],
             'simplify: a vertex coordinate is not finite': [lambda: meshsimplify.host_simplify(broken, TET_F, resolution=2),
                                                             lambda: meshsimplify.simplify_mesh((broken, high), resolution=2)],
             'atlas: a face refers to vertex 7 of 4': [lambda: meshbake.host_atlas_points(atlas, TET_V, high)],
             'atlas: 3 normals for 4 vertices': [lambda: meshbake.host_atlas_points(atlas, TET_V, TET_F, np.zeros((3, 3)))]}
    for message, fns in calls.items():
        for fn in fns:
            with pytest.raises(ValueError) as info:
                fn()
            assert str(info.value).startswith(message)
    assert np.isnan(meshclean.host_clean(broken, TET_F)[0]).any()                 # only the simplification refuses such a vertex


def test_on_device_and_to_numpy():
    t = torch.from_numpy(TET_V)
    assert not core.on_device(TET_V) and not core.on_device(t) and not core.on_device(t, 'cpu')
    assert core.on_device(TET_V, 'cuda') and core.on_device(t, torch.device('cuda:0'))
    assert core.to_numpy(TET_V) is TET_V and core.to_numpy(None) is None
    back = core.to_numpy(t.clone().requires_grad_(True))
    assert isinstance(back, np.ndarray) and np.array_equal(back, TET_V)


def test_face_cross_and_areas_are_the_same_bytes_on_arrays_and_cpu_tensors():
    g = np.random.RandomState(0)
    v = np.concatenate([g.standard_normal((40, 3)) * np.array([1e-3, 1.0, 1e3]), [[0.25, 0.5, 0.75]] * 2])
    f = np.concatenate([g.randint(0, 40, (60, 3)), [[3, 3, 9], [40, 41, 5], [7, 8, 7]]]).astype(np.int64)    # the last three: zero area
    want = core.face_areas(v, f)
    assert want.dtype == np.float64 and want.shape == (63,) and (want[-3:] == 0.0).all() and (want[:-3] > 0.0).sum() > 50
    got = core.face_areas(torch.from_numpy(v), torch.from_numpy(f))
    assert torch.is_tensor(got) and got.dtype == torch.float64 and got.numpy().tobytes() == want.tobytes()
    for a, b in zip(core.face_cross(v, f), core.face_cross(torch.from_numpy(v), torch.from_numpy(f))):
        assert b.numpy().tobytes() == a.tobytes()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    np.testing.assert_allclose(np.stack(core.face_cross(v, f), 1), np.cross(b - a, c - a), rtol=1e-12, atol=0)
    assert core.face_areas(TET_V, TET_F).tolist() == [0.5, 0.5, 0.5, 0.5 * 3.0 ** 0.5]
    assert meshdist.host_face_areas(v, f).tobytes() == want.tobytes()


@pytest.mark.parametrize('with_n', [False, True])
@pytest.mark.parametrize('ext', ['.obj', '.ply'])
def test_export_and_load_round_trip(tmp_path, ext, with_n):
    g = np.random.RandomState(1)
    v = g.standard_normal((30, 3)) / 3.0
    f = g.randint(0, 30, (50, 3)).astype(np.int64)
    normals = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    mesh = core.Mesh(v, f, vertex_normals=normals if with_n else None)
    back = core.load_mesh(mesh.export(str(tmp_path / ('m' + ext))))
    assert isinstance(back, core.Mesh) and back.vertices.dtype == np.float64 and back.faces.dtype == np.int64
    assert np.array_equal(back.faces, f) and (back.vertex_normals is not None) == with_n
    if ext == '.obj':
        assert np.array_equal(back.vertices, v)                                     # %.17g: bit-equal
    else:
        assert np.array_equal(back.vertices.astype(np.float32), v.astype(np.float32))
    if with_n:
        assert np.array_equal(back.vertex_normals.astype(np.float32), normals)
    with pytest.raises(NotImplementedError):
        mesh.export(str(tmp_path / 'm.stl'))
    with pytest.raises(ValueError, match='m.stl'):
        core.load_mesh(str(tmp_path / 'm.stl'))


def test_the_old_import_paths_name_the_same_objects():
    import psnerf_amd.stage1 as s1
    from psnerf_amd.stage1 import extracting
    assert extracting.Mesh is core.Mesh and s1.Mesh is core.Mesh and meshdist.load_mesh is core.load_mesh
