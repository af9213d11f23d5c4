"""Mesh extraction on the GPU (csrc/mesh.hip through psnerf_amd/stage1/extracting.py): the kernels alone against the numpy host
path, the look-up field of tests/mesh_fields.py through the whole device pipeline against the reference's recorded results, a
sphere-initialised network under ops.strict() against the CPU oracle and against the host path run on the device's own values,
the shipped extraction size (resolution 64, 3 upsampling steps: a 513^3 grid), and the edge cases of tests/mesh_cases.py kernel
by kernel: the refinement in lock step with the host path round by round, psn_mise_collect alone (capacities below the count,
sentinel-filled lists), the hole filling on constructed lines, psn_mc_count's codes and run sums and the meshes at ties,
non-finite values and thresholds that are no float32 value, and Extractor3D at resolutions that are no powers of two."""
import hashlib
import json
import os
import time

import numpy as np
import pytest
import torch

from tests.helpers import ATOL_LOGIT, ATOL_NORMAL, GOLDEN, assert_close, stage1_cfg
from tests import mesh_cases as mc
from tests import mesh_fields as mf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _holes(n, seed):
    g = np.random.RandomState(seed)
    grid = g.randn(n, n, n).astype(np.float32)
    grid[g.rand(n, n, n) < 0.7] = np.nan
    grid[:, n // 2, :] = np.nan           # lines along x and z that are all holes (they are filled by the y pass, if at all)
    grid[0, :, 0] = np.nan                # holes at index 0 of the x and z lines, and a y line that is all holes
    grid[0, 0, :] = np.nan                # a z line of holes that no pass can fill
    grid[n - 1, n - 1, n - 1] = 1.5
    return grid


@pytest.mark.parametrize('n', [3, 17, 65, 21])
def test_grid_ffill_is_bit_exact(n):
    from psnerf_amd import hip
    from psnerf_amd.stage1.extracting import host_ffill
    grid = _holes(n, n)
    ref = host_ffill(grid.copy())
    out = hip.grid_ffill(torch.from_numpy(grid).to(DEV)).cpu().numpy()
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    assert out.view(np.int32).tobytes() == ref.view(np.int32).tobytes()


@pytest.mark.parametrize('n', [3, 17, 65, 21])
def test_marching_cubes_kernels_against_the_host_path(n):
    from psnerf_amd import hip
    from psnerf_amd.stage1.extracting import CORNERS, host_marching_cubes, to_world
    grid = mf.checker(n - 1, seed=n)
    v_ref, f_ref = host_marching_cubes(grid, 0.0)
    dgrid = torch.from_numpy(grid).to(DEV)
    v, f = hip.marching_cubes(dgrid, 0.0)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    if n >= 17:   # every one of the 256 cases occurs
        P = np.pad(grid.astype(np.float64), 1, 'constant', constant_values=-1e6) <= 0.0
        M = n + 1
        cube = sum(P[dx:dx + M, dy:dy + M, dz:dz + M].astype(np.int64) << c for c, (dx, dy, dz) in enumerate(CORNERS))
        assert len(np.unique(cube)) == 256
    assert f.dtype == np.int64 and v.dtype == np.float64 and np.array_equal(f, f_ref) and v.shape == v_ref.shape
    err = np.abs(v - v_ref).max()
    print('n=%d: %d vertices, %d faces, max vertex difference %.3e lattice units, bit-equal: %s' % (n, len(v), len(f), err, np.array_equal(v, v_ref)))
    assert err <= 1e-12
    vw, fw = hip.marching_cubes(dgrid, 0.0, 2.4)
    errw = np.abs(vw.cpu().numpy() - to_world(v_ref, n, 2.4)).max()
    print('n=%d: world units: max difference %.3e, bit-equal: %s' % (n, errw, errw == 0.0))
    assert errw <= 1e-12 * 2.4 / (n - 1) and np.array_equal(fw.cpu().numpy(), f_ref)


def _to_lattice(vertices, n, box=2.4):
    return (np.asarray(vertices) / box + 0.5) * (n - 1) + 1.0


def _device_lookup(R, res0, depth):
    from psnerf_amd.stage1.extracting import Extractor3D
    model = mf.LookupModel(mf.sphere_rod_torus(R))
    ex = Extractor3D(model, device=DEV, resolution0=res0, upsampling_steps=depth, points_batch_size=3000)
    mesh, stats = ex.generate_mesh()
    return ex, model, mesh, stats


def test_lookup_field_through_the_device_pipeline_r32():
    g = np.load(os.path.join(GOLDEN, 'mesh_mise_r32.npz'))
    ex, model, mesh, stats = _device_lookup(32, 8, 2)
    known = np.zeros((33, 33, 33), dtype=bool)
    known[g['known'][:, 0], g['known'][:, 1], g['known'][:, 2]] = True
    seen = model.seen.cpu().numpy()
    assert np.array_equal(seen > 0, known) and seen.max() == 1 and np.array_equal(ex.last_known.cpu().numpy(), known)
    assert stats['n_points_evaluated'] == model.n_points == int(known.sum())
    assert ex.last_grid.cpu().numpy().tobytes() == g['dense'].tobytes()
    mf.assert_same_surface(_to_lattice(mesh.vertices, 33), mesh.faces, g['vertices'], g['faces'].astype(np.int64), 'device R=32')
    print('device R=32: rounds %d, points %d' % (stats['n_rounds'], stats['n_points_evaluated']))


def test_lookup_field_through_the_device_pipeline_r64():
    d = json.load(open(os.path.join(GOLDEN, 'mesh_mise_r64.json')))
    ex, model, mesh, stats = _device_lookup(64, 16, 2)
    assert stats['n_points_evaluated'] == model.n_points == d['n_known'] and int(model.seen.max()) == 1
    assert hashlib.sha256(np.ascontiguousarray(ex.last_grid.cpu().numpy().astype('<f4')).tobytes()).hexdigest() == d['dense_sha256']
    lat = _to_lattice(mesh.vertices, 65)
    assert (len(mesh.vertices), len(mesh.faces)) == (d['n_vertices'], d['n_faces'])
    assert mf.edges_digest(lat) == d['edges_sha256'] and mf.is_closed_oriented(mesh.faces)
    area, vol = mf.area_volume(lat, mesh.faces)
    assert vol * d['signed_volume'] > 0 and abs(vol - d['signed_volume']) < d['n_faces'] and abs(area - d['area']) < d['n_faces']


@pytest.mark.parametrize('case', ['below', 'above', 'clip', 'no_upsampling'])
def test_device_pipeline_equals_the_host_path_on_the_edge_cases(case):
    """An all-below field (empty mesh), an all-above field (the closed box the padding produces), clip=True and
    upsampling_steps=0: the device pipeline returns what the host path returns."""
    from psnerf_amd.stage1.extracting import Extractor3D
    field = {'below': np.full((33, 33, 33), -1.0, dtype=np.float32), 'above': np.full((33, 33, 33), 1.0, dtype=np.float32),
             'clip': mf.sphere_rod_torus(32) + np.float32(6.0), 'no_upsampling': mf.sphere_rod_torus(32)}[case]
    kw = dict(resolution0=33, upsampling_steps=0) if case == 'no_upsampling' else dict(resolution0=8, upsampling_steps=2)
    hm, dm = mf.LookupModel(field), mf.LookupModel(field)
    host, hstats = Extractor3D(hm, **kw).generate_mesh(clip=case == 'clip')
    ex = Extractor3D(dm, device=DEV, **kw)
    mesh, stats = ex.generate_mesh(clip=case == 'clip')
    assert np.array_equal(mesh.faces, host.faces) and mesh.vertices.shape == host.vertices.shape
    assert np.abs(mesh.vertices - host.vertices).max() <= 1e-12 * 2.4 / 32 if len(host.vertices) else True
    assert stats['n_points_evaluated'] == hstats['n_points_evaluated'] == dm.n_points and stats['n_rounds'] == hstats['n_rounds']
    assert mesh.is_empty == (case == 'below') and mf.is_closed_oriented(mesh.faces)
    if case == 'clip':
        assert bool((ex.last_grid[:, :, :3] == -30.0).all())


def _networks(seed=0):
    import psnerf_amd.stage1 as s1
    from oracle import stage1 as o1
    cfg = stage1_cfg('bear')
    torch.manual_seed(seed)
    onet = o1.NeuralNetwork(cfg)
    net = s1.NeuralNetwork(cfg)
    net.load_state_dict(onet.state_dict())
    return net.to(DEV), onet


def _n_components(n_vertices, faces):
    """Connected components of the vertex graph of a mesh (label propagation)."""
    label = np.arange(n_vertices)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], axis=0)
    while True:
        m = np.minimum(label[e[:, 0]], label[e[:, 1]])
        new = label.copy()
        np.minimum.at(new, e[:, 0], m)
        np.minimum.at(new, e[:, 1], m)
        if np.array_equal(new, label):
            return len(np.unique(label))
        label = new


def test_network_extraction_strict_against_oracle_and_host_path():
    from psnerf_amd import ops
    from psnerf_amd.stage1.extracting import Extractor3D, grid_points_host
    net, onet = _networks()
    ops.reset_hits()
    with ops.strict():
        ex = Extractor3D(net, device=DEV, resolution0=16, upsampling_steps=2, with_normals=True)
        mesh, stats = ex.generate_mesh()
        grid, known = ex.last_grid.cpu().numpy(), ex.last_known.cpu().numpy()
        mesh2, stats2 = Extractor3D(net, device=DEV, resolution0=16, upsampling_steps=2, with_normals=True).generate_mesh()
        # upsampling_steps = 0 (extracting.py:90-96): the points are formed on the host and uploaded; still the lean engine
        flat, fstats = Extractor3D(net, device=DEV, resolution0=33, upsampling_steps=0).generate_mesh()
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    assert fstats['n_points_evaluated'] == 33 ** 3 and len(flat.faces) > 500 and mf.is_closed_oriented(flat.faces)
    print('network R=64: %s; %d vertices, %d faces' % (stats, len(mesh.vertices), len(mesh.faces)))
    assert stats['n_points_evaluated'] == int(known.sum()) and len(mesh.faces) > 1000
    # two runs are bit-identical
    assert np.array_equal(mesh.vertices, mesh2.vertices) and np.array_equal(mesh.faces, mesh2.faces)
    assert np.array_equal(mesh.vertex_normals, mesh2.vertex_normals) and stats2['n_rounds'] == stats['n_rounds']
    # the values of the evaluated points against the oracle on the host
    idx = np.argwhere(known)
    p = grid_points_host(idx, 64, 2.4)
    with torch.no_grad():
        ref = onet(p.unsqueeze(0), None, return_logits=True).reshape(-1)
    assert_close(torch.from_numpy(grid[known]), ref, 1e-4, 'mesh extraction: -logit of the evaluated points', atol=ATOL_LOGIT)
    # the host path on the device's own values: same evaluated set, identical mesh
    host_model = mf.LookupModel(grid)
    hmesh, hstats = Extractor3D(host_model, resolution0=16, upsampling_steps=2).generate_mesh()
    assert np.array_equal(host_model.seen.numpy() > 0, known) and hstats['n_points_evaluated'] == stats['n_points_evaluated']
    assert hstats['n_rounds'] == stats['n_rounds']
    assert np.array_equal(hmesh.faces, mesh.faces)
    err = np.abs(hmesh.vertices - mesh.vertices).max() if len(mesh.vertices) else 0.0
    print('device mesh vs host path on the same values: max vertex difference %.3e (world units), bit-equal: %s' % (err, err == 0.0))
    assert err <= 1e-12 * 2.4 / 64
    assert mf.is_closed_oriented(mesh.faces)
    # normals: -gradient / |gradient| of the oracle at the (float32) vertices
    pv = torch.as_tensor(mesh.vertices, dtype=torch.float32)
    g = onet.gradient(pv.unsqueeze(0), tflag=False).reshape(-1, 3)
    nref = -g / torch.norm(g, dim=-1, keepdim=True)
    assert_close(torch.from_numpy(mesh.vertex_normals), nref, 1e-4, 'mesh extraction: vertex normals', atol=ATOL_NORMAL)


def test_shipped_extraction_size_513():
    """resolution 64, upsampling_steps 3 (every shipped config): closed, consistently oriented; F = 2 V - 4 if the surface is one
    component of genus 0 (a sphere-initialised network: asserted only when the host path at a smaller size finds one component);
    inside the test's own time limit."""
    from psnerf_amd import ops
    from psnerf_amd.stage1.extracting import Extractor3D
    net, _ = _networks()
    with ops.strict():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.time()
        ex = Extractor3D(net, device=DEV, resolution0=64, upsampling_steps=3)
        mesh, stats = ex.generate_mesh()
        dt = time.time() - t0
    peak = torch.cuda.max_memory_allocated() / 2.0 ** 20
    print('513^3: %.2f s, %s, %d vertices, %d faces, peak device memory %.0f MiB' % (dt, stats, len(mesh.vertices), len(mesh.faces), peak))
    assert dt < 120.0
    assert ex.last_grid.shape == (513, 513, 513) and stats['n_points_evaluated'] < 0.2 * 513 ** 3
    assert len(mesh.faces) > 100000 and mf.is_closed_oriented(mesh.faces)
    assert int(mesh.faces.max()) == len(mesh.vertices) - 1 and len(np.unique(mesh.faces)) == len(mesh.vertices)
    # Euler characteristic: the host path on the small grid's values says how many components the surface has
    from psnerf_amd.stage1.extracting import host_marching_cubes
    sgrid = Extractor3D(net, device=DEV, resolution0=16, upsampling_steps=2)
    sgrid.generate_mesh()
    hv, hf = host_marching_cubes(sgrid.last_grid.cpu().numpy(), 0.0)
    n_comp = _n_components(len(hv), hf)
    print('host path at 65^3: %d component(s), V = %d, F = %d' % (n_comp, len(hv), len(hf)))
    if n_comp == 1 and len(hf) == 2 * len(hv) - 4:
        assert len(mesh.faces) == 2 * len(mesh.vertices) - 4
    else:
        assert (len(mesh.faces) - 2 * len(mesh.vertices)) % 4 == 0   # F = 2 V - 4 (components - handles)


# ------------------------------------------------------------------------------------------------ the edge cases, kernel by kernel
def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _mise_state(res0, depth):
    """(grid, flags, vox, counts) as Extractor3D._mise_device sets them up."""
    from psnerf_amd import hip
    res = res0 << depth
    n = res + 1
    grid = torch.full((n * n * n,), float('nan'), dtype=torch.float32, device=DEV)
    flags = hip.mise_flags(res, DEV)
    s = 1 << depth
    flags[:n * n * n].view(n, n, n)[::s, ::s, ::s] = 1
    vox = torch.zeros(sum((res0 << l) ** 3 for l in range(depth)), dtype=torch.uint8, device=DEV)
    vox[:res0 ** 3] = 1
    return grid, flags, vox, torch.zeros(2, dtype=torch.int64, device=DEV)


def _assert_collected(rows, points, expect_rows, res, box_size, what):
    """rows (any order) are exactly expect_rows (sorted), points are grid_points_host of their rows, bit for bit."""
    from psnerf_amd.stage1.extracting import grid_points_host
    n = res + 1
    assert np.array_equal(np.sort(rows), expect_rows), what
    idx = np.stack(np.unravel_index(rows, (n, n, n)), axis=1)
    ref = grid_points_host(idx, res, box_size).numpy()
    assert ref.dtype == np.float32 and np.array_equal(_bits(points), _bits(ref)), what


@pytest.mark.parametrize('case', mc.mise_cases(), ids=lambda c: c[0])
def test_mise_kernels_in_lock_step_with_the_host_path(case):
    """psn_mise_collect -> scatter the field's values -> psn_mise_refine, side by side with tests/mesh_cases.lock_step: after every
    collect the count, the set of rows, the points (bit-equal, box sizes 2.4 and 2.0) and the flag bytes; after every refine the
    flag bytes, every voxel level and the pending count."""
    from psnerf_amd import hip
    cid, res0, depth, fname, tname = case
    thr = mc.THRESHOLDS[tname]
    res = res0 << depth
    n3 = (res + 1) ** 3
    values = mc.field(fname, res)
    rounds, _ = mc.lock_step(values, res0, depth, thr)
    dvalues = torch.from_numpy(values.copy()).to(DEV).view(-1)
    grid, flags, vox, counts = _mise_state(res0, depth)
    sizes = [(res0 << l) ** 3 for l in range(depth)]
    for r, h in enumerate(rounds):
        what = '%s round %d' % (cid, r)
        cap = len(h['rows'])
        flags2 = flags.clone()
        rows, points = hip.mise_collect(flags, res, 2.4, cap, counts[0:1])
        assert int(counts[0].item()) == cap, what
        _assert_collected(rows.cpu().numpy(), points.cpu().numpy(), h['rows'], res, 2.4, what)
        f = flags.cpu().numpy()
        assert np.array_equal(f[:n3], h['flags_collect'].ravel()) and not f[n3:].any(), what
        rows2, points2 = hip.mise_collect(flags2, res, 2.0, cap, counts[0:1])      # the other box size, on a copy of the flags
        assert int(counts[0].item()) == cap and torch.equal(flags2, flags), what
        _assert_collected(rows2.cpu().numpy(), points2.cpu().numpy(), h['rows'], res, 2.0, what)
        grid[rows] = dvalues[rows]
        hip.mise_refine(grid, flags, vox, res0, depth, thr, counts[1:2])
        f = flags.cpu().numpy()
        assert np.array_equal(f[:n3], h['flags_refine'].ravel()) and not f[n3:].any(), what
        for l, lv in enumerate(np.split(vox.cpu().numpy(), np.cumsum(sizes)[:-1])):
            assert np.array_equal(lv, h['vox'][l].ravel()), what + ' level %d' % l
        assert int(counts[1].item()) == h['new'], what
    assert rounds[-1]['new'] == 0
    print('%s: %d rounds, %d points' % (cid, len(rounds), sum(len(h['rows']) for h in rounds)))


def test_mise_refine_semantics_at_ties_and_unusual_values():
    """One voxel (resolution0 1, depth 1) whose eight corners are known, straight from the definition (active iff a known value
    >= thr and a known value <= thr): one tie alone activates; NaN never does; +-1e-40 against 0 are no ties; -0.0 is one."""
    from psnerf_amd import hip
    inf, nan, den = np.inf, np.nan, 1e-40
    cases = [([1.0] * 8, 0.0, False), ([1.0] * 7 + [0.0], 0.0, True), ([-1.0] * 7 + [0.0], 0.0, True), ([0.0] * 8, 0.0, True),
             ([-1.0] * 7 + [-0.375], -0.375, True), ([nan] * 7 + [0.0], 0.0, True), ([1.0] * 7 + [-0.0], 0.0, True), ([-0.375] + [1.0] * 7, -0.375, True),
             ([-0.375] + [1.0] * 7, float(np.nextafter(np.float32(-0.375), np.float32(-1))), False), ([nan] * 8, 0.0, False),
             ([nan] * 7 + [1.0], 0.0, False), ([nan] * 6 + [1.0, -1.0], 0.0, True), ([den] * 8, 0.0, False), ([-den] * 8, 0.0, False),
             ([den] * 7 + [-den], 0.0, True), ([den] * 7 + [0.0], 0.0, True), ([inf] * 8, 0.0, False), ([inf] * 7 + [-inf], 0.0, True),
             ([-inf] * 7 + [nan], 0.0, False), ([1.0] * 8, mc.THR_LOGIT_03, False), ([-1.0] * 7 + [-0.5], mc.THR_LOGIT_03, True)]
    for corners, thr, active in cases:
        grid, flags, vox, counts = _mise_state(1, 1)
        flags[:27].view(3, 3, 3)[::2, ::2, ::2] = 2
        grid.view(3, 3, 3)[::2, ::2, ::2] = torch.tensor(corners, dtype=torch.float32, device=DEV).view(2, 2, 2)
        hip.mise_refine(grid, flags, vox, 1, 1, thr, counts[1:2])
        what = '%s at %r' % (corners, thr)
        assert int(counts[1].item()) == (19 if active else 0) and int(vox[0].item()) == (2 if active else 1), what
        f = flags[:27].view(3, 3, 3).cpu().numpy()
        assert (f[::2, ::2, ::2] == 2).all() and int((f == 1).sum()) == (19 if active else 0) and not bool(flags[27:].any()), what


@pytest.mark.parametrize('res', [2, 3, 4, 6, 24])
def test_mise_collect_alone_with_every_capacity(res):
    """psn_mise_collect through the raw entry point on random flags from {0, 1, 2}, lists over-allocated and filled with a
    sentinel: capacity = count, 0 (null lists), 1 and count // 2; then flag bytes of value 1 in the padding behind the grid, which
    are no grid points."""
    from psnerf_amd import hip
    n = res + 1
    n3 = n ** 3
    assert n3 % 4 == {2: 3, 3: 0, 4: 1, 6: 3, 24: 1}[res]
    g = np.random.RandomState(res)
    start = np.zeros((n3 + 3) // 4 * 4, dtype=np.uint8)
    start[:n3] = g.randint(0, 3, size=n3)
    pending = np.nonzero(start[:n3] == 1)[0].astype(np.int64)
    count = len(pending)
    assert count >= 2 and (start[:n3] == 0).any() and (start[:n3] == 2).any()
    after = start.copy()
    after[:n3][start[:n3] == 1] = 2
    SENT_ROW, SENT_PT, EXTRA = -7, -777.0, 16
    variants = [(cap, False) for cap in (count, 0, 1, count // 2)] + ([(count, True)] if n3 % 4 else [])
    for cap, dirty_padding in variants:
        what = 'res %d capacity %d of %d%s' % (res, cap, count, ' (padding bytes set)' if dirty_padding else '')
        fl, expect = start.copy(), after.copy()
        if dirty_padding:
            fl[n3:] = 1
            expect[n3:] = 1
        flags = torch.from_numpy(fl).to(DEV)
        rows = torch.full((count + EXTRA,), SENT_ROW, dtype=torch.int64, device=DEV)
        points = torch.full((count + EXTRA, 3), SENT_PT, dtype=torch.float32, device=DEV)
        cnt = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        box = 2.4 if cap != 1 else 2.0
        rc = hip._lib.psn_mise_collect(flags.data_ptr(), res, box, cap, rows.data_ptr() if cap else None, points.data_ptr() if cap else None,
                                       cnt.data_ptr(), hip._stream())
        assert rc == 0, hip._lib.psn_last_error()
        torch.cuda.synchronize()
        assert int(cnt.item()) == count, what                                      # all pending points are reported ...
        assert np.array_equal(flags.cpu().numpy(), expect), what                   # ... and known now; 0, 2 and the padding untouched
        rows, points = rows.cpu().numpy(), points.cpu().numpy()
        kept = min(cap, count)
        assert (rows[kept:] == SENT_ROW).all() and (points[kept:] == np.float32(SENT_PT)).all(), what   # nothing behind capacity
        assert len(np.unique(rows[:kept])) == kept and np.isin(rows[:kept], pending).all(), what
        if kept == count:
            assert np.array_equal(np.sort(rows[:kept]), pending), what
        _assert_collected(rows[:kept], points[:kept], np.sort(rows[:kept]), res, box, what)


@pytest.mark.parametrize('n', mc.FFILL_SIZES)
def test_grid_ffill_on_constructed_lines(n):
    """n = 1, 2, 63, 64, 129, 130 on tests/mesh_cases.ffill_grid (z lines whose middle 64-point chunk is all holes, lines known only
    at z = 0, a first point that is a hole, x / y runs across the strided kernel's batches; -0.0, denormals and infinities among the
    values): bit for bit what host_ffill returns."""
    from psnerf_amd import hip
    from psnerf_amd.stage1.extracting import host_ffill
    grid = mc.ffill_grid(n)
    ref = host_ffill(grid.copy())
    out = hip.grid_ffill(torch.from_numpy(grid.copy()).to(DEV)).cpu().numpy()
    same = _bits(out) == _bits(ref)
    assert same.all(), 'n=%d: %d values differ, first at %s' % (n, (~same).sum(), np.argwhere(~same)[:4].tolist())


def _assert_vertices(v, v_ref, gate, what):
    """Same NaN rows; finite rows within the gate."""
    nan, nan_ref = np.isnan(v).any(axis=1), np.isnan(v_ref).any(axis=1)
    assert v.shape == v_ref.shape and np.array_equal(nan, nan_ref), what + ': NaN vertex rows differ'
    assert np.array_equal(np.isnan(v), np.isnan(v_ref)), what
    fin = ~nan
    assert np.isfinite(v[fin]).all() and np.isfinite(v_ref[fin]).all(), what
    err = float(np.abs(v[fin] - v_ref[fin]).max()) if fin.any() else 0.0
    print('%s: %d vertices (%d NaN rows), max difference %.3e, bit-equal: %s' % (what, len(v), int(nan.sum()), err,
                                                                                 np.array_equal(v[fin], v_ref[fin])))
    assert err <= gate, what


@pytest.mark.parametrize('case', mc.mc_cases(), ids=lambda c: c[0])
def test_marching_cubes_kernels_on_the_edge_cases(case):
    """psn_mc_count alone (codes and the sums per run of 256 cells, into sentinel-filled arrays) against the definition, then the
    mesh in lattice units and in world units (box 2.4; n - 1 = 6 and 11 are no powers of two) against host_marching_cubes."""
    from psnerf_amd import hip
    from psnerf_amd.stage1.extracting import host_marching_cubes, to_world
    cid, n, fname, tname = case
    thr = mc.THRESHOLDS[tname]
    grid = mc.field(fname, n - 1)
    dgrid = torch.from_numpy(grid.copy()).to(DEV)
    # the first pass alone
    code_ref, bv_ref, bt_ref = mc.mc_code(grid, thr)
    nb = int(hip._lib.psn_mc_blocks(n))
    assert nb == ((n + 1) ** 3 + 255) // 256 == len(bv_ref)
    code = torch.full(((n + 1) ** 3 + 64,), 0xee, dtype=torch.uint8, device=DEV)
    blk = torch.full((2, nb + 4), -9, dtype=torch.int32, device=DEV)
    rc = hip._lib.psn_mc_count(dgrid.data_ptr(), n, thr, code.data_ptr(), blk[0].data_ptr(), blk[1].data_ptr(), hip._stream())
    assert rc == 0, hip._lib.psn_last_error()
    torch.cuda.synchronize()
    code, blk = code.cpu().numpy(), blk.cpu().numpy()
    assert np.array_equal(code[:(n + 1) ** 3], code_ref) and (code[(n + 1) ** 3:] == 0xee).all(), cid
    assert np.array_equal(blk[0, :nb], bv_ref) and np.array_equal(blk[1, :nb], bt_ref) and (blk[:, nb:] == -9).all(), cid
    # both passes
    with np.errstate(invalid='ignore'):
        v_ref, f_ref = host_marching_cubes(grid, thr)
    assert len(v_ref) == int(bv_ref.sum()) and len(f_ref) == int(bt_ref.sum())
    v, f = hip.marching_cubes(dgrid, thr)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert f.dtype == np.int64 and v.dtype == np.float64 and np.array_equal(f, f_ref) and mf.is_closed_oriented(f), cid
    assert (len(f) == 0) == (fname == 'all_tie375')
    _assert_vertices(v, v_ref, 1e-12, cid + ' lattice units')
    vw, fw = hip.marching_cubes(dgrid, thr, 2.4)
    assert np.array_equal(fw.cpu().numpy(), f_ref), cid
    _assert_vertices(vw.cpu().numpy(), to_world(v_ref, n, 2.4), 1e-12 * 2.4 / (n - 1), cid + ' world units')


@pytest.mark.parametrize('threshold', [0.5, 0.3])
@pytest.mark.parametrize('res0,steps,fname', [(3, 2, 'sphere_rod_torus'), (5, 2, 'tie_checker'), (6, 1, 'ternary'), (1, 4, 'ternary')])
def test_extractor_on_the_device_equals_the_host_path_at_odd_resolutions(res0, steps, fname, threshold):
    """Extractor3D with a look-up model, device against host: resolutions 12, 20, 12 (depth 1) and 16 (resolution0 1), occupancy
    thresholds 0.5 (iso value 0, ties in the ternary field) and 0.3 (an iso value that is no float32 value), batches of 1000."""
    from psnerf_amd.stage1.extracting import Extractor3D
    res = res0 << steps
    values = mc.field(fname, res)
    hm, dm = mf.LookupModel(values.copy()), mf.LookupModel(values.copy())
    kw = dict(resolution0=res0, upsampling_steps=steps, threshold=threshold, points_batch_size=1000)
    hex_ = Extractor3D(hm, **kw)
    host, hstats = hex_.generate_mesh()
    ex = Extractor3D(dm, device=DEV, **kw)
    mesh, stats = ex.generate_mesh()
    what = '%dx%d %s threshold %g' % (res0, steps, fname, threshold)
    assert stats['n_rounds'] == hstats['n_rounds'] and stats['n_points_evaluated'] == hstats['n_points_evaluated'] == dm.n_points, what
    assert int(dm.seen.max()) == 1 and np.array_equal(ex.last_known.cpu().numpy(), hex_.last_known), what
    assert np.array_equal(_bits(ex.last_grid.cpu().numpy()), _bits(hex_.last_grid)), what
    assert np.array_equal(mesh.faces, host.faces) and len(host.faces) > 0 and mf.is_closed_oriented(mesh.faces), what
    _assert_vertices(mesh.vertices, host.vertices, 1e-12 * 2.4 / res, what)
    print('%s: rounds %d, points %d' % (what, stats['n_rounds'], stats['n_points_evaluated']))
