"""Mesh extraction without a GPU: the generated marching-cubes table, the numpy host path (psnerf_amd/stage1/extracting.py)
against results recorded from the reference's own libraries (tests/golden/mesh_*.{npz,json}, written by
tools/gen_golden_mesh.py), Extractor3D end to end on CPU tensors, and the argument checks of the new C entry points.

"Same surface" (tests/mesh_fields.assert_same_surface): equal sets of vertex-carrying lattice edges with vertices equal to 1e-9
lattice units; closed and consistently oriented; equal sets of directed face segments; equal triangle counts; area / signed
volume within (cells with triangles) x (cell face area / cell volume).  Triangle-for-triangle identity is NOT the contract: the
table is derived (tools/gen_mc_table.py), and may choose other interior diagonals inside a cell than the reference's."""
import ctypes
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, ROOT
from tests import mesh_fields as mf


def _gen():
    spec = importlib.util.spec_from_file_location('gen_mc_table', os.path.join(ROOT, 'tools', 'gen_mc_table.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# the cube, written out once more independently of the generator
CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
# faces: corners in cyclic order; edge i of a face joins corner i and corner i + 1
FACE_CORNERS = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5)]


def _edge_id(a, b):
    return [e for e in range(12) if set(EDGES[e]) == {a, b}][0]


FACE_EDGES = [tuple(_edge_id(f[i], f[(i + 1) % 4]) for i in range(4)) for f in FACE_CORNERS]


def _mid(e):
    return np.array([(CORNERS[EDGES[e][0]][k] + CORNERS[EDGES[e][1]][k]) / 2.0 for k in range(3)])


def _table():
    from psnerf_amd.stage1.extracting import mc_table
    ntri, tri = mc_table()
    return [[tuple(int(x) for x in tri[c, 3 * t:3 * t + 3]) for t in range(int(ntri[c]))] for c in range(256)]


def test_generator_reproduces_the_committed_header():
    gen = _gen()
    assert gen.render() == open(os.path.join(ROOT, 'psnerf_amd', 'csrc', 'mc_table.h')).read()


def test_table_properties_for_all_256_cases():
    tab = _table()
    assert tab[0] == [] and tab[255] == [] and tab[1] == [(0, 8, 3)]       # (v): case 1, normal (-, -, -)
    for case in range(256):
        tris = tab[case]
        bit = [(case >> c) & 1 for c in range(8)]
        active = set(e for e in range(12) if bit[EDGES[e][0]] != bit[EDGES[e][1]])
        assert set(e for t in tris for e in t) == active, case                                       # (i)
        directed = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
        assert len(set(directed)) == len(directed), case
        boundary = [d for d in directed if (d[1], d[0]) not in directed]
        interior = [d for d in directed if (d[1], d[0]) in directed]
        # (ii) the boundary is the face walk
        expect = set()
        for fc, fe in zip(FACE_CORNERS, FACE_EDGES):
            act = [i for i in range(4) if fe[i] in active]
            if len(act) == 2:
                expect.add(frozenset((fe[act[0]], fe[act[1]])))
            elif len(act) == 4:   # ambiguous face: every corner whose bit is set is cut off on its own
                for i in range(4):
                    if bit[fc[i]]:
                        expect.add(frozenset((fe[(i - 1) % 4], fe[i])))
        assert set(frozenset(d) for d in boundary) == expect and len(boundary) == len(expect), case
        # (iii) closed loops of 3..7 vertices, each triangulated as a disc
        nxt = dict(boundary)
        assert len(nxt) == len(boundary) and set(nxt.keys()) == set(nxt.values()) == active, case
        seen, lengths = set(), []
        for start in sorted(nxt):
            if start in seen:
                continue
            k, e = 0, start
            while e not in seen:
                seen.add(e)
                e = nxt[e]
                k += 1
            lengths.append(k)
        assert all(3 <= k <= 7 for k in lengths) and len(tris) == sum(k - 2 for k in lengths) and len(tris) <= 5, case
        # (iv) no interior diagonal inside a cube face
        for a, b in interior:
            assert not any(a in fe and b in fe for fe in FACE_EDGES), (case, a, b)
        # (v) the normal points towards the corners with the bit set.  The triangles of a loop form a consistently oriented disc
        # (checked above: no directed edge twice, every interior edge once in each direction), so the direction of the boundary
        # decides it: seen along the normal the surface lies to the left of a boundary segment a -> b, i.e. with m the inward
        # normal of the cube face the segment lies in and t the in-face direction from the segment to the set corner(s) it
        # cuts off, ((b - a) x m) . t > 0
        for a, b in boundary:
            for fc, fe in zip(FACE_CORNERS, FACE_EDGES):
                if a not in fe or b not in fe:
                    continue
                centre = np.mean([CORNERS[c] for c in fc], axis=0)
                m = (np.array([0.5, 0.5, 0.5]) - centre) * 2.0
                n_act = sum(1 for e in fe if e in active)
                cut = [c for c in fc if bit[c] and (n_act == 2 or (c in EDGES[a] and c in EDGES[b]))]
                assert cut, (case, a, b)
                t = np.mean([CORNERS[c] for c in cut], axis=0) - (_mid(a) + _mid(b)) / 2.0
                assert float(np.dot(np.cross(_mid(b) - _mid(a), m), t)) > 0, (case, a, b)


def test_table_against_the_reference_cases():
    """Per case, against what the reference's marching_cubes returned for one 2 x 2 x 2 volume: same edges, same directed face
    segments (hence the same winding), same triangle count."""
    g = np.load(os.path.join(GOLDEN, 'mesh_mc_cases.npz'))
    tab = _table()
    for case in range(256):
        rv = g['vertices'][g['v_off'][case]:g['v_off'][case + 1]]
        rf = g['faces'][g['f_off'][case]:g['f_off'][case + 1]].astype(np.int64)
        used = sorted(set(e for t in tab[case] for e in t))
        pos = dict((e, i) for i, e in enumerate(used))
        ov = np.array([_mid(e) for e in used]).reshape(-1, 3)
        of = np.array([[pos[e] for e in t] for t in tab[case]], dtype=np.int64).reshape(-1, 3)
        assert len(of) == len(rf), case
        if len(rf) == 0:
            assert len(rv) == 0
            continue
        re_, oe = mf.lattice_edges(rv), mf.lattice_edges(ov)
        assert set(map(tuple, re_.tolist())) == set(map(tuple, oe.tolist())), case
        assert mf.face_segments(rv, rf) == mf.face_segments(ov, of), case


# ------------------------------------------------------------------------------------------------ host path against the fixtures
def _run_host_mise(R, res0, depth):
    from psnerf_amd.stage1.extracting import Extractor3D
    model = mf.LookupModel(mf.sphere_rod_torus(R))
    ex = Extractor3D(model, resolution0=res0, upsampling_steps=depth, points_batch_size=3000)
    mesh, stats = ex.generate_mesh()
    return ex, model, mesh, stats


def _to_lattice(vertices, n, box=2.4):
    return (np.asarray(vertices) / box + 0.5) * (n - 1) + 1.0


def test_host_path_r32_against_the_reference_fixture():
    g = np.load(os.path.join(GOLDEN, 'mesh_mise_r32.npz'))
    ex, model, mesh, stats = _run_host_mise(32, 8, 2)
    seen = model.seen.numpy()
    known = np.zeros((33, 33, 33), dtype=bool)
    known[g['known'][:, 0], g['known'][:, 1], g['known'][:, 2]] = True
    assert np.array_equal(seen > 0, known)                                   # the known set is the reference's
    assert seen.max() == 1 and stats['n_points_evaluated'] == model.n_points == int(known.sum())   # no point twice
    assert ex.last_grid.dtype == np.float32 and ex.last_grid.tobytes() == g['dense'].tobytes()     # to_dense, bit for bit
    from psnerf_amd.stage1.extracting import host_marching_cubes
    v, f = host_marching_cubes(g['dense'], 0.0)
    mf.assert_same_surface(v, f, g['vertices'], g['faces'].astype(np.int64), 'host R=32')
    # Extractor3D's world-unit vertices are the fixture's through extracting.py:175-181
    mf.assert_same_surface(_to_lattice(mesh.vertices, 33), mesh.faces, g['vertices'], g['faces'].astype(np.int64), 'Extractor3D R=32')
    from psnerf_amd.stage1.extracting import to_world
    assert np.abs(mesh.vertices - to_world(v, 33, 2.4)).max() == 0.0
    assert set(stats) >= {'time (eval points)', 'time (marching cubes)', 'n_points_evaluated', 'n_rounds'}


def test_host_marching_cubes_on_a_random_grid_visits_every_case():
    g = np.load(os.path.join(GOLDEN, 'mesh_mise_r32.npz'))
    from psnerf_amd.stage1.extracting import host_marching_cubes
    v, f = host_marching_cubes(mf.checker(12), 0.0)
    mf.assert_same_surface(v, f, g['checker_vertices'], g['checker_faces'].astype(np.int64), 'random +- grid')


def test_host_path_r64_against_the_reference_digests():
    d = json.load(open(os.path.join(GOLDEN, 'mesh_mise_r64.json')))
    ex, model, mesh, stats = _run_host_mise(64, 16, 2)
    assert stats['n_points_evaluated'] == model.n_points == d['n_known'] and int(model.seen.max()) == 1
    assert hashlib.sha256(np.ascontiguousarray(ex.last_grid.astype('<f4')).tobytes()).hexdigest() == d['dense_sha256']
    lat = _to_lattice(mesh.vertices, 65)
    assert (len(mesh.vertices), len(mesh.faces)) == (d['n_vertices'], d['n_faces'])
    assert mf.edges_digest(lat) == d['edges_sha256']
    assert mf.is_closed_oriented(mesh.faces)
    area, vol = mf.area_volume(lat, mesh.faces)
    n_cells = d['n_faces']  # (an upper bound of the number of cells that carry triangles is enough for this loose check)
    assert vol * d['signed_volume'] > 0 and abs(vol - d['signed_volume']) < n_cells and abs(area - d['area']) < n_cells


# ------------------------------------------------------------------------------------------------ the edge cases (tests/mesh_cases.py)
def test_edge_cases_do_what_they_are_for():
    """Every case of tests/mesh_cases.py has the property it exists for (so that the device tests cannot pass on cases that
    degenerated): ties put vertices exactly on lattice points, ties alone drive a refinement, the non-finite field gives NaN vertex
    rows on a closed surface, and the marching-cubes sizes give the intended numbers of 256-cell runs."""
    from tests import mesh_cases as mc
    from psnerf_amd.stage1.extracting import host_marching_cubes, iso_value
    assert mc.THR_LOGIT_03 == iso_value(0.3) and mc.THR_LOGIT_03 != float(np.float32(mc.THR_LOGIT_03))
    assert [((n + 1) ** 3 + 255) // 256 for n in mc.MC_SIZES] == [1, 2, 9, 16] and (mc.MC_SIZES[-1] + 1) ** 3 % 256 == 0
    assert max(r << d for r, d in mc.MISE_PAIRS) == 48 and {r << d for r, d in mc.MISE_PAIRS} >= {12, 20, 48}
    for n in mc.MC_SIZES[1:]:
        v, f = host_marching_cubes(mc.field('ternary', n - 1), 0.0)
        on = int(mc.on_lattice_point(v).sum())
        print('ternary n=%d: %d of %d vertices exactly on lattice points' % (n, on, len(v)))
        assert on > len(v) // 4 and mf.is_closed_oriented(f)
        v, f = host_marching_cubes(mc.field('tie_checker', n - 1), mc.THR_TIE)
        assert int(mc.on_lattice_point(v).sum()) > 0 and mf.is_closed_oriented(f)
        v, f = host_marching_cubes(mc.field('tie_checker', n - 1), mc.THR_LOGIT_03)
        assert int(mc.on_lattice_point(v).sum()) == 0 and len(f) > 0
        v, f = host_marching_cubes(mc.field('nonfinite', n - 1), 0.0)
        nan_rows = int(np.isnan(v).any(axis=1).sum())
        print('nonfinite n=%d: %d NaN rows of %d vertices' % (n, nan_rows, len(v)))
        assert 0 < nan_rows < len(v) and mf.is_closed_oriented(f) and len(f) > 0
        fld = mc.field('nonfinite', n - 1)
        assert np.isnan(fld).any() and np.isposinf(fld).any() and np.isneginf(fld).any() and (np.signbit(fld) & (fld == 0)).any()
        assert (fld == np.float32(1e-40)).any() and (fld == np.float32(-1e-40)).any() and np.float32(1e-40) != 0
    for n in mc.MC_SIZES:
        assert len(host_marching_cubes(mc.field('all_tie375', n - 1), mc.THR_TIE)[1]) == 0
        v, f = host_marching_cubes(mc.field('all_above', n - 1), 0.0)
        assert len(f) == 2 * len(v) - 4 and mf.is_closed_oriented(f)
    # ties alone drive a refinement: sparse_tie(t) at thr = t evaluates more points than the same field with the ties set to +1
    for res0, depth in mc.MISE_PAIRS:
        if res0 < 2:
            continue
        R = res0 << depth
        for name, thr in (('sparse_tie0', mc.THR_ZERO), ('sparse_tie375', mc.THR_TIE)):
            fld = mc.field(name, R)
            assert (fld == np.float32(thr)).any() and set(np.unique(fld).tolist()) == {float(np.float32(thr)), 1.0}
            rounds, _ = mc.lock_step(fld, res0, depth, thr)
            plain, _ = mc.lock_step(np.ones_like(fld), res0, depth, thr)
            n_tie, n_plain = sum(len(r['rows']) for r in rounds), sum(len(r['rows']) for r in plain)
            assert n_plain == (res0 + 1) ** 3 and len(plain) == 1 and n_tie > n_plain and len(rounds) > 1, (res0, depth, name)
    # resolution0 = 1 is paired with fields that do refine there
    for cid, res0, depth, fname, tname in mc.mise_cases():
        if res0 == 1:
            rounds, _ = mc.lock_step(mc.field(fname, res0 << depth), res0, depth, mc.THRESHOLDS[tname])
            assert len(rounds) > depth and rounds[0]['new'] == 19, cid


def test_fill_cases_reach_the_paths_they_are_built_for():
    """tests/mesh_cases.ffill_grid: what the z kernel starts from (after the x and y passes) has the constructed lines, and the
    x / y runs are the holes the strided kernel meets."""
    from tests import mesh_cases as mc
    from psnerf_amd.stage1.extracting import host_ffill
    assert mc.FFILL_SIZES == [1, 2, 63, 64, 129, 130]
    for n in mc.FFILL_SIZES:
        grid = mc.ffill_grid(n)
        before_z = mc.ffill_before_z(grid)
        known = ~np.isnan(before_z)
        out = host_ffill(grid.copy())
        if n >= 2:
            assert not known[0, 0].any() and np.isnan(out[0, 0]).all()              # a first point that is a hole, never filled
            assert known[0, 1].tolist() == [True] + [False] * (n - 1)               # known only at z = 0 ...
            assert np.signbit(out[0, 1]).all() and (out[0, 1] == 0).all()           # ... and -0.0 travels down the whole line
        if n >= 7:
            assert np.nonzero(known[1, 0])[0].tolist() == [5] and np.isnan(out[1, 0, :5]).all() and np.isneginf(out[1, 0, 5:]).all()
        if n >= 129:
            for j, val in ((2, 1e-40), (3, -1e-40)):
                assert known[0, j, :64].all() and not known[0, j, 64:128].any() and known[0, j, 128:].all()
                assert (out[0, j, 63:128] == np.float32(val)).all() and np.float32(val) != 0
        if n >= 38:
            seen = set()
            for c, (q, length) in enumerate((q, length) for q in range(7, 11) for length in range(9, 18)):
                k = 1 + c
                for line in (grid[0, :, k], grid[:, n - 1, k]):                      # a y run and an x run
                    assert not np.isnan(line[q - 1]) and np.isnan(line[q:q + length]).all() and not np.isnan(line[q + length])
                assert out[0, q:q + length, k].view(np.int32).tolist() == [int(grid[0, q - 1, k].view(np.int32))] * length
                assert out[q:q + length, n - 1, k].view(np.int32).tolist() == [int(grid[q - 1, n - 1, k].view(np.int32))] * length
                seen.add((q, length))
            assert len(seen) == 36
            vals = grid[~np.isnan(grid)]
            assert (np.signbit(vals) & (vals == 0)).any() and np.isinf(vals).any() and ((vals != 0) & (np.abs(vals) < 1e-38)).any()


def test_lock_step_driver_is_the_extractor_on_the_host():
    """The round-by-round driver and Extractor3D's own host loop (query / update) evaluate the same points in the same rounds."""
    from tests import mesh_cases as mc
    from psnerf_amd.stage1.extracting import Extractor3D
    for res0, depth, fname, threshold in ((3, 2, 'tie_checker', 0.3), (2, 3, 'ternary', 0.5), (6, 1, 'nonfinite', 0.5)):
        fld = mc.field(fname, res0 << depth)
        model = mf.LookupModel(fld.copy())
        ex = Extractor3D(model, resolution0=res0, upsampling_steps=depth, threshold=threshold, points_batch_size=1000)
        _, stats = ex.generate_mesh()
        rounds, mise = mc.lock_step(fld, res0, depth, mc.THR_ZERO if threshold == 0.5 else mc.THR_LOGIT_03)
        assert stats['n_rounds'] == len(rounds) and stats['n_points_evaluated'] == sum(len(r['rows']) for r in rounds)
        assert np.array_equal(ex.last_known, mise.flags == 2) and int(model.seen.max()) == 1
        assert ex.last_grid.tobytes() == mise.to_dense().tobytes()


def _edge_golden():
    return json.load(open(os.path.join(GOLDEN, 'mesh_edge_cases.json')))


def _assert_mc_record(v, f, rec, what):
    """A host mesh (lattice units) against a record of the reference's: counts exactly, the lattice edges where they are
    defined, closed and oriented, area / signed volume within the gate of the R = 64 digests (triangles x unit cell: inside a
    cell the derived table may choose other diagonals than the reference's)."""
    from tests import mesh_cases as mc
    assert (len(v), len(f)) == (rec['n_vertices'], rec['n_faces']), what
    assert int(mc.on_lattice_point(v).sum()) == rec['n_on_lattice_points'], what
    assert mf.is_closed_oriented(f), what
    assert ('edges_sha256' in rec) == mc.edges_defined(v), what
    if 'edges_sha256' in rec:
        assert mf.edges_digest(v) == rec['edges_sha256'], what
    area, vol = mf.area_volume(v, f)
    gate = max(rec['n_faces'], 1)
    assert vol * rec['signed_volume'] > 0 or (vol == 0 and rec['signed_volume'] == 0), what
    assert abs(vol - rec['signed_volume']) < gate and abs(area - rec['area']) < gate, what


def test_host_path_reproduces_the_reference_on_the_edge_cases():
    """HostMISE round by round, to_dense and host_marching_cubes against what the reference's libmise / libmcubes recorded for
    every finite case (tests/golden/mesh_edge_cases.json, tools/gen_golden_mesh.py): ties, thresholds that are no float32 value,
    resolutions 2 .. 48 that are no powers of two, depth 1 and resolution0 1."""
    from tests import mesh_cases as mc
    from psnerf_amd.stage1.extracting import host_marching_cubes
    gold = _edge_golden()
    finite = [c for c in mc.mise_cases() if mc.is_finite_case(c[3])]
    assert sorted(gold['mise']) == sorted(c[0] for c in finite)
    for cid, res0, depth, fname, tname in finite:
        rec, thr = gold['mise'][cid], mc.THRESHOLDS[tname]
        rounds, mise = mc.lock_step(mc.field(fname, res0 << depth), res0, depth, thr)
        assert [len(r['rows']) for r in rounds] == rec['rounds'], cid
        assert mc.sha256(np.nonzero((mise.flags == 2).ravel())[0], '<i8') == rec['known_sha256'], cid
        dense = mise.to_dense()
        assert dense.dtype == np.float32 and mc.sha256(dense, '<f4') == rec['dense_sha256'], cid
        v, f = host_marching_cubes(dense, thr)
        _assert_mc_record(v, f, rec, cid)
    finite = [c for c in mc.mc_cases() if mc.is_finite_case(c[2])]
    assert sorted(gold['mc']) == sorted(c[0] for c in finite)
    for cid, n, fname, tname in finite:
        v, f = host_marching_cubes(mc.field(fname, n - 1), mc.THRESHOLDS[tname])
        _assert_mc_record(v, f, gold['mc'][cid], cid)


# ------------------------------------------------------------------------------------------------ Extractor3D on the CPU
def test_extractor_without_upsampling():
    from psnerf_amd.stage1.extracting import Extractor3D, host_marching_cubes, to_world
    field = mf.sphere_rod_torus(20)                       # 21 points per axis = resolution0
    model = mf.LookupModel(field)
    mesh, stats = Extractor3D(model, resolution0=21, upsampling_steps=0).generate_mesh()
    assert model.n_points == 21 ** 3 == stats['n_points_evaluated']
    v, f = host_marching_cubes(field, 0.0)
    assert np.array_equal(mesh.faces, f) and np.array_equal(mesh.vertices, to_world(v, 21, 2.4)) and len(f) > 100
    assert mf.is_closed_oriented(mesh.faces)


def test_extractor_clip():
    from psnerf_amd.stage1.extracting import Extractor3D, host_marching_cubes, to_world
    g = np.load(os.path.join(GOLDEN, 'mesh_mise_r32.npz'))
    field = mf.sphere_rod_torus(32) + np.float32(6.0)     # mostly above the iso value: the surface reaches below z = -1
    ex = Extractor3D(mf.LookupModel(field), resolution0=8, upsampling_steps=2)
    mesh, _ = ex.generate_mesh(clip=True)
    z = (2.4 * torch.linspace(-0.5, 0.5, 33)).numpy()
    assert (z < -1).sum() == 3
    assert (ex.last_grid[:, :, z < -1] == -30.0).all() and (ex.last_grid[:, :, z >= -1] != -30.0).all()
    v, f = host_marching_cubes(ex.last_grid, 0.0)
    assert np.array_equal(mesh.faces, f) and np.array_equal(mesh.vertices, to_world(v, 33, 2.4))
    assert mesh.vertices[:, 2].min() > 2.4 * (2.0 / 32 - 0.5) and mf.is_closed_oriented(mesh.faces)
    assert g['dense'].shape == ex.last_grid.shape


def test_extractor_empty_and_full_fields_and_export(tmp_path):
    from psnerf_amd.stage1.extracting import Extractor3D, Mesh
    below = np.full((33, 33, 33), -1.0, dtype=np.float32)
    model = mf.LookupModel(below)
    mesh, stats = Extractor3D(model, resolution0=8, upsampling_steps=2).generate_mesh()
    assert mesh.is_empty and mesh.faces.shape == (0, 3) and model.n_points == 9 ** 3 and stats['n_rounds'] == 1
    for ext in ('.obj', '.ply'):
        p = mesh.export(str(tmp_path / ('empty' + ext)))
        assert os.path.getsize(p) >= 0 and _read_mesh(p)[0].shape == (0, 3)
    # all above: the -1e6 padding closes the surface into the box of the grid (one component of genus 0)
    mesh, stats = Extractor3D(mf.LookupModel(-below), resolution0=8, upsampling_steps=2).generate_mesh()
    assert not mesh.is_empty and mf.is_closed_oriented(mesh.faces) and len(mesh.faces) == 2 * len(mesh.vertices) - 4
    cell = 2.4 / 32
    assert 1.2 < np.abs(mesh.vertices).max() < 1.2 + 1e-3 * cell
    assert stats['n_points_evaluated'] == 9 ** 3     # every value >= iso, none <= iso: no voxel is active
    # exports parse back
    ex = Extractor3D(mf.LookupModel(mf.sphere_rod_torus(32)), resolution0=8, upsampling_steps=2)
    mesh, _ = ex.generate_mesh()
    for ext in ('.obj', '.ply'):
        p = mesh.export(str(tmp_path / ('m' + ext)))
        v, f, _n = _read_mesh(p)
        assert np.array_equal(f, mesh.faces)
        if ext == '.obj':
            assert np.array_equal(v, mesh.vertices)
        else:
            assert np.array_equal(v, mesh.vertices.astype(np.float32))
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]]), (len(mesh.vertices), 1))
    for ext in ('.obj', '.ply'):
        p = Mesh(mesh.vertices, mesh.faces, nrm).export(str(tmp_path / ('n' + ext)))
        v, f, n = _read_mesh(p)
        assert np.array_equal(f, mesh.faces) and np.array_equal(n, nrm)
    with pytest.raises(NotImplementedError):
        mesh.export(str(tmp_path / 'm.stl'))


def _read_mesh(path):
    """Minimal readers for what Mesh.export writes -> (vertices, faces, normals or None)."""
    if path.endswith('.obj'):
        v, n, f = [], [], []
        for line in open(path):
            w = line.split()
            if not w:
                continue
            if w[0] == 'v':
                v.append([float(x) for x in w[1:4]])
            elif w[0] == 'vn':
                n.append([float(x) for x in w[1:4]])
            elif w[0] == 'f':
                f.append([int(x.split('/')[0]) - 1 for x in w[1:4]])
        return (np.array(v, dtype=np.float64).reshape(-1, 3), np.array(f, dtype=np.int64).reshape(-1, 3),
                np.array(n).reshape(-1, 3) if n else None)
    raw = open(path, 'rb').read()
    head, body = raw.split(b'end_header\n', 1)
    lines = head.decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    nv = int([l for l in lines if l.startswith('element vertex')][0].split()[2])
    nf = int([l for l in lines if l.startswith('element face')][0].split()[2])
    props = [l.split()[2] for l in lines if l.startswith('property float')]
    vert = np.frombuffer(body, dtype='<f4', count=nv * len(props)).reshape(nv, len(props))
    rec = np.frombuffer(body, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=nf, offset=4 * nv * len(props))
    assert len(body) == 4 * nv * len(props) + 13 * nf and (rec['n'] == 3).all()
    return vert[:, :3], rec['i'].astype(np.int64).reshape(-1, 3), (vert[:, 3:6].astype(np.float64) if len(props) == 6 else None)


def test_extractor_refuses_what_it_does_not_implement():
    from psnerf_amd.stage1.extracting import Extractor3D
    model = mf.LookupModel(mf.sphere_rod_torus(32))
    with pytest.raises(NotImplementedError, match='refinement_step'):
        Extractor3D(model, resolution0=8, upsampling_steps=2, refinement_step=1).generate_mesh()
    with pytest.raises(NotImplementedError, match='mask_loader'):
        Extractor3D(model, resolution0=8, upsampling_steps=2).generate_mesh(mask_loader=[{}])
    import psnerf_amd.stage1 as s1
    assert s1.Extractor3D is Extractor3D


# ------------------------------------------------------------------------------------------------ C entry points, no GPU needed
def test_mesh_entry_points_validate_their_arguments_without_a_gpu():
    from psnerf_amd import hip
    lib = hip._lib
    dummy = ctypes.c_void_p(64)
    odd = ctypes.c_void_p(66)
    big = hip.MESH_MAX_RESOLUTION + 1
    rc = lib.psn_mise_collect(None, 32, 2.4, 10, dummy, dummy, dummy, None)
    assert rc == -1 and b'null' in lib.psn_last_error()
    rc = lib.psn_mise_collect(dummy, 32, 2.4, 10, None, dummy, dummy, None)
    assert rc == -1 and b'null' in lib.psn_last_error()
    rc = lib.psn_mise_collect(dummy, 0, 2.4, 10, dummy, dummy, dummy, None)
    assert rc == -1 and b'resolution' in lib.psn_last_error()
    rc = lib.psn_mise_collect(dummy, big, 2.4, 10, dummy, dummy, dummy, None)
    assert rc == -3 and b'resolution' in lib.psn_last_error()
    rc = lib.psn_mise_collect(odd, 32, 2.4, 10, dummy, dummy, dummy, None)
    assert rc == -1 and b'aligned' in lib.psn_last_error()
    rc = lib.psn_mise_refine(None, dummy, dummy, 8, 2, 0.0, dummy, None)
    assert rc == -1 and b'null' in lib.psn_last_error()
    rc = lib.psn_mise_refine(dummy, dummy, dummy, 8, 0, 0.0, dummy, None)
    assert rc == -1 and b'depth' in lib.psn_last_error()
    rc = lib.psn_mise_refine(dummy, dummy, dummy, 1024, 1, 0.0, dummy, None)
    assert rc == -3 and b'resolution' in lib.psn_last_error()
    rc = lib.psn_mise_refine(dummy, odd, dummy, 8, 2, 0.0, dummy, None)
    assert rc == -1 and b'aligned' in lib.psn_last_error()
    rc = lib.psn_grid_ffill(None, 33, None)
    assert rc == -1 and b'null' in lib.psn_last_error()
    rc = lib.psn_grid_ffill(dummy, 0, None)
    assert rc == -1
    rc = lib.psn_grid_ffill(dummy, big + 1, None)
    assert rc == -3
    assert lib.psn_mc_blocks(33) == (34 ** 3 + 255) // 256 and lib.psn_mc_blocks(0) == 0 and lib.psn_mc_blocks(big + 1) == 0
    rc = lib.psn_mc_count(dummy, 33, 0.0, None, dummy, dummy, None)
    assert rc == -1 and b'null' in lib.psn_last_error()
    rc = lib.psn_mc_count(dummy, 1, 0.0, dummy, dummy, dummy, None)
    assert rc == -1 and b'n=1' in lib.psn_last_error()
    rc = lib.psn_mc_count(dummy, big + 1, 0.0, dummy, dummy, dummy, None)
    assert rc == -3
    rc = lib.psn_mc_emit(dummy, 33, 0.0, dummy, dummy, None, 3, 1, 2.4, dummy, dummy, dummy, None)
    assert rc == -1 and b'null' in lib.psn_last_error()
    rc = lib.psn_mc_emit(dummy, 33, 0.0, dummy, dummy, dummy, 3, 1, 2.4, dummy, None, dummy, None)
    assert rc == -1 and b'null output' in lib.psn_last_error()
    rc = lib.psn_mc_emit(dummy, 33, 0.0, dummy, dummy, dummy, -1, 1, 2.4, dummy, dummy, dummy, None)
    assert rc == -1 and b'n_vertices' in lib.psn_last_error()
    rc = lib.psn_mc_emit(dummy, 33, 0.0, dummy, dummy, dummy, 1 << 31, 1, 2.4, dummy, dummy, dummy, None)
    assert rc == -3 and b'32-bit' in lib.psn_last_error()
    rc = lib.psn_mc_emit(dummy, big + 1, 0.0, dummy, dummy, dummy, 3, 1, 2.4, dummy, dummy, dummy, None)
    assert rc == -3
    # the wrappers refuse host tensors like every other product path
    with pytest.raises(RuntimeError):
        hip.grid_ffill(torch.zeros(3, 3, 3))
    with pytest.raises(RuntimeError):
        hip.marching_cubes(torch.zeros(3, 3, 3), 0.0)


def test_extract_mesh_tool_on_the_host(tmp_path):
    """tools/extract_mesh.py with the reference script's arguments: config.yaml + models/model.pt in, mesh.<ext> out."""
    import yaml
    from oracle.stage1 import NeuralNetwork
    from psnerf_amd.checkpoints import CheckpointIO
    from psnerf_amd.synthetic import stage1_cfg
    spec = importlib.util.spec_from_file_location('extract_mesh_tool', os.path.join(ROOT, 'tools', 'extract_mesh.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cfg = stage1_cfg('bear')
    cfg['extraction'] = {'resolution': 8, 'upsampling_steps': 3, 'refinement_step': 0}
    exp = tmp_path / 'out' / 'bear' / 'test_1'
    os.makedirs(str(exp / 'models'))
    with open(str(exp / 'config.yaml'), 'w') as f:
        yaml.safe_dump(cfg, f)
    torch.manual_seed(0)
    CheckpointIO(str(exp / 'models'), model=NeuralNetwork(cfg)).save('model.pt')
    args = ['--no-cuda', '--obj_name', 'bear', '--exp_folder', str(tmp_path / 'out'), '--test_out_dir', str(tmp_path / 'test_out'),
            '--upsampling-steps', '1', '--mesh_extension', 'ply']
    path = tool.main(args)
    assert path == str(tmp_path / 'test_out' / 'bear' / 'test_1' / 'mesh.ply')
    v, f, _n = _read_mesh(path)
    assert len(f) == 2 * len(v) - 4 and len(f) > 200 and mf.is_closed_oriented(f)   # the sphere of the geometric initialisation
    with pytest.raises(NotImplementedError):
        tool.main(args + ['--refinement-step', '2'])
