#!/usr/bin/env python
"""Write the mesh-extraction fixtures under tests/golden/ from the REFERENCE's own native libraries.

Needs the reference checkout (argument or $PSNERF_REFERENCE), a C++ compiler and Cython.  The sources of its two libraries
(stage1/utils/libmise: multi-resolution iso-surface refinement; stage1/utils/libmcubes: marching cubes) are copied to a
temporary directory OUTSIDE this repository, built there, run on the fields of tests/mesh_fields.py, and only their RESULTS
are stored:
  mesh_mc_cases.npz   vertices / faces of marching_cubes for the 256 sign patterns of one 2 x 2 x 2 volume (values -+1)
  mesh_mise_r32.npz   resolution0 8, depth 2: known points, to_dense grid (float32), vertices (float64) and faces of the padded
                      marching cubes; plus the marching cubes of a random +- grid (mesh_fields.checker) that visits every
                      ambiguous-face configuration
  mesh_mise_r64.json  resolution0 16, depth 2: digests only
  mesh_edge_cases.json  the finite cases of tests/mesh_cases.py (ties, thresholds that are no float32 value, odd resolutions,
                      depth 1, resolution0 1): per refinement case the points per round, digests of the known set and of the dense
                      grid and the counts / area / signed volume of its marching cubes; per marching-cubes case the same counts;
                      the lattice-edge digest only where no vertex sits on a lattice point.  The non-finite field is left out: the
                      reference's behaviour there is not a contract

    python tools/gen_golden_mesh.py /path/to/reference [base] [edge]      (which files to write; default: all of them)
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

SETUP = '''
import numpy
from setuptools import setup, Extension
from Cython.Build import cythonize
defs = [('PyArray_DOUBLE', 'NPY_DOUBLE'), ('PyArray_ULONG', 'NPY_ULONG'), ('PyArray_LONG', 'NPY_LONG'), ('PyArray_INT', 'NPY_INT'),
        ('PyArray_FLOAT', 'NPY_FLOAT'), ('PyArray_UINT', 'NPY_UINT'), ('PyArray_BOOL', 'NPY_BOOL')]
args = ['-std=c++11', '-fpermissive', '-ffp-contract=off', '-w']
exts = [Extension('utils.libmise.mise', ['utils/libmise/mise.pyx'], language='c++', include_dirs=[numpy.get_include()], extra_compile_args=args),
        Extension('utils.libmcubes.mcubes', ['utils/libmcubes/mcubes.pyx', 'utils/libmcubes/pywrapper.cpp', 'utils/libmcubes/marchingcubes.cpp'],
                  language='c++', include_dirs=[numpy.get_include(), 'utils/libmcubes'], define_macros=defs, extra_compile_args=args)]
setup(name='ref_mesh', ext_modules=cythonize(exts, language_level=3), script_args=['build_ext', '--inplace'])
'''


def build_reference(ref):
    tmp = tempfile.mkdtemp(prefix='psnerf_ref_mesh_')
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    os.makedirs(os.path.join(tmp, 'utils'))
    open(os.path.join(tmp, 'utils', '__init__.py'), 'w').close()
    for lib in ('libmise', 'libmcubes'):
        src = os.path.join(ref, 'stage1', 'utils', lib)
        dst = os.path.join(tmp, 'utils', lib)
        os.makedirs(dst)
        for name in os.listdir(src):
            if name.endswith(('.pyx', '.cpp', '.h', '.py')) and name not in ('setup.py', 'mcubes.cpp', 'test.py'):
                shutil.copy(os.path.join(src, name), dst)
    with open(os.path.join(tmp, 'build_ref.py'), 'w') as f:
        f.write(SETUP)
    subprocess.check_call([sys.executable, 'build_ref.py'], cwd=tmp)
    sys.path.insert(0, tmp)
    return tmp


def reference_extract(field, resolution0, depth, thr=0.0):
    """extracting.py:98-119 + 170-178 with the reference's libraries and a look-up of ``field`` -> dict of results."""
    from utils.libmise import MISE
    from utils import libmcubes
    mise = MISE(resolution0, depth, thr)
    rounds, known = [], []
    points = mise.query()
    while points.shape[0] != 0:
        values = field[points[:, 0], points[:, 1], points[:, 2]].astype(np.float64)
        mise.update(points, values)
        rounds.append(int(points.shape[0]))
        known.append(points)
        points = mise.query()
    dense = mise.to_dense()
    assert np.array_equal(dense, dense.astype(np.float32).astype(np.float64))
    v, f = reference_mc(dense, thr)
    return dict(rounds=rounds, known=np.concatenate(known, 0), dense=dense.astype(np.float32), vertices=v, faces=f)


def reference_mc(grid, thr=0.0, pad=True):
    """libmcubes.marching_cubes on the padded grid, its +0.5 shift removed: vertices in units of the (padded) lattice."""
    from utils import libmcubes
    g = np.asarray(grid, dtype=np.float64)
    if pad:
        g = np.pad(g, 1, 'constant', constant_values=-1e6)
    v, f = libmcubes.marching_cubes(np.ascontiguousarray(g), thr)
    return v - 0.5, f.astype(np.int64)


def cube_histogram(grid, thr=0.0):
    from psnerf_amd.stage1.extracting import CORNERS
    P = np.pad(np.asarray(grid, dtype=np.float64), 1, 'constant', constant_values=-1e6)
    M = P.shape[0] - 1
    cube = np.zeros((M, M, M), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = CORNERS[c]
        cube |= (P[dx:dx + M, dy:dy + M, dz:dz + M] <= thr).astype(np.int64) << c
    return np.bincount(cube.ravel(), minlength=256)


def mc_record(vertices, faces):
    """Counts, area and signed volume of a reference mesh (lattice units); the lattice-edge digest where it is defined."""
    from tests import mesh_cases as mc, mesh_fields as mf
    area, volume = mf.area_volume(vertices, faces)
    rec = dict(n_vertices=int(len(vertices)), n_faces=int(len(faces)), area=area, signed_volume=volume,
               n_on_lattice_points=int(mc.on_lattice_point(vertices).sum()))
    if mc.edges_defined(vertices):   # (lattice_edges refuses a vertex on, or within 1e-9 of, a lattice point)
        rec['edges_sha256'] = mf.edges_digest(vertices)
    return rec


def edge_cases():
    """tests/golden/mesh_edge_cases.json from the reference's libraries on the finite cases of tests/mesh_cases.py."""
    from tests import mesh_cases as mc
    out = dict(mise={}, mc={})
    for cid, res0, depth, fname, tname in mc.mise_cases():
        if not mc.is_finite_case(fname):
            continue
        R = res0 << depth
        r = reference_extract(mc.field(fname, R), res0, depth, mc.THRESHOLDS[tname])
        rec = dict(rounds=r['rounds'], known_sha256=mc.sha256(np.sort(mc.linear(r['known'], R + 1)), '<i8'),
                   dense_sha256=mc.sha256(r['dense'], '<f4'))
        rec.update(mc_record(r['vertices'], r['faces']))
        out['mise'][cid] = rec
        print(cid, rec['rounds'], rec['n_vertices'], rec['n_faces'])
    for cid, n, fname, tname in mc.mc_cases():
        if not mc.is_finite_case(fname):
            continue
        v, f = reference_mc(mc.field(fname, n - 1), mc.THRESHOLDS[tname])
        out['mc'][cid] = mc_record(v, f)
        print(cid, out['mc'][cid]['n_vertices'], out['mc'][cid]['n_faces'], out['mc'][cid]['n_on_lattice_points'])
    with open(os.path.join(GOLDEN, 'mesh_edge_cases.json'), 'w') as f:   # one case per line: a few kB
        f.write('{\n')
        for gi, group in enumerate(('mise', 'mc')):
            f.write(' "%s": {\n' % group)
            keys = list(out[group])
            for i, k in enumerate(keys):
                f.write('  "%s": %s%s\n' % (k, json.dumps(out[group][k], sort_keys=True, separators=(',', ':')), ',' if i + 1 < len(keys) else ''))
            f.write(' }%s\n' % (',' if gi == 0 else ''))
        f.write('}\n')


def main():
    args = [a for a in sys.argv[1:] if a not in ('base', 'edge')]
    which = [a for a in sys.argv[1:] if a in ('base', 'edge')] or ['base', 'edge']
    ref = args[0] if args else os.environ.get('PSNERF_REFERENCE')
    assert ref and os.path.isdir(ref), 'usage: gen_golden_mesh.py /path/to/reference [base] [edge]'
    tmp = build_reference(ref)
    try:
        if 'edge' in which:
            edge_cases()
        if 'base' in which:
            base_fixtures()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def base_fixtures():
    if True:
        from tests import mesh_fields as mf
        from psnerf_amd.stage1.extracting import CORNERS
        # -- the 256 single-cell cases
        vs, fs, voff, foff = [], [], [0], [0]
        for case in range(256):
            vol = np.ones((2, 2, 2), dtype=np.float64)
            for m in range(8):
                if (case >> m) & 1:
                    vol[tuple(CORNERS[m])] = -1.0
            v, f = reference_mc(vol, 0.0, pad=False)
            vs.append(v.reshape(-1, 3)); fs.append(f.reshape(-1, 3))
            voff.append(voff[-1] + len(vs[-1])); foff.append(foff[-1] + len(fs[-1]))
        np.savez_compressed(os.path.join(GOLDEN, 'mesh_mc_cases.npz'), vertices=np.concatenate(vs, 0), faces=np.concatenate(fs, 0).astype(np.int32),
                            v_off=np.array(voff, dtype=np.int32), f_off=np.array(foff, dtype=np.int32))
        # -- R = 32, full
        r = reference_extract(mf.sphere_rod_torus(32), 8, 2)
        hist = cube_histogram(r['dense'])
        print('R=32: rounds', r['rounds'], 'known', len(r['known']), 'of', 33 ** 3, 'vertices', len(r['vertices']), 'faces', len(r['faces']))
        print('R=32: cube indices visited: %d of 256; missing %s' % ((hist > 0).sum(), np.nonzero(hist == 0)[0].tolist()))
        chk = mf.checker(12)
        cv, cf = reference_mc(chk)
        print('checker: cube indices visited: %d of 256' % (cube_histogram(chk) > 0).sum())
        np.savez_compressed(os.path.join(GOLDEN, 'mesh_mise_r32.npz'), known=r['known'].astype(np.int16), dense=r['dense'],
                            vertices=r['vertices'], faces=r['faces'].astype(np.int32), rounds=np.array(r['rounds'], dtype=np.int32),
                            checker_vertices=cv, checker_faces=cf.astype(np.int32))
        # -- R = 64, digests
        r = reference_extract(mf.sphere_rod_torus(64), 16, 2)
        area, volume = mf.area_volume(r['vertices'], r['faces'])
        dig = dict(resolution0=16, depth=2, rounds=r['rounds'], n_known=int(len(r['known'])),
                   dense_sha256=hashlib.sha256(np.ascontiguousarray(r['dense'].astype('<f4')).tobytes()).hexdigest(),
                   n_vertices=int(len(r['vertices'])), n_faces=int(len(r['faces'])), edges_sha256=mf.edges_digest(r['vertices']),
                   area=area, signed_volume=volume)
        print('R=64:', dig)
        with open(os.path.join(GOLDEN, 'mesh_mise_r64.json'), 'w') as f:
            json.dump(dig, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
