#!/usr/bin/env python3
"""The photographs of a dataset projected onto an exported mesh: the photo atlas, per-vertex colours and visibility, and (with the
photometric-stereo normal maps) fused per-vertex normals against the mesh's own (psnerf_amd/meshproject.py, meshbake.bake_views).

    python tools/project_views.py MESH DATASET_DIR [--light N | --light-avg] [--normals DIR] [--views V [V ...]] [--size 2048]
                                  [--out NAME] [--cos-min C] [--weight cosine|uniform] [--host]

DATASET_DIR is one object in the reference's layout: params.json ('K', 'pose_c2w' in OpenGL axes, 'n_view'), mask/view_XX.png and
img/view_XX/NNN.png, cameras and masks read the way VisualHull.from_params reads them.  --light N (default 1) takes light N of every
view; --light-avg the mean over a view's lights (photostereo.light_average).  A sample is taken only where all four pixels of its
footprint lie inside the view's mask.
Writes  NAME_photo.png, NAME_seen.png     the atlas (with NAME.obj / NAME.mtl that carry its texture coordinates)
        NAME_vertex_rgb.npy               float32 [V, 3], the weighted mean over the seeing views (0 where none sees the vertex)
        NAME_vertex_seen.npy              int32 [V], the number of views that see each vertex
  --normals DIR (the outnpy maps tools/photometric_stereo.py writes, view_XX.npy, camera frame):
        NAME_vertex_normal_ps.npy         float32 [V, 3], the maps taken to the world and fused per vertex
        NAME_vertex_normal_angle.npy      float32 [V], the angle in degrees to the mesh's own vertex normal (NaN where unseen)
and prints one JSON report: the share of the surface area seen, the mean spread and the mean angle.  NAME defaults to the mesh's
path without its extension.  --host runs the float64 numpy definition instead of the device kernel."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description='Project the views onto the mesh')
    ap.add_argument('mesh')
    ap.add_argument('dataset')
    which = ap.add_mutually_exclusive_group()
    which.add_argument('--light', type=int, default=1, help='the light of every view, from 1')
    which.add_argument('--light-avg', action='store_true', help='the mean over each view\'s lights')
    ap.add_argument('--normals', type=str, default=None, metavar='DIR')
    ap.add_argument('--views', type=int, nargs='+', default=None, help='view numbers from 1 (default: all)')
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--out', type=str, default=None, metavar='NAME')
    ap.add_argument('--cos-min', type=float, default=0.0)
    ap.add_argument('--weight', choices=('cosine', 'uniform'), default='cosine')
    ap.add_argument('--host', action='store_true', help='the numpy definition instead of the device kernel')
    args = ap.parse_args(argv)

    import numpy as np
    from psnerf_amd import meshbake, meshproject as mp, meshtopo, photostereo as ps
    from psnerf_amd.hull import cameras_from_params, masks_from_dir
    from psnerf_amd.imgmetrics import load_image
    from psnerf_amd.meshcore import face_areas, load_mesh, to_numpy

    K, poses, views, _ = cameras_from_params(os.path.join(args.dataset, 'params.json'), args.views, 'project_views')
    masks = masks_from_dir(os.path.join(args.dataset, 'mask'), views)
    images = []
    for i, vi in enumerate(views):
        folder = os.path.join(args.dataset, 'img', 'view_%02d' % vi)
        if args.light_avg:
            lights = np.stack([load_image(p)[..., :3] for p in sorted(glob.glob(os.path.join(folder, '[0-9][0-9][0-9].png')))])
            images.append(np.asarray(to_numpy(ps.light_average(lights, masks[i])[1])))
        else:
            images.append(load_image(os.path.join(folder, '%03d.png' % args.light))[..., :3])
    images = np.ascontiguousarray(np.stack(images))
    mesh = load_mesh(args.mesh)
    v, f = np.asarray(mesh.vertices, dtype=np.float64), np.asarray(mesh.faces, dtype=np.int64)
    device = None if args.host else 'cuda'
    options = dict(masks=masks.astype(np.uint8), cos_min=args.cos_min, weight=args.weight, device=device)
    name = args.out if args.out is not None else os.path.splitext(args.mesh)[0]
    os.makedirs(os.path.dirname(os.path.abspath(name)), exist_ok=True)

    baked = meshbake.bake_views((v, f), images, K, poses, size=args.size, **options)
    files = meshbake.export_textured(name, (v, f), baked)
    per_vertex = mp.vertex_views((v, f), images, K, poses, **options)
    np.save(name + '_vertex_rgb.npy', to_numpy(mp.mean(per_vertex)).astype(np.float32))
    np.save(name + '_vertex_seen.npy', to_numpy(per_vertex.n_seen))
    faces_seen = to_numpy(mp.face_visibility((v, f), K, poses, images.shape[1], images.shape[2], masks=options['masks'], cos_min=args.cos_min,
                                             device=device))
    area = face_areas(v, f)
    seen_texels = to_numpy(baked['seen'])[..., 0][baked['atlas'].owner()[0] >= 0] > 0
    spread = to_numpy(baked['spread'])[baked['atlas'].owner()[0] >= 0][seen_texels]
    report = {'n_views': len(views), 'n_vertices': int(v.shape[0]), 'n_faces': int(f.shape[0]), 'path': 'host' if args.host else 'device',
              'area_seen': float(area[faces_seen > 0].sum() / area.sum()), 'vertices_seen': float((to_numpy(per_vertex.n_seen) > 0).mean()),
              'texels_seen': float(seen_texels.mean()), 'mean_spread': float(spread.mean()) if spread.size else 0.0, 'mean_angle': None,
              'photo': files['photo'], 'seen': files['seen']}
    if args.normals is not None:
        maps = np.stack([np.load(os.path.join(args.normals, 'view_%02d.npy' % vi)).astype(np.float32) for vi in views])
        fused = mp.vertex_views((v, f), np.ascontiguousarray(maps), K, poses, frame='camera_normal', **options)
        ps_normal = to_numpy(mp.fused_normals(fused))
        own = to_numpy(meshtopo.vertex_normals((v, f)))
        has = (to_numpy(fused.n_seen) > 0) & (np.abs(ps_normal).sum(axis=1) > 0)
        angle = np.full(v.shape[0], np.nan, dtype=np.float32)
        angle[has] = np.rad2deg(np.arccos(np.clip((ps_normal[has] * own[has]).sum(axis=1), -1.0, 1.0)))
        np.save(name + '_vertex_normal_ps.npy', ps_normal.astype(np.float32))
        np.save(name + '_vertex_normal_angle.npy', angle)
        report['mean_angle'] = float(angle[has].mean()) if has.any() else None
    print(json.dumps(report))
    return report


if __name__ == '__main__':
    main()
