#!/usr/bin/env python
"""Render an exported mesh from the cameras of a dataset: per view the normal map, the depth map and the silhouette, and on request
binary shadow maps -- the maps of the ASSET (or of a ground-truth scan), to be compared with the dataset's own.

    python tools/render_mesh.py --mesh test_out/bear/test_1/mesh.ply --cameras data/bear/params.json --out mesh_maps
                                [--views 1 5 9] [--hw H W] [--vertex-normals] [--gt-normal data/bear/normal/npy]
                                [--gt-mask data/bear/norm_mask] [--lights FILE] [--textures] [--host]

--cameras is the dataset's params.json, read as stage1/dataloading/dataset.py and tools/evaluate.py read it: 'K' (intrinsics),
'pose_c2w' (camera to world per view, OpenGL axes: columns 1 and 2 are negated to get the OpenCV pose the renderer takes), 'imhw',
'n_view', and for the shadow maps 'light_direction' / 'light_is_same'.  Views are numbered from 1, as the files view_VV.* are.
Written per view under --out: normal/view_VV.npy (float32 [H, W, 3], world space, unit length, zeros off the mesh),
depth/view_VV.npy (float32 [H, W], distance from the camera), mask/view_VV.npy (bool) and, where PIL is present, the same as .png
(normals as imgmetrics.to_img((n + 1) / 2), depth scaled to its range over the mask).
--vertex-normals interpolates the mesh file's vertex normals instead of taking the geometric face normal.
--gt-normal DIR (view_VV.npy, as the dataset's normal/npy) prints the mean angular error per view and overall through
imgmetrics.evaluate_normals over the pixels where the render, the ground truth and, with --gt-mask DIR (view_VV.png), that mask
agree; ground-truth normals in camera space ('gt_normal_world' false) are rotated to the world as tools/evaluate.py does.
--lights FILE: the light directions of the shadow maps: the cameras file itself (its 'light_direction'), a .npy / .json [L, 3], or a
text table.  shadow/view_VV.npy is bool [L, H, W]: True where the light is visible from the surface point under the pixel going by
the mesh (meshrender.mesh_light_visibility: binary occlusion, not the network's transmittance); off the mesh True.
--textures: --mesh is a textured asset of tools/bake_materials.py (name.obj with name_albedo.png / name_normal.png /
name_specular.npy / name_ao.png / name_bent.png beside it, whichever exist); each map is looked up at the first hits
(meshbake.atlas_sample) and written as <map>/view_VV.npy (float32 [H, W, C], NaN off the mesh) and, for all but specular, .png.  The
PNG maps are read back as the bytes they are (albedo and occlusion u / 255, normal and bent 2 u / 255 - 1): what another renderer
would see.
On a GPU everything runs on the device; --host takes the numpy definition (small meshes only: it is a brute force)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_lights(path, view):
    """[L, 3] float64 light directions for view index ``view`` (0-based) from any of the accepted files."""
    ext = os.path.splitext(path)[1].lower()
    if ext == '.npy':
        table = np.load(path)
    elif ext == '.json':
        with open(path) as f:
            table = json.load(f)
        if isinstance(table, dict):
            same = table.get('light_is_same', True)
            table = table['light_direction'] if same else table['light_direction'][view]
    else:
        table = np.loadtxt(path)
    table = np.asarray(table, dtype=np.float64).reshape(-1, 3)
    if table.shape[0] == 0:
        raise SystemExit('render_mesh: %s holds no light direction' % path)
    return table


def save_png(path, array):
    try:
        from PIL import Image
    except ImportError:
        return False
    Image.fromarray(array).save(path)
    return True


def read_textures(mesh_path, n_faces):
    """The maps beside a baked name.obj -> ({name: float32 [T, T, C]}, Atlas)."""
    from PIL import Image
    from psnerf_amd import meshbake as mb
    base = os.path.splitext(mesh_path)[0]
    maps = {}
    for name, decode in (('albedo', lambda u: u / np.float32(255.0)), ('normal', lambda u: u * np.float32(2.0 / 255.0) - np.float32(1.0))):
        if os.path.exists(base + '_%s.png' % name):
            maps[name] = decode(np.asarray(Image.open(base + '_%s.png' % name).convert('RGB')).astype(np.float32))
    if os.path.exists(base + '_specular.npy'):
        maps['specular'] = np.load(base + '_specular.npy').astype(np.float32)
    if os.path.exists(base + '_ao.png'):                         # (bake_materials.py --occlusion)
        maps['occlusion'] = (np.asarray(Image.open(base + '_ao.png').convert('L')).astype(np.float32) / np.float32(255.0))[..., None]
    if os.path.exists(base + '_bent.png'):
        maps['bent'] = np.asarray(Image.open(base + '_bent.png').convert('RGB')).astype(np.float32) * np.float32(2.0 / 255.0) - np.float32(1.0)
    if not maps:
        raise SystemExit('render_mesh: --textures, but no %s_albedo.png / _normal.png / _specular.npy' % base)
    sizes = set(m.shape[:2] for m in maps.values())
    if len(sizes) != 1 or len(set(sizes.pop())) != 1:
        raise SystemExit('render_mesh: the maps of %s are not square textures of one size' % base)
    return maps, mb.Atlas(next(iter(maps.values())).shape[0], n_faces)


def main(argv=None):
    ap = argparse.ArgumentParser(description='Normal, depth, mask and shadow maps of a mesh from a dataset\'s cameras.')
    ap.add_argument('--mesh', required=True, help='.obj or .ply (meshdist.load_mesh)')
    ap.add_argument('--cameras', required=True, help='the dataset\'s params.json')
    ap.add_argument('--out', required=True)
    ap.add_argument('--views', type=int, nargs='*', default=None, help='view numbers from 1 (default: all)')
    ap.add_argument('--hw', type=int, nargs=2, default=None, help='image height and width (default: imhw of the cameras file)')
    ap.add_argument('--vertex-normals', action='store_true', help='interpolate the file\'s vertex normals')
    ap.add_argument('--gt-normal', default=None, help='directory of ground-truth normal maps view_VV.npy')
    ap.add_argument('--gt-mask', default=None, help='directory of ground-truth masks view_VV.png')
    ap.add_argument('--lights', default=None, help='light directions for binary shadow maps')
    ap.add_argument('--textures', action='store_true', help='--mesh is a baked asset: also look its maps up at the first hits')
    ap.add_argument('--host', action='store_true', help='run the float64 numpy definition on the CPU')
    args = ap.parse_args(argv)

    import torch
    from psnerf_amd import imgmetrics as im, meshdist as md, meshrender as mr, metrics
    if not args.host and not torch.cuda.is_available():
        raise SystemExit('render_mesh: no GPU visible (the device path has no fall-back; --host runs the numpy definition)')
    dev = None if args.host else torch.device('cuda:0')
    mesh = md.load_mesh(args.mesh)
    if len(mesh.faces) == 0:
        raise SystemExit('render_mesh: %s has no faces' % args.mesh)
    vn = None
    if args.vertex_normals:
        if mesh.vertex_normals is None:
            raise SystemExit('render_mesh: %s carries no vertex normals' % args.mesh)
        vn = mesh.vertex_normals
    index = mr._index(mesh, dev if dev is not None else 'cpu')       # one index for every view
    textures, atlas = read_textures(args.mesh, len(mesh.faces)) if args.textures else (None, None)
    if textures is not None and dev is not None:
        textures = dict((k, torch.from_numpy(np.ascontiguousarray(t)).to(dev)) for k, t in textures.items())
    with open(args.cameras) as f:
        para = json.load(f)
    H, W = args.hw if args.hw is not None else para['imhw']
    K = torch.from_numpy(np.array(para['K']).astype(np.float32))[None]
    pose_gl = np.array(para['pose_c2w']).astype(np.float32)
    pose = pose_gl.copy()
    pose[:, :3, 1:3] *= -1.0                                          # OpenGL -> OpenCV, stage1/dataloading/dataset.py:56
    views = args.views if args.views else list(range(1, int(para.get('n_view', len(pose))) + 1))
    for sub in ('normal', 'depth', 'mask') + (('shadow',) if args.lights else ()) + tuple('tex_' + k for k in (textures or ())):
        os.makedirs(os.path.join(args.out, sub), exist_ok=True)
    maes, wrote_png = [], True
    for vi in views:
        if not 1 <= vi <= len(pose):
            raise SystemExit('render_mesh: view %d of %d' % (vi, len(pose)))
        name = 'view_%02d' % vi
        c2w = torch.from_numpy(pose[vi - 1])[None]
        if dev is not None:
            out = mr.render_view(index, K.to(dev), c2w.to(dev), H, W, vertex_normals=vn, textures=textures, atlas=atlas)
        else:
            out = mr.render_view(index, K, c2w, H, W, vertex_normals=vn, textures=textures, atlas=atlas)
        mask = out['mask']
        normal = out['normals'].to(torch.float32)
        depth = out['depth'].to(torch.float32)
        np.save(os.path.join(args.out, 'normal', name + '.npy'), normal.cpu().numpy())
        np.save(os.path.join(args.out, 'depth', name + '.npy'), depth.cpu().numpy())
        np.save(os.path.join(args.out, 'mask', name + '.npy'), mask.cpu().numpy())
        on = depth[mask]
        lo, hi = (float(on.min()), float(on.max())) if on.numel() else (0.0, 1.0)
        shade = torch.where(mask, 1.0 - 0.8 * (depth - lo) / max(hi - lo, 1e-12), torch.zeros_like(depth))
        wrote_png = (save_png(os.path.join(args.out, 'normal', name + '.png'), im.to_img((normal + 1.0) / 2.0 * mask[..., None]).cpu().numpy())
                     and save_png(os.path.join(args.out, 'depth', name + '.png'), im.to_img(shade).cpu().numpy())
                     and save_png(os.path.join(args.out, 'mask', name + '.png'), im.to_img(mask.to(torch.float32)).cpu().numpy()))
        line = '%s: %d of %d pixels on the mesh, depth %.4f .. %.4f' % (name, int(mask.sum()), H * W, lo, hi)
        for key in (textures or ()):
            tex = out[key].to(torch.float32)
            np.save(os.path.join(args.out, 'tex_' + key, name + '.npy'), tex.cpu().numpy())
            if key in ('albedo', 'normal', 'occlusion', 'bent'):
                shown = torch.nan_to_num((tex + 1.0) / 2.0 if key in ('normal', 'bent') else tex, nan=0.0) * mask[..., None]
                shown = im.to_img(shown).cpu().numpy()
                save_png(os.path.join(args.out, 'tex_' + key, name + '.png'), shown[..., 0] if shown.shape[-1] == 1 else shown)
        if args.gt_normal:
            gt = np.load(os.path.join(args.gt_normal, name + '.npy')).astype(np.float32)
            if not para.get('gt_normal_world', True):
                gt = np.einsum('ij,hwj->hwi', pose_gl[vi - 1, :3, :3], gt)         # tools/evaluate.py
            both = mask.cpu().numpy() & (np.abs(gt).sum(-1) > 0)
            if args.gt_mask:
                both &= im.load_image(os.path.join(args.gt_mask, name + '.png')).astype(bool).reshape(H, W, -1)[..., 0]
            if dev is not None:
                mae = float(im.evaluate_normals(normal.contiguous(), torch.from_numpy(np.ascontiguousarray(gt)).to(dev), torch.from_numpy(both).to(dev))[0])
            else:
                mae = float(metrics.MAE(normal.numpy(), gt, both)[0])
            maes.append(mae)
            line += ', normal MAE %.3f deg over %d pixels' % (mae, int(both.sum()))
        if args.lights:
            lights = read_lights(args.lights, vi - 1)
            vis = torch.ones((lights.shape[0], H, W), dtype=torch.bool, device=mask.device)
            if bool(mask.any()):
                vis[:, mask] = mr.mesh_light_visibility(index, out['points'][mask], torch.from_numpy(lights).to(mask.device))
            np.save(os.path.join(args.out, 'shadow', name + '.npy'), vis.cpu().numpy())
            save_png(os.path.join(args.out, 'shadow', name + '.png'), im.to_img(vis.to(torch.float32).mean(0) * mask).cpu().numpy())
            line += ', %d lights, %.1f %% of the surface pixels x lights in shadow' % (lights.shape[0], 100.0 * float((~vis[:, mask]).double().mean()) if bool(mask.any()) else 0.0)
        print(line)
    if not wrote_png:
        print('PIL is not installed: .npy only')
    if maes:
        print('Normal MAE Error:  %.2f' % float(np.mean(maes)))
    return maes


if __name__ == '__main__':
    main()
