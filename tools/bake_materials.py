#!/usr/bin/env python
"""Bake the stage-2 materials onto an exported mesh and write the textured asset: name.obj + name.mtl + name_albedo.png +
name_normal.png + name_specular.npy (psnerf_amd.meshbake: two faces per square cell of the atlas, bilinear-safe gutters).

    python tools/bake_materials.py --mesh test_out/bear/test_1/mesh.ply --conf exps/bear/runconf.conf
                                   --checkpoint exps/bear/checkpoints [--epoch latest] --out baked/bear.obj
                                   [--size 2048] [--maps albedo specular normal] [--simplify N] [--chunk-faces N] [--fill 0]
                                   [--gamma 1.0] [--host] [--occlusion K [--occlusion-distance D] [--occlusion-bias B]]

--conf is the stage-2 run's conf file (stage2/confs/<obj>.conf or the runconf.conf a run leaves behind); --checkpoint is the run's
checkpoint directory (ModelParameters/<epoch>.pth inside it, as stage2/trainer.py writes them) or a ModelParameters .pth file itself.
--simplify N first reduces the mesh to about N faces (meshsimplify.simplify_mesh): a texture of T x T texels holds at most
2 (T // 4)^2 faces, and a face wants more than the minimum of 4 x 4 texels -- the tool prints the cell size it arrived at.
--occlusion K also bakes the mesh's own shadow on the same atlas (meshbake.bake_occlusion): name_ao.png, the ambient occlusion from K
cosine-weighted directions per texel (map_Ka in the MTL), and name_bent.png, the bent normals; --occlusion-distance D ends the rays at D
(default: no end), --occlusion-bias B lifts their origins by B along the normal (default: 1e-4 x the bounding-box diagonal).
On a GPU everything runs on the device; --host evaluates the networks in torch on the CPU (small meshes and textures)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_model(conf_path, checkpoint, epoch, device):
    import torch
    import psnerf_amd.stage2 as s2
    from psnerf_amd.stage2.conf import load_conf
    net = s2.PSNetwork(load_conf(conf_path))
    path = checkpoint if os.path.isfile(checkpoint) else os.path.join(checkpoint, 'ModelParameters', str(epoch) + '.pth')
    state = torch.load(path, map_location='cpu')
    net.load_state_dict(state.get('model_state_dict', state))
    return net.to(device).eval()


def main(argv=None):
    ap = argparse.ArgumentParser(description='Albedo, specular and normal textures of a stage-2 model on a mesh, as OBJ + MTL + PNG.')
    ap.add_argument('--mesh', required=True, help='.obj or .ply (meshdist.load_mesh)')
    ap.add_argument('--conf', required=True, help='the stage-2 conf file of the run')
    ap.add_argument('--checkpoint', required=True, help='the run\'s checkpoint directory, or a ModelParameters .pth file')
    ap.add_argument('--epoch', default='latest')
    ap.add_argument('--out', required=True, help='name.obj (its siblings are written next to it)')
    ap.add_argument('--size', type=int, default=2048, help='texels per side of the textures')
    ap.add_argument('--maps', nargs='+', default=['albedo', 'specular', 'normal'], choices=['albedo', 'specular', 'normal'])
    ap.add_argument('--simplify', type=int, default=None, help='reduce the mesh to about this many faces first')
    ap.add_argument('--chunk-faces', type=int, default=None)
    ap.add_argument('--fill', type=float, default=0.0, help='the value of the texels no face owns')
    ap.add_argument('--gamma', type=float, default=1.0, help='the albedo PNG stores albedo ^ (1 / gamma)')
    ap.add_argument('--occlusion', type=int, default=None, metavar='K', help='also bake ambient occlusion and bent normals from K directions')
    ap.add_argument('--occlusion-distance', type=float, default=float('inf'), metavar='D', help='the length of the occlusion rays')
    ap.add_argument('--occlusion-bias', type=float, default=None, metavar='B', help='the offset of their origins along the normal')
    ap.add_argument('--host', action='store_true', help='run on the CPU (the numpy definition, the networks in torch)')
    args = ap.parse_args(argv)

    import torch
    from psnerf_amd import meshbake as mb, meshdist as md
    if not args.host and not torch.cuda.is_available():
        raise SystemExit('bake_materials: no GPU visible (the device path has no fall-back; --host runs on the CPU)')
    dev = torch.device('cpu' if args.host else 'cuda:0')
    mesh = md.load_mesh(args.mesh)
    if len(mesh.faces) == 0:
        raise SystemExit('bake_materials: %s has no faces' % args.mesh)
    if args.simplify is not None and len(mesh.faces) > args.simplify:
        from psnerf_amd import meshsimplify
        before = len(mesh.faces)
        mesh, _ = meshsimplify.simplify_mesh(mesh, args.simplify, device=None if args.host else dev)
        print('simplified %d -> %d faces' % (before, len(mesh.faces)))
    try:
        atlas = mb.Atlas(args.size, len(mesh.faces))
    except ValueError as e:
        raise SystemExit('bake_materials: %s (a larger --size, or --simplify)' % e)
    print('%d faces in %d x %d texels: cells of %d x %d, %d rows per face, %.1f %% of the texels owned' % (
        atlas.F, atlas.T, atlas.T, atlas.c, atlas.c, atlas.K, 100.0 * atlas.F * atlas.K / atlas.T ** 2))
    net = load_model(args.conf, args.checkpoint, args.epoch, dev)
    baked = mb.bake_materials(net, mesh, size=args.size, maps=tuple(args.maps), chunk_faces=args.chunk_faces, fill=args.fill,
                              occlusion=args.occlusion, occlusion_bias=args.occlusion_bias, occlusion_distance=args.occlusion_distance)
    files = mb.export_textured(args.out, mesh, baked, gamma=args.gamma)
    for what in sorted(files):
        print('%-8s %s' % (what, files[what]))
    return files


if __name__ == '__main__':
    main()
