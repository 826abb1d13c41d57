"""Drop-in for Render/render_custom_templates.py on a HIP device: renders the multi-view templates of one CAD model -- rgb_i.png,
mask_i.png and xyz_i.npy under <output_dir>/templates -- with sam6d_hip.onboard's rasteriser instead of BlenderProc, its surface
sampler instead of trimesh and PIL instead of cv2.  The reference script's arguments, plus --cam_poses: the reference's
Instance_Segmentation_Model/utils/poses/predefined_poses/cam_poses_level0.npy (this package ships no copy of it).

The geometry of the output (mask, xyz) is bitwise reproducible; the shading of rgb is the package's own and is not pinned against
Cycles.  --size and --fov default to what BlenderProc's default configuration is believed to use.  --cad_path: a PLY, or an OBJ with
its MTL; a model that names a texture image (map_Kd, or a PLY's `comment TextureFile`) is rendered with it.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _flag(v):
    """the reference declares its switches without a type, so they arrive as text"""
    if isinstance(v, bool):
        return v
    if v.lower() in ("1", "true", "yes", "on"):
        return True
    if v.lower() in ("0", "false", "no", "off"):
        return False
    raise argparse.ArgumentTypeError("expected true or false, got '%s'" % v)


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--cad_path", required=True, help="The path of CAD model (PLY or OBJ)")
    parser.add_argument("--output_dir", required=True, help="The path to save CAD templates")
    parser.add_argument("--normalize", default=True, type=_flag, help="Whether to normalize CAD model or not")
    parser.add_argument("--colorize", default=False, type=_flag, help="Whether to colorize CAD model or not")
    parser.add_argument("--base_color", default=0.05, type=float, help="The base color used in CAD model")
    parser.add_argument("--cam_poses", required=True, help="cam_poses_level0.npy of the reference (42 x 4 x 4)")
    parser.add_argument("--size", default=512, type=int, help="image side in pixels")
    parser.add_argument("--fov", default=0.691111, type=float, help="horizontal field of view in radians")
    parser.add_argument("--seed", default=0, type=int, help="seed of the surface samples behind --normalize")
    args = parser.parse_args(argv)
    if not args.cad_path.lower().endswith((".ply", ".obj")):
        parser.error("--cad_path: PLY and OBJ models are read (got %s)" % args.cad_path)
    from sam6d_hip import onboard
    mesh = onboard.load_mesh(args.cad_path)
    out = onboard.render_templates(mesh, np.load(args.cam_poses), normalize=args.normalize, colorize=args.colorize,
                                   base_color=args.base_color, size=args.size, fov=args.fov, seed=args.seed)
    save_fpath = onboard.save_templates(out, os.path.join(args.output_dir, "templates"))
    print("%d templates of %s (scale %.6g) -> %s" % (out["rgb"].shape[0], args.cad_path, out["scale"], save_fpath))


if __name__ == "__main__":
    main()
