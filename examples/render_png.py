#!/usr/bin/env python3
"""Render one of the synthetic scenes through the host layer + HIP kernels and save it as a PNG (needs an MI355X).

    python examples/render_png.py {box,helmet,skinned,atrium,zoo,instanced,transparent} out.png [--width W --height H --msaa 4 --mipmap]

The output image of the opaque pass is linear HDR RGBA16F; the PNG is Reinhard tone-mapped and gamma-encoded for viewing.  With any of
--tonemap {khronos,aces,none}, --bloom, --dof, --smaa the frame ends with the effects + display passes instead, and the PNG is the device's
RGBA8 display image as it stands (--dof uses the reference's focus distance 10 and aperture 5.6 unless --focus / --aperture say otherwise).
--sky-gradient makes the skybox the reference's default gradient sky (CubemapImage::new_sky_gradient, 256^2 with its mip chain, built on the
device); --env-ktx2 PATH loads a KTX2 cube map as the skybox and as the prefiltered environment of the IBL.  With --bake-ibl the scene is lit
by the skybox either of them made: the prefiltered chain (128^2, down to 4^2) and the irradiance cube (32^2) are filtered from it on the device.
--hdr FILE projects an equirectangular Radiance .hdr panorama into the skybox (--hdr-size N, default 512; --hdr-yaw R radians turns it about the
vertical); an EXPOSURE= in the file is divided out.  Together with --bake-ibl the scene is lit from the file.
--shadow [LIGHT] casts shadows from one directional, spot or point light of the scene (--shadow-size N, --shadow-strength X): a depth map from the
light, looked up per pixel and multiplied into the opaque image; a point light gets the six faces of a cube, and --shadow-cascades N gives a
directional light N nested maps along the camera's depth (1 .. 4).
--ssao darkens creases and contact lines: ambient occlusion estimated from the geometry pass's depth (--ssao-radius R in world units, --ssao-intensity I).
--taa N renders N frames of the still view with the projection jittered per frame and resolves each into a history (temporal anti-aliasing, in front of the
post pass: it implies the post pass) and writes the last; with --select the N frames are the selected ones.
--grid draws the editor's ground grid (the plane y = 0: unit lines, every tenth stronger, the X axis red and the Z axis blue) under the transparent meshes.
--select X,Y (may be repeated) picks the mesh under each pixel of a first frame and renders again with those meshes selected: an outline around their
visible pixels and a wire box around each one's world bounding box, dimmed where other geometry hides it.
--select-transparent [T] lets --select hit a transparent mesh where its fragment was drawn with alpha >= T (default 0.5): the pick then reads the
transparent pass's fragment lists as well as the visibility keys; such a mesh gets its box only.  --select-rect X0,Y0,X1,Y1 selects every mesh the
rectangle shows (a marquee).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from awsm_renderer_amd import scenes                      # noqa: E402
from awsm_renderer_amd.hip_backend import HipDevice       # noqa: E402
from awsm_renderer_amd.host import Renderer               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", choices=["box", "helmet", "skinned", "atrium", "zoo", "instanced", "transparent"])
    ap.add_argument("out")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--msaa", type=int, default=0, choices=(0, 4))
    ap.add_argument("--mipmap", action="store_true")
    ap.add_argument("--tonemap", choices=["khronos", "aces", "none"], help="run the post pass with this tone map (the reference's default: khronos)")
    ap.add_argument("--bloom", action="store_true")
    ap.add_argument("--dof", action="store_true")
    ap.add_argument("--smaa", action="store_true")
    ap.add_argument("--focus", type=float, default=10.0)
    ap.add_argument("--aperture", type=float, default=5.6)
    ap.add_argument("--sky-gradient", action="store_true", help="skybox = the default zenith / nadir gradient cube")
    ap.add_argument("--env-ktx2", metavar="PATH", help="a KTX2 cube map for the skybox and the prefiltered environment")
    ap.add_argument("--hdr", metavar="FILE", help="an equirectangular Radiance .hdr panorama for the skybox")
    ap.add_argument("--hdr-size", type=int, default=512, metavar="N", help="side of the skybox cube made from --hdr")
    ap.add_argument("--hdr-yaw", type=float, default=0.0, metavar="R", help="radians added to the panorama's azimuth")
    ap.add_argument("--bake-ibl", action="store_true", help="with --sky-gradient / --env-ktx2 / --hdr: filter the IBL cubes from the skybox on the device")
    ap.add_argument("--grid", action="store_true", help="the editor's ground grid, drawn by the transparent pass")
    ap.add_argument("--ssao", action="store_true", help="screen-space ambient occlusion from the visibility depth, multiplied into the opaque image")
    ap.add_argument("--ssao-radius", type=float, default=None, metavar="R", help="with --ssao: the sampling radius in world units (default 0.5)")
    ap.add_argument("--ssao-intensity", type=float, default=None, metavar="I", help="with --ssao: the estimator's scale (default 1.0)")
    ap.add_argument("--taa", type=int, default=0, metavar="N", help="temporal anti-aliasing: render N jittered frames of the still view, write the last (implies the post pass)")
    ap.add_argument("--shadow", nargs="?", const=-1, type=int, default=None, metavar="LIGHT",
                    help="shadows from one directional, spot or point light: an index into the scene's lights (default: the first directional light); not with --via-glb, "
                         "whose lights are the file's and have no index here")
    ap.add_argument("--shadow-size", type=int, default=None, metavar="N", help="with --shadow: the shadow map is N x N (default 2048)")
    ap.add_argument("--shadow-cascades", type=int, default=None, metavar="N", help="with --shadow on a directional light: N nested maps along the camera's depth, 1 .. 4 (default 1)")
    ap.add_argument("--shadow-strength", type=float, default=None, metavar="X", help="with --shadow: how dark a shadow is, 0 .. 1 (default 0.7)")
    ap.add_argument("--select", action="append", default=[], metavar="X,Y", help="select the mesh under this pixel (outline + bounding box); may be repeated; not with --via-glb")
    ap.add_argument("--select-transparent", nargs="?", const=0.5, type=float, default=None, metavar="T",
                    help="with --select / --select-rect: pick through the transparent meshes' fragments too, those drawn with alpha >= T (default 0.5); a transparent mesh gets its box only")
    ap.add_argument("--select-rect", metavar="X0,Y0,X1,Y1", help="select every mesh the rectangle [X0, X1) x [Y0, Y1) shows; not with --via-glb")
    ap.add_argument("--via-glb", action="store_true", help="write the scene to a .glb next to the output and render from the file (native glTF reader)")
    a = ap.parse_args()
    W, H = a.width, a.height
    sc = {"box": lambda: scenes.box_scene(W, H), "helmet": lambda: scenes.helmet_scene(W, H), "skinned": lambda: scenes.skinned_morph_scene(W, H),
          "atrium": lambda: scenes.atrium_scene(W, H, tex_scale=0.5), "zoo": lambda: scenes.material_zoo_scene(W, H),
          "instanced": lambda: scenes.instanced_scene(W, H), "transparent": lambda: scenes.transparent_scene(W, H, tex_size=256)}[a.scene]()
    gltf = None
    if a.via_glb:
        from awsm_renderer_amd import gltf_export
        gltf = os.path.splitext(a.out)[0] + ".glb"
        gltf_export.write_glb(sc, gltf)
    r = Renderer(sc, msaa=a.msaa, mipmap=a.mipmap, gltf=gltf)
    if a.sky_gradient:
        r.host.env_cube_sky_gradient(0, 256)
    if a.bake_ibl and not (a.sky_gradient or a.env_ktx2 or a.hdr):
        ap.error("--bake-ibl filters the skybox cube: give --sky-gradient, --env-ktx2 or --hdr")
    if a.env_ktx2:
        info = r.host.env_cube_load_ktx2(0, a.env_ktx2)
        if not a.bake_ibl:
            r.host.env_cube_load_ktx2(1, a.env_ktx2)
            r.host.set_ibl_mip_counts(info["mips"], sc.irradiance_mip_count)      # the prefiltered lookup scales roughness by the file's level count
        print(f"{a.env_ktx2}: {info['size']}^2 {info['format_name']}, {info['levels']} stored level(s), {info['mips']} in the cube")
    if a.hdr:
        from awsm_renderer_amd.host import hdr_info
        with open(a.hdr, "rb") as fh:
            data = fh.read()
        exposure = hdr_info(data)["exposure"]
        info = r.host.env_cube_load_hdr(0, data, a.hdr_size, yaw=a.hdr_yaw, scale=1.0 / exposure)
        print(f"{a.hdr}: {info['width']}x{info['height']}{' (+Y)' if info['flipped_y'] else ''}, exposure {info['exposure']:g} -> skybox {a.hdr_size}^2 with its chain")
    if a.bake_ibl:
        r.host.env_bake_ibl(128, 6, 32)                                           # 128 64 32 16 8 4; sets the IBL mip counts
    post = a.tonemap is not None or a.bloom or a.dof or a.smaa or a.taa > 0
    if post:
        from awsm_renderer_amd.hip_backend import TONEMAP
        r.set_post_processing(TONEMAP[a.tonemap or "khronos"], bloom=a.bloom, dof=a.dof, smaa=a.smaa)
        if a.dof:
            r.camera_set_dof(a.focus, a.aperture)
    if a.grid:
        r.set_editor_grid(True)
    if a.ssao:
        r.set_ssao(True, **{k: v for k, v in (("radius", a.ssao_radius), ("intensity", a.ssao_intensity)) if v is not None})
    if a.shadow is not None:
        if a.via_glb:
            ap.error("--shadow names a light by its index in the scene description; a scene read from a .glb keeps no such index (Host.set_shadow takes a light's key)")
        r.set_shadow(True if a.shadow < 0 else a.shadow, **{k: v for k, v in (("map_size", a.shadow_size), ("strength", a.shadow_strength), ("cascades", a.shadow_cascades)) if v is not None})
    if a.taa > 0:
        r.set_taa(True)
    stats = r.render(sync=True)
    picked = []
    if a.select or a.select_rect:
        if a.via_glb:
            ap.error("--select / --select-rect pick through the scene description's meshes; not with --via-glb")
        through = a.select_transparent is not None
        threshold = a.select_transparent if through else 0.5
        for xy in a.select:
            x, y = (int(v) for v in xy.split(","))
            key = r.host.pick(x, y, transparent=through, alpha_threshold=threshold)
            print(f"--select {x},{y}: " + ("nothing there" if key is None else f"mesh {key:#x}"))
            if key is not None and key not in picked:
                picked.append(key)
        if a.select_rect:
            x0, y0, x1, y1 = (int(v) for v in a.select_rect.split(","))
            shown = r.host.pick_rect(x0, y0, x1, y1, transparent=through, alpha_threshold=threshold)
            print(f"--select-rect {x0},{y0},{x1},{y1}: " + (", ".join(f"mesh {key:#x} (layer {layer}, {px} px)" for key, layer, px in shown) or "nothing there"))
            picked += [key for key, layer, _ in shown if key not in picked and layer < 2]      # HUD meshes are not selectable (the host leaves them out)
        if picked:
            r.set_selection(picked)
            stats = r.render(sync=True)
    for _ in range(a.taa - 1):      # the first of the N frames is the one above (or the selected one)
        stats = r.render(sync=True)
    dev = HipDevice.from_ctx(r.host.device_ctx, W, H)
    if post:
        rgba = dev.read_display()
        r.close()
        from PIL import Image
        Image.fromarray(rgba[..., :3]).save(a.out)
        print(f"{a.out}: {W}x{H}, post pass {a.tonemap or 'khronos'} bloom={a.bloom} dof={a.dof} smaa={a.smaa}{f' taa={a.taa} frames' if a.taa else ''}, the device's RGBA8 display image")
        return
    final = dev.read_composite() if stats["forward_triangles"] or a.grid or picked else dev.read_opaque()      # the image after the transparent pass, when the scene has one
    img = final.view(np.float16).astype(np.float32)[..., :3]
    r.close()
    ldr = np.clip(img / (1.0 + img), 0.0, 1.0) ** (1.0 / 2.2)
    from PIL import Image
    Image.fromarray((ldr * 255.0 + 0.5).astype(np.uint8)).save(a.out)
    print(f"{a.out}: {W}x{H}, {stats['triangles_in']} triangles, {stats['covered_pixels']} covered pixels, "
          f"geometry {stats['ms_transform'] + stats['ms_bin'] + stats['ms_raster']:.3f} ms, opaque {stats['ms_shade']:.3f} ms, transparent {stats['ms_forward']:.3f} ms")


if __name__ == "__main__":
    main()
