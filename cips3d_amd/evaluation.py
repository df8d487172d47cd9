"""Evaluation / image-dump path around the generator: what
exp/cips3d/scripts/gen_images.py:30-69 (the FID path: fake images as JPEG files) and
exp/cips3d/scripts/train.py:87-170 (`save_images`: the sample grids written with every checkpoint) do with
`generator.forward`.  The float image -> uint8 quantisation of the FID path runs on the HIP library
(`cips_image_to_u8`, bit-exact torchvision arithmetic); JPEG encoding is PIL on the host, as torchvision does it.
FID itself (torch-fidelity's Inception network, eval_fid.py:36-50) is outside this repository: the submodule is not
vendored in the reference, so parity is stated on the pixels that reach it."""
import contextlib
import copy
import ctypes as C
import math
import os
from types import SimpleNamespace

import torch

from . import _lib
from ._lib import check


def image_to_u8(imgs, value_range=(-1.0, 1.0)):
    """(B, C, H, W) fp32 on the GPU -> (B, H, W, C) uint8, quantised exactly like torchvision.utils.save_image(img,
    normalize=True, value_range=value_range) (gen_images.py:60)."""
    if not imgs.is_cuda:
        raise RuntimeError("image_to_u8 needs a tensor on the GPU (no CPU fallback)")
    x = imgs.detach().contiguous().float()
    B, Cc, H, W = x.shape
    out = torch.empty(B, H, W, Cc, dtype=torch.uint8, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib.cips_image_to_u8(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), B, Cc, H, W, float(value_range[0]),
                                   float(value_range[1]), st), "cips_image_to_u8")
    return out


def _save_u8(arr_hwc, path, quality=75):
    from PIL import Image
    a = arr_hwc.cpu().numpy()
    im = Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a)
    im.save(path, **({"quality": quality} if path.lower().endswith((".jpg", ".jpeg")) else {}))


def make_grid(imgs, nrow=8, padding=2, normalize=False, value_range=None, scale_each=False, pad_value=0.0):
    """torchvision.utils.make_grid (the subset save_images uses): -> (C, H', W') float grid"""
    t = imgs.detach().float().clone()
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if normalize:
        def norm_ip(img, low, high):
            img.clamp_(min=low, max=high)
            img.sub_(low).div_(max(high - low, 1e-5))

        def norm_range(img, vr):
            if vr is not None:
                norm_ip(img, vr[0], vr[1])
            else:
                norm_ip(img, float(img.min()), float(img.max()))
        if scale_each:
            for im in t:
                norm_range(im, value_range)
        else:
            norm_range(t, value_range)
    if t.size(0) == 1:
        return t.squeeze(0)
    nmaps = t.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    h, w = int(t.size(2) + padding), int(t.size(3) + padding)
    grid = t.new_full((t.size(1), h * ymaps + padding, w * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * h + padding, h - padding).narrow(2, x * w + padding, w - padding).copy_(t[k])
            k += 1
    return grid


def save_image(imgs, path, nrow=8, padding=2, normalize=False, value_range=None, scale_each=False):
    """torchvision.utils.save_image: grid -> uint8 (the HIP quantiser for GPU tensors) -> PIL."""
    grid = make_grid(imgs, nrow=nrow, padding=padding, normalize=normalize, value_range=value_range, scale_each=scale_each)
    if grid.is_cuda:
        u8 = image_to_u8(grid.unsqueeze(0), value_range=(0.0, 1.0))[0]
    else:
        u8 = grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)
    _save_u8(u8, path)


def density_lattice(N, cube_length, center):
    """The three coordinate tensors (x, y, z), each (N,) fp32 on the CPU, of GeneratorNerfINR.density_grid's lattice: axis a
    runs from center[a] - L/2 to center[a] + L/2 as  arange(N) * (L / (N - 1)) + (center[a] - L/2)  — integer indices times
    one voxel size (rounded to fp32 once), unlike exp/pigan/scripts/extract_shapes.py:18-31 (see density_grid)."""
    if N < 2:
        raise ValueError("a density lattice needs at least 2 points per axis")
    idx = torch.arange(N, dtype=torch.float32)
    return tuple(idx * (cube_length / (N - 1)) + (c - cube_length / 2) for c in center)


def save_ply(path, vertices, faces, normals=None, colors=None):
    """One triangle mesh (GeneratorNerfINR.extract_mesh, ops.mesh_from_volume) as a binary little-endian PLY file: vertices
    (V, 3) as float x y z, normals (V, 3) as float nx ny nz when given, colors (V, 3) in [-1, 1] (extract_mesh(colors=...)) as
    uchar red green blue when given, faces (T, 3) as `list uchar int vertex_indices`.  Colours are quantised by image_to_u8's
    rule for value_range (-1, 1), in fp32 with every step rounded on its own: clamp, (c + 1) * 0.5, * 255, + 0.5, clamp to
    [0, 255], truncate.  Tensors on any device or arrays.  Without colors the file is what it was before colours existed, byte
    for byte.  (No .mrc writer: see DESIGN.md section 6.)"""
    import numpy as np

    def host(t, dtype):
        return np.ascontiguousarray((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(dtype))
    v, f = host(vertices, "<f4"), host(faces, "<i4")
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("save_ply takes vertices (V, 3) and faces (T, 3)")
    cols = [v]
    props = ["property float x", "property float y", "property float z"]
    if normals is not None:
        n = host(normals, "<f4")
        if n.shape != v.shape:
            raise ValueError("save_ply: normals must have the vertices' shape")
        cols.append(n)
        props += ["property float nx", "property float ny", "property float nz"]
    body = np.ascontiguousarray(np.concatenate(cols, 1))
    if colors is not None:
        c = host(colors, "<f4")
        if c.shape != v.shape:
            raise ValueError("save_ply: colors must have the vertices' shape")
        one, half = np.float32(1.), np.float32(0.5)
        q = (np.clip(c, -one, one) + one) * half
        q = np.clip(q * np.float32(255.) + half, np.float32(0.), np.float32(255.)).astype("u1")
        props += ["property uchar red", "property uchar green", "property uchar blue"]
        packed = np.empty(len(v), dtype=[("f", "<f4", (body.shape[1],)), ("c", "u1", (3,))])      # one vertex, no padding
        packed["f"] = body
        packed["c"] = q
        body = packed
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", *props, f"element face {len(f)}",
              "property list uchar int vertex_indices", "end_header"]
    rows = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rows["n"] = 3
    rows["i"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(body.tobytes())
        fh.write(rows.tobytes())


@torch.no_grad()
def shade_surface(surface, light=(0., 0., 1.), ambient=0.2, albedo=False):
    """A picture of GeneratorNerfINR.surface's result for save_image / save_images: Lambert shading of the normals,
    ambient + (1 - ambient) * max(0, n . l) with l = light / |light| (world space), mapped to [-1, 1] and repeated over three
    channels -> (b, 3, H, W); -1 (black) where mask == 0, the rays that cross no surface.
    albedo=True with surface.rgb present (GeneratorNerfINR.surface_colored): the Lambert factor multiplies the colour instead of white —
    (rgb + 1) / 2 in [0, 1] times the factor, mapped back to [-1, 1]; the background stays -1.  Without .rgb, or by default,
    the grey picture."""
    if surface.normals is None:
        raise ValueError("shade_surface needs normals (GeneratorNerfINR.surface(..., normals=True))")
    n = surface.normals
    l = torch.tensor(light, dtype=n.dtype, device=n.device)
    l = l / l.norm()
    lambert = (n * l.view(1, 3, 1, 1)).sum(1, keepdim=True).clamp(0., 1.)
    if albedo and getattr(surface, "rgb", None) is not None:
        shade = (surface.rgb.clamp(-1., 1.) + 1.) * 0.5 * (ambient + (1. - ambient) * lambert) * 2. - 1.
        return torch.where(surface.mask == 0, torch.full_like(shade, -1.), shade.clamp(-1., 1.)).contiguous()
    shade = (ambient + (1. - ambient) * lambert) * 2. - 1.
    shade = torch.where(surface.mask == 0, torch.full_like(shade, -1.), shade.clamp(-1., 1.))
    return shade.expand(-1, 3, -1, -1).contiguous()


@torch.no_grad()
def gen_images(rank, world_size, generator, G_kwargs, fake_dir, num_imgs, img_size, batch_size, forward_points=256 ** 2,
               progress=False):
    """gen_images.py:30-69: `num_imgs` samples of `generator` (normally G_ema) at psi = 1 as
    <fake_dir>/<index:05d>.jpg, interleaved over ranks exactly like the reference (index = batch * batch_size +
    i * world_size + rank).  Returns the number of files this rank wrote."""
    if rank == 0:
        os.makedirs(fake_dir, exist_ok=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()
    metadata = copy.deepcopy(dict(G_kwargs))
    batch_gpu = batch_size // world_size
    metadata["img_size"] = img_size
    metadata["psi"] = 1
    generator.eval()
    written = 0
    for idx_b in range((num_imgs + batch_size - 1) // batch_size):
        zs = generator.get_zs(batch_gpu)
        generated = generator(zs, forward_points=forward_points, **metadata)[0]
        u8 = image_to_u8(generated, value_range=(-1.0, 1.0))
        for idx_i in range(u8.shape[0]):
            _save_u8(u8[idx_i], f"{fake_dir}/{idx_b * batch_size + idx_i * world_size + rank:0>5}.jpg")
            written += 1
        if progress and rank == 0:
            print(f"gen_images: {min((idx_b + 1) * batch_size, num_imgs)}/{num_imgs}", flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()
    return written


@torch.no_grad()
def save_images(saved_dir, G, G_ema, G_kwargs, fixed_z, img_size, forward_points=256 ** 2):
    """train.py:87-170: the six sample grids written next to every checkpoint (frontal view of G and G_ema, truncated
    G_ema, tilted views, the mirror-symmetry pair), same file names and view parameters."""
    os.makedirs(saved_dir, exist_ok=True)
    G.eval(); G_ema.eval()
    bs = len(list(fixed_z.values())[0])
    G_kwargs = copy.deepcopy(dict(G_kwargs))
    G_kwargs["img_size"] = img_size
    nrow = int(math.sqrt(bs))

    def run(net, meta, zs=fixed_z):
        return net(zs, return_aux_img=True, forward_points=forward_points, **meta)[0]

    meta = copy.deepcopy(G_kwargs); meta["h_stddev"] = 0; meta["v_stddev"] = 0
    save_image(run(G, meta), f"{saved_dir}/0Gz.jpg", nrow=nrow, normalize=True, scale_each=True)
    save_image(run(G_ema, meta), f"{saved_dir}/0Gz_ema.jpg", nrow=nrow, normalize=True, scale_each=True)
    meta["psi"] = 0.7
    save_image(run(G_ema, meta), f"{saved_dir}/0G_trunc_ema.jpg", nrow=nrow, normalize=True, scale_each=True)
    meta = copy.deepcopy(G_kwargs); meta["h_stddev"] = 0; meta["v_stddev"] = 0; meta["h_mean"] = math.pi * 0.5 + 0.5
    save_image(run(G, meta), f"{saved_dir}/0Gz_tilted.jpg", nrow=nrow, normalize=True, scale_each=True)
    save_image(run(G_ema, meta), f"{saved_dir}/0Gz_tilted_ema.jpg", nrow=nrow, normalize=True, scale_each=True)
    bs2 = min(20, bs)
    sub = {k: v[:bs2] for k, v in fixed_z.items()}
    meta = copy.deepcopy(G_kwargs); meta["h_stddev"] = 0; meta["v_stddev"] = 0; meta["h_mean"] = 1.44
    f1 = run(G_ema, meta, sub)
    meta["h_mean"] = 1.70
    f2 = run(G_ema, meta, sub)
    save_image(torch.cat([f1, f2]), f"{saved_dir}/0G_flip_ema.jpg", nrow=max(bs2 // 2, 1), normalize=True, scale_each=True)


def saved_models(model_dict, info_msg, G, G_ema, G_kwargs, fixed_z, img_size, saved_dir):
    """train.py:56-84 without tl2's rotating-directory bookkeeping: checkpoint files + info + sample grids."""
    from .checkpoint import save_models
    save_models(saved_dir, model_dict, info_msg=info_msg)
    save_images(saved_dir, G, G_ema, G_kwargs, fixed_z, img_size)


@torch.no_grad()
def render_views(G, styles, yaws, pitches=None, **render_kw):
    """The multi-view strip of the reference's Projector (exp/cips3d/models/st_web.py:66-186): the styles of
    cips3d_amd.projection.project (or of G.styles) rendered from a list of angles -> a list with one (b, 3, H, W) image
    batch per angle, each what G.forward_styles(styles, h_mean=yaw, v_mean=pitch, **render_kw) returns under no_grad.
    `pitches`: one per yaw, default pi / 2.  render_kw: forward_styles' arguments; img_size is required, the others default to
    the projection loop's camera (fov 12, rays 0.88..1.12, 24 steps, no hierarchical sampling, a fixed camera)."""
    yaws = [float(y) for y in yaws]
    pitches = [math.pi * 0.5] * len(yaws) if pitches is None else [float(p) for p in pitches]
    if len(pitches) != len(yaws):
        raise ValueError(f"render_views: {len(yaws)} yaws but {len(pitches)} pitches")
    kw = dict(fov=12, ray_start=0.88, ray_end=1.12, num_steps=24, h_stddev=0., v_stddev=0., hierarchical_sample=False,
              sample_dist='gaussian')
    kw.update(render_kw)
    return [G.forward_styles(styles, h_mean=yaw, v_mean=pitch, **kw)[0] for yaw, pitch in zip(yaws, pitches)]


def relative_pose(tgt_cam2world, src_cam2world):
    """Two cam2world batches (b,4,4) or (b,3,4), as the namespaces of GeneratorNerfINR.render() / geometry() / surface() carry
    them -> tgt2src (b,3,4) fp32 = [R_s^T R_t | R_s^T (t_t - t_s)]: the rigid transform that takes a point of the target
    camera's space to the source camera's, what ops.reproject wants.  Composed in fp64 on the matrices' device with plain torch
    ops and rounded to fp32 once: t_t - t_s is the difference of two camera positions of norm ~1, the one cancellation in the
    reprojection chain, and it must not happen in fp32.  No gradient (the camera gets none from ops.reproject either) and no
    host synchronisation."""
    for name, m in (("tgt_cam2world", tgt_cam2world), ("src_cam2world", src_cam2world)):
        if m.dim() != 3 or m.shape[1] not in (3, 4) or m.shape[2] != 4:
            raise ValueError(f"relative_pose: {name} (b,4,4) or (b,3,4) expected, got {tuple(m.shape)}")
    if tgt_cam2world.shape[0] != src_cam2world.shape[0]:
        raise ValueError(f"relative_pose: {tgt_cam2world.shape[0]} target cameras but {src_cam2world.shape[0]} source cameras")
    with torch.no_grad():
        t, s = tgt_cam2world.detach().double(), src_cam2world.detach().double()
        RsT = s[:, :3, :3].transpose(1, 2)
        rot = RsT @ t[:, :3, :3]
        trans = RsT @ (t[:, :3, 3:] - s[:, :3, 3:])
        return torch.cat([rot, trans], 2).float().contiguous()


def world2cam(cam2world):
    """cam2world (b,4,4) or (b,3,4), a rigid camera matrix -> its inverse [R^T | -R^T t] (b,3,4) fp32, what ops.rasterize wants:
    composed in fp64 on the matrices' device and rounded to fp32 once, as relative_pose is.  No gradient, no host
    synchronisation."""
    if cam2world.dim() != 3 or cam2world.shape[1] not in (3, 4) or cam2world.shape[2] != 4:
        raise ValueError(f"world2cam: cam2world (b,4,4) or (b,3,4) expected, got {tuple(cam2world.shape)}")
    with torch.no_grad():
        m = cam2world.detach().double()
        rt = m[:, :3, :3].transpose(1, 2)
        return torch.cat([rt, -(rt @ m[:, :3, 3:])], 2).float().contiguous()


def orbit_cameras(yaws, pitches=None, radius=1.0, lookat=(0., 0., 0.), device='cuda'):
    """Cameras on a sphere around `lookat`, looking at it -> cam2world (b,4,4) fp32 on `device`: camera b sits at yaw yaws[b]
    and pitch pitches[b] (default pi / 2, the equator) at distance `radius`, built from camera_origin_from_angles and
    create_cam2world_matrix — for lookat = 0 and radius = 1 the camera that forward(h_mean=yaw, v_mean=pitch, h_stddev=0,
    v_stddev=0) and render_views use for those angles."""
    from .generator import _normalize, camera_origin_from_angles, create_cam2world_matrix
    yaws = [float(y) for y in yaws]
    pitches = [math.pi * 0.5] * len(yaws) if pitches is None else [float(p) for p in pitches]
    if len(pitches) != len(yaws):
        raise ValueError(f"orbit_cameras: {len(yaws)} yaws but {len(pitches)} pitches")
    theta = torch.tensor(yaws, dtype=torch.float32, device=device).view(-1, 1)
    phi = torch.tensor(pitches, dtype=torch.float32, device=device).view(-1, 1)
    offset, _ = camera_origin_from_angles(theta, phi, float(radius))
    origin = offset + torch.tensor([float(c) for c in lookat], dtype=torch.float32, device=device)
    return create_cam2world_matrix(_normalize(-offset), origin)


@torch.no_grad()
def render_mesh(mesh, cam2world, fov, img_size, near=1e-4, far=float('inf'), cull=None):
    """One triangle mesh seen from b cameras, without the network: ops.rasterize and ops.raster_interpolate.  mesh: anything
    with .vertices (V,3) fp32 and .faces (T,3) int32 on the GPU and optionally .normals, .colors (V,3) — an element of
    GeneratorNerfINR.extract_mesh's list, or a mesh loaded from elsewhere; cam2world (b,4,4) (orbit_cameras, or the cam2world
    of a render()/surface() namespace); fov in degrees; img_size: H = W.  -> SimpleNamespace in surface()'s layout:
      depth   (b,1,H,W)  distance along the unit ray, `far` on the background
      mask    (b,1,H,W)  uint8, 1 where a triangle was hit, 0 elsewhere
      points  (b,3,H,W)  the interpolated vertices (zeros on the background)
      normals (b,3,H,W)  mesh.normals interpolated and renormalised where the mesh has them, otherwise the geometric normal of
                         the triangle hit, (v1-v0) x (v2-v0) normalised; exact zeros on the background
      rgb     (b,3,H,W)  only if the mesh has .colors: interpolated, -1 on the background
      face (b,H,W) int32, bary (b,H,W,3), cam2world
    so that shade_surface and save_image take it as they take surface()'s result.  near, far, cull: ops.rasterize's.  A view
    costs a pass over the triangles and the pixels; extract once, render as many views as wanted.  Forward only."""
    from . import ops
    from .generator import _zc
    vertices, faces = mesh.vertices, mesh.faces
    H = int(img_size)
    face, bary, depth, mask = ops.rasterize(vertices, faces, world2cam(cam2world), _zc(fov), H, H, near=near, far=far, cull=cull)
    hit = mask.unsqueeze(1) != 0
    out = SimpleNamespace(depth=depth.unsqueeze(1), mask=mask.unsqueeze(1), face=face, bary=bary, cam2world=cam2world,
                          points=ops.raster_interpolate(face, bary, faces, vertices))
    vn = getattr(mesh, "normals", None)
    if vn is not None:
        n = ops.raster_interpolate(face, bary, faces, vn)
        norm = n.norm(dim=1, keepdim=True)
        out.normals = torch.where(hit & (norm > 0), n / norm, torch.zeros_like(n))
    else:
        if vertices.shape[0] and faces.shape[0]:
            # (T, 3 corners, 3); an index outside the mesh is clamped for the gather: the rasteriser never hits such a triangle
            tri = vertices[faces.long().clamp(0, vertices.shape[0] - 1)]
            fn = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1)
            norm = fn.norm(dim=-1, keepdim=True)
            fn = torch.where(norm > 0, fn / norm, torch.zeros_like(fn))
            picked = fn[face.clamp_min(0).long()]
        else:
            picked = torch.zeros(*face.shape, 3, device=face.device)
        out.normals = torch.where(hit, picked.permute(0, 3, 1, 2), torch.zeros((), device=face.device)).contiguous()
    colors = getattr(mesh, "colors", None)
    if colors is not None:
        out.rgb = ops.raster_interpolate(face, bary, faces, colors, fill=-1.)
    return out


def render_volume(volume, cam2world, fov, img_size, ray_start, ray_end, num_steps, clamp_mode='relu', last_back=False,
                  white_back=False, skip=True, grad=False):
    """A baked volume seen from b cameras, without the network: ops.render_volume.  volume: anything with .rgbs (Bv,nx,ny,nz,4),
    .occupancy, .lo and .hi — GeneratorNerfINR.bake's namespace, Bv = 1 (a turntable of one volume) or b; cam2world (b,4,4)
    (orbit_cameras, or the cam2world of a render() namespace); fov in degrees; img_size: H = W; ray_start, ray_end, num_steps:
    the depths linspace(ray_start, ray_end, num_steps) of forward() before jitter; clamp_mode, last_back, white_back:
    forward()'s; skip: the empty-space skip (same bits either way; 'relu' only, pass skip=False with 'softplus').
    -> SimpleNamespace in render()'s layout:
      imgs    (b,3,H,W)  the composited colours ('aux' colours for a volume of bake): soft and view-consistent
      depth   (b,1,H,W)  the expected depth sum w z
      opacity (b,1,H,W)  sum w, the matte
      cam2world
    so that save_image and warp_view take it as they take render()'s result.  grad=False (the default) runs under no_grad;
    grad=True runs with autograd as the caller has it: where volume.rgbs or cam2world requires a gradient, imgs, depth and
    opacity are differentiable with respect to it (the nodes and the cameras: ops.render_volume; a cam2world built from leaf
    angles keeps its graph, fit_cameras does that), and volume.occupancy must be the occupancy of volume.rgbs as it stands
    (ops.volume_occupancy)."""
    from . import ops
    from .generator import _zc
    H = int(img_size)
    with contextlib.nullcontext() if grad else torch.no_grad():
        rgb, depth, opacity = ops.render_volume(volume.rgbs, volume.occupancy, volume.lo, volume.hi, cam2world, _zc(fov), H, H,
                                                ray_start=ray_start, ray_end=ray_end, num_steps=num_steps, clamp_mode=clamp_mode,
                                                last_back=last_back, white_back=white_back, skip=skip)
    return SimpleNamespace(imgs=rgb, depth=depth, opacity=opacity, cam2world=cam2world)


@torch.no_grad()
def render_feature_volume(G, volume, cam2world, fov, img_size, ray_start, ray_end, num_steps, clamp_mode='relu', last_back=False,
                          white_back=False, skip=True, return_aux_img=False):
    """A baked feature volume seen from b cameras: forward()'s picture without the SIREN.  ops.render_feature_volume composites
    the 32 features per ray, then the generator's own tail runs on them — G._head (the INR head WITHOUT img_size, as forward()
    calls it, and the auxiliary layer with its tanh) and G._images (G.filters): the code _render runs behind its NeRF stage.
    G: the generator the volume was baked from; volume: GeneratorNerfINR.bake_features' namespace (.sigma, .features,
    .occupancy, .lo, .hi, .styles), one volume for all b cameras (its styles are expanded to b) or one per camera; the other
    arguments: render_volume's.  -> SimpleNamespace in render()'s layout:
      imgs     (b,3,H,W)   the INR image
      aux      (b,3,H,W)   the auxiliary image, only with return_aux_img
      depth    (b,1,H,W)   the expected depth sum w z
      opacity  (b,1,H,W)   sum w, the matte
      features (b,H*W,32)  the composited features the head ran on
      cam2world
    so that save_image and warp_view take it as they take render()'s result.  A view costs a gather-and-composite pass and
    one head pass over H W pixels, where forward() costs H W num_steps SIREN evaluations.  No gradient; GPU only."""
    from . import ops
    from .generator import _zc
    H = int(img_size)
    fea, depth, opacity = ops.render_feature_volume(volume.sigma, volume.features, volume.occupancy, volume.lo, volume.hi,
                                                    cam2world, _zc(fov), H, H, ray_start=ray_start, ray_end=ray_end,
                                                    num_steps=num_steps, clamp_mode=clamp_mode, last_back=last_back,
                                                    white_back=white_back, skip=skip)
    b = fea.shape[0]
    styles = {name: (t.expand(b, -1).contiguous() if t.shape[0] == 1 and b != 1 else t) for name, t in volume.styles.items()}
    rows, aux_rows = G._head(SimpleNamespace(return_aux_img=bool(return_aux_img)), fea, styles, False)
    inr_img, aux_img = G._images(rows, aux_rows, b, H)
    out = SimpleNamespace(imgs=inr_img.contiguous(), depth=depth, opacity=opacity, features=fea, cam2world=cam2world)
    if return_aux_img:
        out.aux = aux_img.contiguous()
    return out


def fit_volume(volume, targets, cam2world, fov, ray_start, ray_end, num_steps, *, steps, lr, clamp_mode='relu', last_back=False,
               white_back=False, level_weights=(1.,), kind='mse', target_depth=None, target_opacity=None, depth_weight=0.,
               opacity_weight=0.):
    """Fit the nodes of a baked volume to images: a copy of volume.rgbs (Bv,nx,ny,nz,4) — colours and sigma — is optimised so
    that render_volume from cam2world (b,4,4) gives targets (b,3,H,H).  Bv = 1: one volume seen from b views; Bv = b: one volume
    per view.  fov, ray_start, ray_end, num_steps, clamp_mode, last_back, white_back: render_volume's.
    Per step: ops.render_volume with autograd -> loss (b,) = ops.pyramid_loss(imgs, targets, None, level_weights, kind)
    + depth_weight * MSE(depth, target_depth (b,1,H,H)) + opacity_weight * MSE(opacity, target_opacity (b,1,H,H)) (a term runs
    where its weight is > 0; it then needs its target) -> backward to the nodes -> FusedClipAdamEMA without clip or EMA, as
    projection.project uses it.  Under 'relu' the occupancy is refreshed from the moving sigma (ops.volume_occupancy) before
    every forward, so the empty-space skip stays exact; under 'softplus' there is no skip.  steps and lr have no defaults: the
    right values depend on the volume's scale (sigma of a baked generator is in the tens to hundreds, colours in [-1, 1]; one
    learning rate serves both).  The loop never synchronises with the host.
    -> SimpleNamespace like GeneratorNerfINR.bake's: rgbs (the fitted nodes), occupancy (of the fitted nodes), lo, hi, resolution
    (volume's, None if it has none), and losses (steps, b) on the device: the loss of every image BEFORE each step.
    The input volume is not modified."""
    from . import ops
    from .generator import _zc
    from .optim import FusedClipAdamEMA
    who = "fit_volume"
    steps = int(steps)
    lr, depth_weight, opacity_weight = float(lr), float(depth_weight), float(opacity_weight)
    if steps < 1:
        raise ValueError(f"{who}: steps >= 1 expected, got {steps}")
    if not (math.isfinite(lr) and lr > 0):
        raise ValueError(f"{who}: lr must be finite and positive, got {lr}")
    if clamp_mode not in ('relu', 'softplus'):
        raise ValueError(f"{who}: clamp_mode must be 'relu' or 'softplus', got {clamp_mode!r}")
    for name, wt, tgt in (("depth", depth_weight, target_depth), ("opacity", opacity_weight, target_opacity)):
        if not (math.isfinite(wt) and wt >= 0):
            raise ValueError(f"{who}: {name}_weight must be finite and >= 0, got {wt}")
        if wt > 0 and tgt is None:
            raise ValueError(f"{who}: {name}_weight > 0 needs target_{name}")
    rgbs = volume.rgbs
    if not torch.is_tensor(rgbs) or rgbs.dtype != torch.float32 or rgbs.dim() != 5 or rgbs.shape[-1] != 4:
        raise ValueError(f"{who}: volume.rgbs (Bv,nx,ny,nz,4) fp32 expected")
    if not torch.is_tensor(targets) or targets.dtype != torch.float32 or targets.dim() != 4 or targets.shape[1] != 3 \
            or targets.shape[2] != targets.shape[3] or targets.shape[0] == 0:
        raise ValueError(f"{who}: targets (b,3,H,H) fp32 expected, got {tuple(targets.shape) if torch.is_tensor(targets) else targets!r}")
    b, H = targets.shape[0], targets.shape[2]
    if not torch.is_tensor(cam2world) or tuple(cam2world.shape) != (b, 4, 4):
        raise ValueError(f"{who}: cam2world ({b},4,4) expected for {b} targets")
    Bv = rgbs.shape[0]
    if Bv != 1 and Bv != b:
        raise ValueError(f"{who}: one volume or one per view expected, got {Bv} volumes and {b} targets")
    for name, tgt in (("depth", target_depth), ("opacity", target_opacity)):
        if tgt is not None and (not torch.is_tensor(tgt) or tgt.dtype != torch.float32 or tuple(tgt.shape) != (b, 1, H, H)):
            raise ValueError(f"{who}: target_{name} ({b},1,{H},{H}) fp32 expected")
    if not (rgbs.is_cuda and targets.is_cuda and cam2world.is_cuda):
        raise ValueError(f"{who} needs tensors on the GPU (no CPU fallback)")
    use_depth, use_opacity = depth_weight > 0, opacity_weight > 0
    targets = targets.detach().contiguous()
    target_depth = target_depth.detach().contiguous() if use_depth else None
    target_opacity = target_opacity.detach().contiguous() if use_opacity else None
    cam2world = cam2world.detach().contiguous()
    zc, skip, dev = _zc(fov), clamp_mode == 'relu', rgbs.device
    nodes = rgbs.detach().clone(memory_format=torch.contiguous_format).requires_grad_(True)
    nodes.grad = torch.zeros_like(nodes)                 # one buffer for every step: autograd adds into it in place
    opt = FusedClipAdamEMA([nodes], lr=lr, betas=(0.9, 0.999))
    losses = torch.zeros(steps, b, device=dev)
    ones = torch.ones(b, device=dev)
    zg = ops.pixel_grids(H, H, int(num_steps), ray_start, ray_end, dev)[2]
    for i in range(steps):
        with torch.no_grad():
            nodes.grad.zero_()
            occ = ops.volume_occupancy(nodes) if skip else None
        with torch.enable_grad():
            rgb, depth, opacity = ops.render_volume(nodes, occ, volume.lo, volume.hi, cam2world, zc, H, H, zg=zg,
                                                    clamp_mode=clamp_mode, last_back=last_back, white_back=white_back, skip=skip)
            loss = ops.pyramid_loss(rgb, targets, None, level_weights, kind)
            if use_depth:
                loss = loss + ops.pyramid_loss(depth, target_depth, None, (1.,), "mse") * depth_weight
            if use_opacity:
                loss = loss + ops.pyramid_loss(opacity, target_opacity, None, (1.,), "mse") * opacity_weight
        losses[i].copy_(loss.detach())
        torch.autograd.backward(loss, ones)
        opt.step()
    fitted = nodes.detach()
    return SimpleNamespace(rgbs=fitted, occupancy=ops.volume_occupancy(fitted), lo=volume.lo, hi=volume.hi,
                           resolution=getattr(volume, "resolution", None), losses=losses)


def fit_cameras(volume, targets, fov, ray_start, ray_end, num_steps, *, yaws, pitches, radius=1.0, lookat=(0., 0., 0.), steps, lr,
                fit_radius=False, target_depth=None, target_mask=None, depth_weight=0., mask_weight=0., clamp_mode='relu',
                last_back=False, white_back=False, level_weights=(1.,), kind='mse', lr_decay_every=100, lr_gamma=0.75):
    """Fit one camera per view to images of a FROZEN baked volume: yaw and pitch (and, with fit_radius, the distance) of b
    cameras on spheres around `lookat` are optimised so that render_volume gives targets (b,3,H,H).  yaws, pitches: b numbers
    each, the start; radius: a number or b numbers.  volume.rgbs is (1,nx,ny,nz,4) (every view sees it) or (b,...).
    Per step: cam2world = create_cam2world_matrix(-offset, offset + lookat) with offset = camera_origin_from_angles(yaw, pitch,
    radius), the construction of orbit_cameras, kept in autograd (the first iterate is orbit_cameras(yaws, pitches, radius,
    lookat)) -> ops.render_volume -> loss (b,) = ops.pyramid_loss(imgs, targets, None, level_weights, kind)
    + depth_weight * MSE(depth, target_depth (b,1,H,H)) + mask_weight * MSE(opacity, target_mask (b,1,H,H)) (a term runs where
    its weight is > 0; it then needs its target) -> backward through cips_volume_render_bwd_cam to the angles ->
    FusedClipAdamEMA without clip or EMA at lr_at(step, lr, lr_decay_every, lr_gamma): the optimiser and schedule of
    projection.project(fit_camera=True).  The network is not in the loop, the nodes get no gradient and the loop never
    synchronises with the host.  steps and lr have no defaults.  The gradient is that of a piecewise-trilinear field: it sees
    what one sample spacing sees, so a start further off than the picture's features are wide can stall.
    -> SimpleNamespace(yaws (b,), pitches (b,), radius (b,), cam2world (b,4,4) of the fitted angles, losses (steps, b) on the
    device: the loss of every view BEFORE each step)."""
    from . import ops
    from .generator import _normalize, _zc, camera_origin_from_angles, create_cam2world_matrix
    from .optim import FusedClipAdamEMA
    from .projection import lr_at
    who = "fit_cameras"
    steps = int(steps)
    lr, depth_weight, mask_weight = float(lr), float(depth_weight), float(mask_weight)
    if steps < 1:
        raise ValueError(f"{who}: steps >= 1 expected, got {steps}")
    if not (math.isfinite(lr) and lr > 0):
        raise ValueError(f"{who}: lr must be finite and positive, got {lr}")
    if clamp_mode not in ('relu', 'softplus'):
        raise ValueError(f"{who}: clamp_mode must be 'relu' or 'softplus', got {clamp_mode!r}")
    for name, wt, tgt in (("depth", depth_weight, target_depth), ("mask", mask_weight, target_mask)):
        if not (math.isfinite(wt) and wt >= 0):
            raise ValueError(f"{who}: {name}_weight must be finite and >= 0, got {wt}")
        if wt > 0 and tgt is None:
            raise ValueError(f"{who}: {name}_weight > 0 needs target_{name}")
    rgbs = volume.rgbs
    if not torch.is_tensor(rgbs) or rgbs.dtype != torch.float32 or rgbs.dim() != 5 or rgbs.shape[-1] != 4:
        raise ValueError(f"{who}: volume.rgbs (Bv,nx,ny,nz,4) fp32 expected")
    if not torch.is_tensor(targets) or targets.dtype != torch.float32 or targets.dim() != 4 or targets.shape[1] != 3 \
            or targets.shape[2] != targets.shape[3] or targets.shape[0] == 0:
        raise ValueError(f"{who}: targets (b,3,H,H) fp32 expected, got {tuple(targets.shape) if torch.is_tensor(targets) else targets!r}")
    b, H = targets.shape[0], targets.shape[2]
    if rgbs.shape[0] != 1 and rgbs.shape[0] != b:
        raise ValueError(f"{who}: one volume or one per view expected, got {rgbs.shape[0]} volumes and {b} targets")
    for name, tgt in (("depth", target_depth), ("mask", target_mask)):
        if tgt is not None and (not torch.is_tensor(tgt) or tgt.dtype != torch.float32 or tuple(tgt.shape) != (b, 1, H, H)):
            raise ValueError(f"{who}: target_{name} ({b},1,{H},{H}) fp32 expected")
    try:
        yaws, pitches = [float(v) for v in yaws], [float(v) for v in pitches]
        radius = [float(v) for v in radius] if isinstance(radius, (tuple, list)) else [float(radius)] * b
        lookat = [float(v) for v in lookat]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: yaws, pitches, radius and lookat must be numbers") from None
    if len(yaws) != b or len(pitches) != b or len(radius) != b or len(lookat) != 3:
        raise ValueError(f"{who}: {b} yaws, pitches (and radii) and a lookat of 3 numbers expected for {b} targets")
    if not all(math.isfinite(v) for v in yaws + pitches + radius + lookat) or not all(r > 0 for r in radius):
        raise ValueError(f"{who}: finite angles and lookat and a positive radius expected")
    if not (rgbs.is_cuda and targets.is_cuda):
        raise ValueError(f"{who} needs tensors on the GPU (no CPU fallback)")
    use_depth, use_mask = depth_weight > 0, mask_weight > 0
    dev = rgbs.device
    targets = targets.detach().contiguous()
    target_depth = target_depth.detach().contiguous() if use_depth else None
    target_mask = target_mask.detach().contiguous() if use_mask else None
    nodes, occ = rgbs.detach().contiguous(), volume.occupancy
    zc, skip = _zc(fov), clamp_mode == 'relu'
    column = lambda v: torch.tensor(v, dtype=torch.float32, device=dev).view(b, 1)
    theta, phi, rad = column(yaws).requires_grad_(True), column(pitches).requires_grad_(True), column(radius)
    centre = torch.tensor(lookat, dtype=torch.float32, device=dev)
    leaves = [theta, phi] + ([rad.requires_grad_(True)] if fit_radius else [])

    def cameras():
        offset, _ = camera_origin_from_angles(theta, phi, rad)
        return create_cam2world_matrix(_normalize(-offset), offset + centre)

    opt = FusedClipAdamEMA(leaves, lr=lr, betas=(0.9, 0.999))
    losses = torch.zeros(steps, b, device=dev)
    ones = torch.ones(b, device=dev)
    zg = ops.pixel_grids(H, H, int(num_steps), ray_start, ray_end, dev)[2]
    for i in range(steps):
        for p in leaves:
            p.grad = None
        with torch.enable_grad():
            rgb, depth, opacity = ops.render_volume(nodes, occ if skip else None, volume.lo, volume.hi, cameras(), zc, H, H, zg=zg,
                                                    clamp_mode=clamp_mode, last_back=last_back, white_back=white_back, skip=skip)
            loss = ops.pyramid_loss(rgb, targets, None, level_weights, kind)
            if use_depth:
                loss = loss + ops.pyramid_loss(depth, target_depth, None, (1.,), "mse") * depth_weight
            if use_mask:
                loss = loss + ops.pyramid_loss(opacity, target_mask, None, (1.,), "mse") * mask_weight
        losses[i].copy_(loss.detach())
        torch.autograd.backward(loss, ones)
        opt.lr = lr_at(i, lr, lr_decay_every, lr_gamma)
        opt.step()
    with torch.no_grad():
        cam2world = cameras()
    return SimpleNamespace(yaws=theta.detach().view(b), pitches=phi.detach().view(b), radius=rad.detach().view(b),
                           cam2world=cam2world, losses=losses)


def warp_view(src, tgt, fov, src_fov=None, occ_tol=None):
    """What view `src` predicts for view `tgt`: src.imgs seen from tgt's camera through tgt.depth.  src and tgt are two
    namespaces of GeneratorNerfINR.render() / render_styles() (imgs, depth, cam2world; without return_aux_img, so that imgs and
    depth have one batch size); fov: the field of view tgt was rendered with, src_fov (default fov) that of src.
    -> SimpleNamespace(imgs (b,3,Ht,Wt), mask (b,1,Ht,Wt) uint8, uv (b,2,Ht,Wt)): ops.reproject's out, mask and uv.
    occ_tol (in units of depth): a target pixel whose point lies more than occ_tol behind src.depth, sampled where it lands, is
    marked occluded (mask 2) and left black; one sample spacing of the renders, (ray_end - ray_start) / (num_steps - 1), is what
    view_consistency uses.  None: no occlusion test — the namespaces do not say what a sensible tolerance is — and every pixel
    that lands in src's frame counts as visible.
    Differentiable through src.imgs and tgt.depth (so through everything the two renders depend on); not through the mask, the
    cameras or src.depth."""
    from . import ops
    from .generator import _zc
    pose = relative_pose(tgt.cam2world, src.cam2world)
    src_depth = None if occ_tol is None else src.depth
    imgs, mask, uv = ops.reproject(src.imgs, tgt.depth, pose, _zc(fov), _zc(fov if src_fov is None else src_fov),
                                   src_depth=src_depth, occ_tol=occ_tol, return_uv=True)
    return SimpleNamespace(imgs=imgs, mask=mask, uv=uv)


@torch.no_grad()
def view_consistency(G, styles, yaw_a, yaw_b, pitch_a=math.pi * 0.5, pitch_b=math.pi * 0.5, occ_tol=None, **render_kw):
    """Multi-view consistency of the styles of cips3d_amd.projection.project (or of G.styles): view A (yaw_a, pitch_a) and view
    B (yaw_b, pitch_b) are rendered with G.render_styles, B is warped into A's camera through A's depth (warp_view, occlusion
    tested against B's depth) and compared with A where A's pixels are visible in B.  render_kw: render_styles' arguments with
    render_views' defaults (img_size is required).  The two renders make the same random draws (the generator's state is
    rewound between them and left where one render leaves it), so that what differs between them is the camera.
    occ_tol: default one sample spacing, (ray_end - ray_start) / (num_steps - 1).
    -> SimpleNamespace of
      error    (b,)  mean over the visible pixels and the channels of |a.imgs - warped|; NaN for an image with no visible pixel
      coverage (b,)  the share of A's pixels with mask == 1
      warped (b,3,H,W), mask (b,1,H,W) uint8   warp_view's imgs and mask
      a, b           the two render_styles namespaces
    A 3D-consistent generator renders one surface from both cameras and keeps the error at the level of its view-dependent
    effects and of the bilinear resampling; the number says nothing about image quality.
    A ray of A that meets no density at all has opacity 0 and depth 0: it has no point to reproject and counts as not covered
    (mask 0), also when A and B are the same view.  last_back=True gives every ray a depth.
    The tensors of a and b are detached (the NeRF path of a trainable generator records a graph under no_grad too)."""
    kw = dict(fov=12, ray_start=0.88, ray_end=1.12, num_steps=24, h_stddev=0., v_stddev=0., hierarchical_sample=False,
              sample_dist='gaussian')
    kw.update(render_kw)
    if occ_tol is None:
        occ_tol = (kw['ray_end'] - kw['ray_start']) / (kw['num_steps'] - 1)
    dev = next(G.parameters()).device
    state = torch.cuda.get_rng_state(dev) if dev.type == 'cuda' else None
    a = G.render_styles(styles, h_mean=float(yaw_a), v_mean=float(pitch_a), **kw)
    if state is not None:
        torch.cuda.set_rng_state(state, dev)
    b = G.render_styles(styles, h_mean=float(yaw_b), v_mean=float(pitch_b), **kw)
    for ns in (a, b):
        ns.imgs, ns.depth, ns.opacity = ns.imgs.detach(), ns.depth.detach(), ns.opacity.detach()
    w = warp_view(b, a, kw['fov'], occ_tol=occ_tol)
    vis = (w.mask == 1)
    n = vis.sum(dim=(1, 2, 3)).double()
    diff = ((a.imgs - w.imgs).abs() * vis).double().sum(dim=(1, 2, 3))
    error = (diff / (n * a.imgs.shape[1])).float()               # 0 / 0 = NaN: no visible pixel
    coverage = (n / vis[0].numel()).float()
    return SimpleNamespace(error=error, coverage=coverage, warped=w.imgs, mask=w.mask, a=a, b=b)
