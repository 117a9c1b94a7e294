"""Host side of the frame rendering: OBJ reader, position colours, motions, the view rule, and the
call into the device rasteriser (ops.mesh_render_ortho / ops.pos_edge_u8)."""
import math

import numpy as np
import torch

from .. import ops

DEFAULT_SIZE = 512      # config_ortho.blend's resolution, as the 512 of blender_animation.py:72-77
DEFAULT_SPAN = 1.35     # its ortho_scale (blender_animation.py:71,77; save_mesh's ortho_scale)
MAX_SIZE = 2048


def _texture_path(obj_path, mtllib):
    """The first readable map_Kd of the OBJ's material library, or None."""
    import os
    folder = os.path.dirname(os.path.abspath(obj_path))
    mtl = os.path.join(folder, mtllib)
    if not os.path.isfile(mtl):
        return None
    with open(mtl) as fh:
        for line in fh:
            p = line.split(None, 1)
            if len(p) == 2 and p[0] == "map_Kd":
                tex = os.path.join(folder, p[1].strip())
                if os.path.isfile(tex):
                    return tex
    return None


def sample_texture(image, uvs):
    """Nearest sample of an (S,S,3) uint8 texture under the bake's convention (nsr/uv.py): image
    row r, column c holds uv * S = (c, S - 1 - r).  -> (N,3) f32 in [0,1]."""
    S = image.shape[0]
    t = np.asarray(uvs, np.float64) * S
    c = np.clip(np.floor(t[:, 0] + 0.5).astype(np.int64), 0, S - 1)
    r = np.clip(S - 1 - np.floor(t[:, 1] + 0.5).astype(np.int64), 0, S - 1)
    return (image[r, c, :3].astype(np.float32) / np.float32(255.0)).astype(np.float32)


def read_obj(path):
    """Inverse of nsr/mesh.write_obj: `v x y z [r g b]` lines and 1-based triangular faces (`f a b c`,
    `a/b/c` corners accepted).  Returns (verts (V,3) f64, faces (M,3) i64 0-based, colours (V,3) f32
    or None when no vertex carries a colour).  A textured file (nsr/mesh.write_obj_textured: no
    vertex colours, but `vt`, `mtllib` and a readable square `map_Kd`) returns the texture's nearest
    sample at each vertex's uv instead — the first uv a vertex is used with, in file order."""
    verts, cols, faces, vts, corners, mtllib = [], [], [], [], [], None
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                verts.append([float(x) for x in p[1:4]])
                if len(p) >= 7:
                    cols.append([float(x) for x in p[4:7]])
            elif p[0] == "vt":
                vts.append([float(x) for x in p[1:3]])
            elif p[0] == "mtllib" and mtllib is None and len(p) > 1:
                mtllib = line.split(None, 1)[1].strip()
            elif p[0] == "f":
                if len(p) != 4:
                    raise ValueError(f"{path}: only triangular faces are supported: {line.strip()!r}")
                faces.append([int(c.split("/")[0]) - 1 for c in p[1:4]])
                if vts:
                    corners.append([int(c.split("/")[1]) - 1 if c.count("/") and c.split("/")[1] else -1
                                    for c in p[1:4]])
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if cols and len(cols) != len(verts):
        raise ValueError(f"{path}: some vertices carry a colour and some do not")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"{path}: face index out of range")
    if cols:
        return v, f, np.asarray(cols, np.float32).reshape(-1, 3)
    tex = _texture_path(path, mtllib) if (vts and mtllib and len(corners) == len(faces)) else None
    if tex is None:
        return v, f, None
    from PIL import Image
    image = np.array(Image.open(tex).convert("RGB"))
    vt = np.asarray(vts, np.float64).reshape(-1, 2)
    ti = np.asarray(corners, np.int64).reshape(-1)
    if image.shape[0] != image.shape[1] or (ti.size and (ti.min() < 0 or ti.max() >= len(vt))):
        return v, f, None
    vi = f.reshape(-1)
    _, first = np.unique(vi, return_index=True)                        # first use of each vertex
    colours = np.zeros((len(v), 3), np.float32)
    colours[vi[first]] = sample_texture(image, vt[ti[first]])
    return v, f, colours


def read_obj_textured(path):
    """The textured triple of nsr/mesh.write_obj_textured, whole: (verts (V',3) f64, faces (M,3) i64
    0-based, uvs (V',2) f32, image (T,T,3) uint8).  A corner's `v` and `vt` indices may differ: the
    mesh then gets one vertex per distinct (v, vt) pair, in the order of first use; a file whose
    corners all read `a/a` (one uv per vertex, write_obj_textured's) comes back as it is.  ValueError when the file has
    no `vt` on every corner, no readable square `map_Kd`, or an index out of range."""
    verts, vts, corners, mtllib = [], [], [], None
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                verts.append([float(x) for x in p[1:4]])
            elif p[0] == "vt":
                vts.append([float(x) for x in p[1:3]])
            elif p[0] == "mtllib" and mtllib is None and len(p) > 1:
                mtllib = line.split(None, 1)[1].strip()
            elif p[0] == "f":
                if len(p) != 4:
                    raise ValueError(f"{path}: only triangular faces are supported: {line.strip()!r}")
                for c in p[1:4]:
                    q = c.split("/")
                    if len(q) < 2 or not q[1]:
                        raise ValueError(f"{path}: no texture coordinates (vt) on face corner {c!r}")
                    corners.append((int(q[0]) - 1, int(q[1]) - 1))
    if not vts:
        raise ValueError(f"{path}: no texture coordinates (vt)")
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    vt = np.asarray(vts, np.float64).reshape(-1, 2)
    cn = np.asarray(corners, np.int64).reshape(-1, 2)
    if cn.size and (cn[:, 0].min() < 0 or cn[:, 0].max() >= len(v)):
        raise ValueError(f"{path}: face index out of range")
    if cn.size and (cn[:, 1].min() < 0 or cn[:, 1].max() >= len(vt)):
        raise ValueError(f"{path}: vt index out of range")
    tex = _texture_path(path, mtllib) if mtllib else None
    if tex is None:
        raise ValueError(f"{path}: no readable map_Kd texture")
    from PIL import Image
    try:
        image = np.array(Image.open(tex).convert("RGB"))
    except OSError as e:
        raise ValueError(f"{path}: map_Kd {tex} is not a readable image ({e})")
    if image.shape[0] != image.shape[1]:
        raise ValueError(f"{path}: map_Kd {tex} is not square ({image.shape[1]} x {image.shape[0]})")
    if len(v) == len(vt) and np.array_equal(cn[:, 0], cn[:, 1]):
        return v, cn[:, 0].reshape(-1, 3).copy(), vt.astype(np.float32), image      # one uv per vertex already
    index, pairs = {}, []
    faces = np.empty(len(cn), np.int64)
    for k, pair in enumerate(map(tuple, cn.tolist())):
        at = index.get(pair)
        if at is None:
            at = index[pair] = len(pairs)
            pairs.append(pair)
        faces[k] = at
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return v[pairs[:, 0]], faces.reshape(-1, 3), vt[pairs[:, 1]].astype(np.float32), image


def position_colours(verts):
    """blender_animation.py:30-32: (v - min) / (max - min) per axis of the OBJ coordinates (an axis
    without extent gives 0 rather than the reference's 0 / 0)."""
    v = np.asarray(verts, np.float64)
    lo, hi = v.min(0), v.max(0)
    ext = hi - lo
    return (v - lo) / np.where(ext > 0, ext, 1.0)


def rest_pose(verts):
    """(1,V,3): the rest mesh as it is."""
    return np.asarray(verts, np.float64)[None].copy()


def rest_rotate(verts, n_frames=24):
    """(n_frames,V,3): one full turn about the vertical (y) axis through the origin; frame k is the
    rest mesh turned by 2 pi k / n_frames (x right, y up, z towards the viewer: +x turns towards
    the viewer first)."""
    if n_frames < 1:
        raise ValueError("n_frames >= 1")
    v = np.asarray(verts, np.float64)
    out = np.empty((n_frames,) + v.shape, np.float64)
    for k in range(n_frames):
        # exact quarter turns: cos / sin of k pi / 2 taken from the table, not from 1e-16 residues
        q, r = divmod(4 * k, n_frames)
        if r == 0:
            c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][q % 4]
        else:
            a = 2.0 * math.pi * k / n_frames
            c, s = math.cos(a), math.sin(a)
        out[k, :, 0] = c * v[:, 0] + s * v[:, 2]
        out[k, :, 1] = v[:, 1]
        out[k, :, 2] = -s * v[:, 0] + c * v[:, 2]
    return out


def motion_frames(verts, motion, n_frames=24):
    """'rest_pose' | 'rest_rotate' | an (F,V,3) array -> (F,V,3) f64."""
    if isinstance(motion, str):
        if motion == "rest_pose":
            return rest_pose(verts)
        if motion == "rest_rotate":
            return rest_rotate(verts, n_frames)
        raise ValueError(f"unknown motion {motion!r} (rest_pose, rest_rotate or an (F,V,3) array)")
    m = motion.detach().cpu().numpy() if torch.is_tensor(motion) else np.asarray(motion)
    m = m.astype(np.float64)
    if m.ndim != 3 or m.shape[1:] != (len(verts), 3) or m.shape[0] < 1:
        raise ValueError(f"motion of shape {m.shape}, expected (F,{len(verts)},3)")
    return m


def frame_window(frames_xyz):
    """The view rule of blender_animation.py:46-77 -> (cx, cy, size, span): the bounding box over
    all frames, the window re-centred on it; when the larger of its width and height exceeds 1.35,
    size = int(512 / 1.35 * ratio) rounded up to a multiple of 4 and span = 1.35 * size / 512,
    otherwise 512 px across 1.35."""
    p = np.asarray(frames_xyz, np.float64).reshape(-1, 3)
    if not len(p):
        return 0.0, 0.0, DEFAULT_SIZE, DEFAULT_SPAN
    lo, hi = p.min(0), p.max(0)
    cx, cy = float((hi[0] + lo[0]) / 2), float((hi[1] + lo[1]) / 2)
    ratio = float(max(hi[0] - lo[0], hi[1] - lo[1]))
    size, span = DEFAULT_SIZE, DEFAULT_SPAN
    if ratio > DEFAULT_SPAN:
        size = int(DEFAULT_SIZE / DEFAULT_SPAN * ratio)
        if size % 4 > 0:
            size = size + 4 - size % 4
        if size > MAX_SIZE:
            raise ValueError(f"the animation spans {ratio:.3f}: a {size} px window, above {MAX_SIZE}")
        span = DEFAULT_SPAN * (size / DEFAULT_SIZE)
    return cx, cy, size, span


MIP_COVERAGE = ("faces", "all")


def _texture_args(texture, uvs, texture_filter, n_verts, dev, faces=None, mip_coverage="faces",
                  max_anisotropy=None):
    """The uv / texture / filter keywords of ops.mesh_render_ortho from a host or device texture
    (T,T,3|4) uint8 and uvs (V,2), or {} without a texture.  texture_filter "trilinear" adds the
    texture's mip pyramid, built here once for all frames: mip_coverage "faces" averages only the
    texels the uv faces (M,3) cover, "all" every texel.  "anisotropic" adds the same pyramid with
    gutter = max(2, max_anisotropy) rounds — the reach of the outermost probe (include/dsu_hip.h,
    "Anisotropic frames") — and under "faces" dilates level 0 by as many rounds first (ops.uv_dilate:
    covered texels keep their bytes), so a probe that leaves its chart reads the chart's own border."""
    if mip_coverage not in MIP_COVERAGE:
        raise ValueError(f"mip_coverage must be one of {list(MIP_COVERAGE)}")
    if texture_filter == ops.ANISOTROPIC or max_anisotropy is not None:      # the cap, before anything is built
        try:
            cap = ops.check_texture_filter(texture_filter, max_anisotropy)
        except ValueError as e:
            raise ValueError(f"texture_filter / max_anisotropy: {e}") from None
    else:
        cap = None
    if (texture is None) != (uvs is None) or (texture is None and texture_filter in ops.PYRAMID_FILTERS):
        raise ValueError("texture and uvs come together or not at all (texture_filter 'trilinear' and 'anisotropic' "
                         "need both)")
    if texture is None:
        return {}
    if cap is None and texture_filter not in ops.TEXTURE_FILTERS:
        raise ValueError(f"texture_filter must be one of {sorted([*ops.TEXTURE_FILTERS, ops.ANISOTROPIC])}")
    to_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    uv = to_t(uvs).to(dev, torch.float32).reshape(-1, 2)
    if len(uv) != n_verts:
        raise ValueError("one uv per vertex")
    tex = {"uv": uv, "texture": to_t(texture).to(dev), "filter": texture_filter}
    if texture_filter in ops.PYRAMID_FILTERS:
        covered = None
        if mip_coverage == "faces":
            # the bake's own coverage rule (dsu_uv_bake): counter-clockwise uv faces only
            idx = to_t(faces).to(dev).reshape(-1, 3)
            T = tex["texture"].shape[0]
            covered = ops.uv_bake(uv, idx, torch.zeros(n_verts, 3, device=dev), T)[1] >= 0
        if cap is None:
            tex["pyramid"] = ops.mip_pyramid(tex["texture"], covered)
        else:
            gutter = max(2, cap)
            tex["max_anisotropy"] = cap
            if covered is not None:
                rgba = ops.texture_rgba(tex["texture"])
                rgb, covered = ops.uv_dilate(rgba[..., :3].contiguous(), covered, gutter)
                tex["texture"] = torch.cat([rgb, rgba[..., 3:]], -1).contiguous()
            tex["pyramid"] = ops.mip_pyramid(tex["texture"], covered, gutter)
    return tex


# The reconstruction filters of the reference's two engines (run_render.py --engine_type), as
# (window, width in pixels).  Both are UNPINNED: Blender is not here to render against, and the widths
# are read from its source — the width is the only thing a correction would change.
#   cycles  Blackman-Harris; Cycles' filter_width (1.50 px) is the total support.
#   eevee   Blackman-Harris; EEVEE's filter_size (1.50 px) scales a jitter table that spans [-1, 1]
#           (Blender 3.6, eevee_temporal_sampling.c), so the support is 2 x 1.50 px, separable.
PIXEL_FILTER_PRESETS = {"cycles": ("blackman_harris", 1.5), "eevee": ("blackman_harris", 3.0)}
PIXEL_FILTERS = ("box", "blackman_harris", *PIXEL_FILTER_PRESETS)


def _blackman_harris(d, width):
    """k(d) = 0.35875 - 0.48829 cos(2 pi u) + 0.14128 cos(4 pi u) - 0.01168 cos(6 pi u), u = d / width + 0.5,
    evaluated at -|d| so that the two sides of the window agree bit for bit."""
    u = -np.abs(np.asarray(d, np.float64)) / float(width) + 0.5
    return (0.35875 - 0.48829 * np.cos(2.0 * np.pi * u) + 0.14128 * np.cos(4.0 * np.pi * u)
            - 0.01168 * np.cos(6.0 * np.pi * u))


def pixel_filter(kind, width=None, ss=4):
    """The 1-D table of a separable pixel filter for ops.mesh_render_ortho(pixel_filter=...) (include/dsu_hip.h,
    "Pixel filter") -> (taps float64 (ss + 2 halo,), halo).

    kind "box": ones and halo 0, the unfiltered rule.  "blackman_harris": the window of total support
    `width` pixels.  "eevee" / "cycles": PIXEL_FILTER_PRESETS, with `width` overriding the preset's.
    halo = ceil((width / 2 - 0.5) ss) sub-samples, never below 0; tap q + halo = k(d_q) at
    d_q = (q + 0.5) / ss - 0.5 px where |d_q| < width / 2, else 0.  A width whose halo exceeds 2 ss (the
    rasteriser's LDS tile) is refused."""
    ss = int(ss)
    if ss not in (1, 2, 4):
        raise ValueError("ss must be 1, 2 or 4")
    if kind == "box":
        return np.ones(ss, np.float64), 0
    if kind in PIXEL_FILTER_PRESETS:
        kind, preset = PIXEL_FILTER_PRESETS[kind]
        width = preset if width is None else width
    if kind != "blackman_harris":
        raise ValueError(f"pixel filter {kind!r}: one of {list(PIXEL_FILTERS)}")
    if width is None or not np.isfinite(width) or not width > 0:
        raise ValueError("blackman_harris needs a width > 0 (pixels)")
    width = float(width)
    halo = max(int(math.ceil((width / 2.0 - 0.5) * ss)), 0)
    if halo > 2 * ss:
        raise ValueError(f"filter width {width} px reaches {halo} sub-samples beyond the pixel at ss {ss}: "
                         f"at most {2 * ss} (width 5 px)")
    d = (np.arange(-halo, ss + halo, dtype=np.float64) + 0.5) / float(ss) - 0.5
    return np.where(np.abs(d) < width / 2.0, _blackman_harris(d, width), 0.0), halo


def _pixel_filter_args(pixel_filter_kind, filter_width, ss):
    """The pixel_filter keyword of ops.mesh_render_ortho: {} for None (the call as it always was)."""
    if pixel_filter_kind is None:
        if filter_width is not None:
            raise ValueError("filter_width goes with a pixel_filter")
        return {}
    return {"pixel_filter": pixel_filter(pixel_filter_kind, filter_width, ss)}


def _vertex_colours(colours, n_verts, textured):
    """(V,3) f32 vertex colours; None is allowed (and stays None) when a texture gives the colour."""
    if colours is None and textured:
        return None
    if colours is None:
        raise ValueError("vertex colours or a texture are needed")
    c = (colours.detach().cpu().numpy() if torch.is_tensor(colours) else np.asarray(colours))
    c = c.astype(np.float32).reshape(-1, 3)
    if len(c) != n_verts:
        raise ValueError("one colour per vertex")
    return c


@torch.no_grad()
def render_frames(verts, faces, colours, motion="rest_rotate", ss=4, n_frames=24, device="cuda",
                  window=None, want=(), texture=None, uvs=None, texture_filter="bilinear", mip_coverage="faces",
                  pixel_filter=None, filter_width=None, max_anisotropy=None):
    """Render the motion of one mesh.  verts (V,3) in save_mesh's frame (x right, y up, z front; the
    viewer sits on +z), faces (M,3) 0-based, colours (V,3) in [0,1].

    texture (T,T,3|4) uint8 with uvs (V,2) (read_obj_textured's) renders the colour frames from the
    texture, sampled per sub-sample with texture_filter "bilinear", "nearest" or "trilinear"; colours
    may then be None.  The position and edge frames do not depend on it.  "trilinear" reads the
    texture's mip pyramid (ops.mip_pyramid, built once per call): where a sub-sample spans more than a
    texel — ss 1 or 2, a 2048^2 atlas, a character that fills part of the window — the two nearest
    levels are blended instead of skipping texels.  mip_coverage says which texels the coarser levels
    average: "faces" (default) those a uv face covers under the bake's rule (ops.uv_bake: counter-
    clockwise uv faces only), so the background of the atlas does not bleed into the charts; "all"
    every texel — the choice for a foreign OBJ whose charts are mirrored (clockwise in uv), which
    "faces" would count as uncovered.  "anisotropic" reads the same pyramid with up to max_anisotropy
    (1..16, default 8) probes per sub-sample along the long axis of the face's texel footprint, each at
    the level of the footprint divided by their number: a face that turns edge-on towards the
    silhouette keeps the detail along the axis that is not compressed, where "trilinear" blurs both
    (include/dsu_hip.h, "Anisotropic frames").  Its pyramid has max(2, max_anisotropy) gutter rounds
    and, under mip_coverage "faces", a level 0 dilated by as many.

    pixel_filter None is the box over a pixel's own ss^2 samples.  "eevee", "cycles" or
    "blackman_harris" (with filter_width in pixels; it overrides a preset's) reconstruct a pixel with
    that window, which reaches into the neighbouring pixels (see `pixel_filter`): silhouettes soften,
    more pixels are partially covered and the edge lines of pos2edge thicken accordingly.  "box" is the
    same rule through the filtered kernel.

    rest_pose keeps the default camera (origin-centred, 512 px across 1.35: the exported character
    fills the frame as in the reference); every other motion goes through frame_window.  `window`
    (cx, cy, size, span) overrides both.

    Returns a dict: color, pos (F,S,S,4) uint8 RGBA; edge (F,S,S) uint8 (255 = no edge); frames
    (F,6,S,S) f32, the DatasetFullImages tensor with mask and pos on; size; span; centre; plus the
    extra rasteriser outputs named in `want` (face_id, depth, pixels)."""
    dev = torch.device(device)
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    v = to_np(verts).astype(np.float64).reshape(-1, 3)
    f = to_np(faces).astype(np.int64).reshape(-1, 3)
    tex = _texture_args(texture, uvs, texture_filter, len(v), dev, f, mip_coverage, max_anisotropy)
    tex.update(_pixel_filter_args(pixel_filter, filter_width, ss))
    c = _vertex_colours(colours, len(v), texture is not None)
    xyz = motion_frames(v, motion, n_frames)
    if window is not None:
        cx, cy, size, span = window
    elif isinstance(motion, str) and motion == "rest_pose":
        cx, cy, size, span = 0.0, 0.0, DEFAULT_SIZE, DEFAULT_SPAN
    else:
        cx, cy, size, span = frame_window(xyz)
    screen = torch.from_numpy(xyz.astype(np.float32)).to(dev)
    pos = torch.from_numpy(position_colours(v).astype(np.float32)).to(dev)
    out = ops.mesh_render_ortho(screen, torch.from_numpy(f).to(dev), None if c is None else torch.from_numpy(c).to(dev),
                                pos, cx, cy, span, size, ss, want=("color_u8", "pos_u8", "frames", *want), **tex)
    res = {"color": out["color_u8"], "pos": out["pos_u8"], "edge": ops.pos_edge_u8(out["pos_u8"]),
           "frames": out["frames"], "size": int(size), "span": float(span), "centre": (cx, cy)}
    res.update({k: out[k] for k in want})
    return res
