"""Float64 restatement of the pixel-filter rule (include/dsu_hip.h, "Pixel filter":
dsu_mesh_render_ortho_filtered and dsu_pixel_filter_resolve_host) in numpy.  Test infrastructure only.

Rule.  taps holds ss + 2 halo values; tap q + halo belongs to sub-sample offset q in [-halo, ss + halo)
from the pixel's first sample.  Pixel (i, j) walks rows R = i ss + qy, columns C = j ss + qx row-major;
samples outside [0, N) do not exist.  w = taps[qy + halo] taps[qx + halo]; W_all += w; a covered sample
adds w to W_cov and w v_ch to A_ch.  alpha = W_cov / W_all, channel = A_ch / W_cov (0 where W_cov is 0),
uint8 = floor(v 255 + 0.5) (0 for a value that is not a number, clamped to 0..255).

Visibility, the per-sample attributes and the `fragile` mask come from frame_render_ref (and the
textured reads from frame_render_tex_ref / frame_render_mip_ref) rendered at ss = 1 on the N x N
lattice: the lattice depends on N only, so a pixel of that render is a sample of this one.
"""
import numpy as np

import frame_render_ref as R


def quantise(v):
    with np.errstate(invalid="ignore"):
        q = np.floor(np.asarray(v, np.float64) * 255.0 + 0.5)
        return np.where(q >= 0.0, np.minimum(q, 255.0), 0.0).astype(np.uint8)


def resolve(attr, covered, taps, halo, ss):
    """attr (..., N, N, 6) per-sample colour rgb + position rgb, covered (..., N, N) bool -> dict: pixels
    (..., S, S, 8) float64 (colour rgb, alpha, pos rgb, alpha), color_u8 / pos_u8 (..., S, S, 4)."""
    attr = np.asarray(attr, np.float64)
    covered = np.asarray(covered, bool)
    taps = np.asarray(taps, np.float64)
    N = covered.shape[-1]
    S = N // ss
    assert S * ss == N and len(taps) == ss + 2 * halo and attr.shape[-3:] == (N, N, 6)
    lead = covered.shape[:-2]
    w_all, w_cov = np.zeros(lead + (S, S)), np.zeros(lead + (S, S))
    acc = np.zeros(lead + (S, S, 6))
    first = np.arange(S) * ss
    with np.errstate(invalid="ignore", over="ignore"):
        for qy in range(-halo, ss + halo):
            rows = first + qy
            ry = (rows >= 0) & (rows < N)
            for qx in range(-halo, ss + halo):
                cols = first + qx
                cx = (cols >= 0) & (cols < N)
                w = taps[qy + halo] * taps[qx + halo]
                exists = ry[:, None] & cx[None, :]
                rr, cc = np.clip(rows, 0, N - 1), np.clip(cols, 0, N - 1)
                cov = covered[..., rr[:, None], cc[None, :]] & exists
                val = attr[..., rr[:, None], cc[None, :], :]
                w_all = np.where(exists, w_all + w, w_all)
                w_cov = np.where(cov, w_cov + w, w_cov)
                acc = np.where(cov[..., None], acc + w * val, acc)
        alpha = w_cov / w_all
        v = np.where(w_cov[..., None] > 0.0, acc / np.where(w_cov > 0.0, w_cov, 1.0)[..., None], 0.0)
    pixels = np.concatenate([v[..., :3], alpha[..., None], v[..., 3:], alpha[..., None]], -1)
    q = quantise(pixels)
    return {"pixels": pixels, "color_u8": np.ascontiguousarray(q[..., :4]), "pos_u8": np.ascontiguousarray(q[..., 4:])}


def from_samples(base, taps, halo, ss):
    """The filtered frames from an ss = 1 render on the N x N lattice (frame_render_ref.render's dict, or
    a textured one): face_id, depth, fragile (and tex_fragile) stay per sample; pixels, color_u8, pos_u8
    are resolved here."""
    covered = base["face_id"] >= 0
    out = dict(base)
    out.update(resolve(base["pixels"][..., [0, 1, 2, 4, 5, 6]], covered, taps, halo, ss))
    return out


def render(screen, faces, colour, pos, cx, cy, span, S, ss, taps, halo):
    """Vertex-coloured frames under the filter: the dict of frame_render_ref.render."""
    return from_samples(R.render(screen, faces, colour, pos, cx, cy, span, S * ss, 1), taps, halo, ss)


def footprint_any(mask, halo, ss):
    """mask (F, N, N) bool per sample -> (F, S, S) bool: pixels whose footprint (the samples at offsets
    [-halo, ss + halo) in both directions) holds a marked sample."""
    F, N, _ = mask.shape
    S = N // ss
    padded = np.zeros((F, N + 2 * halo, N + 2 * halo), bool)
    padded[:, halo:halo + N, halo:halo + N] = mask
    out = np.zeros((F, S, S), bool)
    for qy in range(ss + 2 * halo):
        for qx in range(ss + 2 * halo):
            out |= padded[:, qy:qy + N:ss, qx:qx + N:ss][:, :S, :S]
    return out
