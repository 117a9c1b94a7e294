"""Corrective smoothing of skinned frames ("delta mush", Mancewicz et al. 2014; Blender's Corrective
Smooth modifier): the host side, once per character.  The rule and its kernels are stated in
include/dsu_hip.h ("Corrective smoothing") and run through ops.corrective_bind /
ops.corrective_smooth; here the mesh graph they walk is built.

Everything runs on the WELDED mesh (nsr/thinning._weld, the rule bone_heat_weights uses): a
seam-split textured export (read_obj_textured) has coincident vertices along its seams, and smoothing
its raw graph would tear it there.
"""
import numpy as np

from ..nsr.thinning import _weld

MAX_ITERATIONS = 255


def check_parameters(iterations, factor):
    """0 <= iterations <= 255 (0: off), 0 <= factor <= 1; ValueError otherwise."""
    if int(iterations) != iterations or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"corrective iterations {iterations!r}: an integer in 0..{MAX_ITERATIONS}")
    if not 0.0 <= factor <= 1.0:
        raise ValueError(f"corrective factor {factor!r}: a number in [0, 1]")


def _csr(rows, cols, n, width):
    """(rows, cols) pairs, cols < width -> (rowptr (n+1) int32, cols int32): ascending and duplicate-free
    per row (one sort of the combined key row * width + col)."""
    key = np.unique(np.asarray(rows, np.int64) * width + np.asarray(cols, np.int64))
    rows, cols = key // width, key % width
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr.astype(np.int32), cols.astype(np.int32)


def smoothing_topology(verts, faces):
    """The graph of the welded mesh: verts (V,3), faces (M,3) 0-based -> a dictionary of numpy int32
    arrays
      rep (V,)                        the lowest index of each cluster of coincident vertices
      faces (G,3)                     the faces over representatives, degenerate ones dropped
      nbr_rowptr (V+1,), nbr_cols     CSR: the row of a representative lists, ascending and without
                                      duplicates, the other representatives it shares a face with;
                                      the row of a non-representative or of a vertex without a face
                                      is empty
      cor_rowptr (V+1,), cor_faces    CSR: the ascending indices into `faces` of the faces that
                                      contain the representative"""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = len(v)
    if n > 2 ** 30 or len(f) > 2 ** 30:
        raise ValueError("mesh too large")
    rep, g = _weld(v, f)
    g = np.asarray(g, np.int64).reshape(-1, 3)
    a, b, c = g[:, 0], g[:, 1], g[:, 2]
    nbr_rowptr, nbr_cols = _csr(np.concatenate([a, b, b, c, c, a]), np.concatenate([b, a, c, b, a, c]), n, max(n, 1))
    cor_rowptr, cor_faces = _csr(g.ravel(), np.repeat(np.arange(len(g), dtype=np.int64), 3), n, max(len(g), 1))
    return {"rep": np.asarray(rep, np.int64).astype(np.int32), "faces": np.ascontiguousarray(g, np.int32),
            "nbr_rowptr": nbr_rowptr, "nbr_cols": nbr_cols, "cor_rowptr": cor_rowptr, "cor_faces": cor_faces}
