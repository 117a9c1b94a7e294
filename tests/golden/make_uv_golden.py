"""Fixture for the UV bake (the export_uv branch): runs the REFERENCE's own
`compute_interpolation_map` (2_charactor_reconstructor/instant_nsr/utils/coloring_utils.py:140-148;
scipy's griddata and PIL are the real ones) at shape (128, 128) on the uvs that
drawingspinup_amd.nsr.uv.parametrize gives for the capsule character and the helicoid.

    python tests/golden/make_uv_golden.py     # needs /root/reference

The colours are an AFFINE function of uv, A uv + b inside [0, 1]: the reference interpolates over
the Delaunay triangulation of the uv points, not over the mesh's triangles, and only affine data
does not depend on the triangulation.  Comparison rule (tests/test_uv_host.py,
check_against_reference_fixture): equality on every texel whose sample lies strictly inside a
face, one level only where colour * 255 is within 1e-6 of an integer, on at most 0.5 % of the
compared texels — asserted here on the reference against tests/uv_ref.py before the file is kept.
This fixture is what pins the texel and flip convention to the reference."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
SIZE = 128


def main():
    import make_mesh_color_golden as G
    import types
    from oracle import mesh_post_ref as P
    G.stub("cv2", MORPH_ELLIPSE=P.MORPH_ELLIPSE, getStructuringElement=P.getStructuringElement,
           erode=P.erode, dilate=P.dilate, flip=P.flip)
    G.stub("trimesh")
    G.stub("mesh_raycast", raycast=P.raycast)
    G.stub("pytorch3d")
    G.stub("pytorch3d.structures", Meshes=object)
    G.stub("pytorch3d.renderer", RasterizationSettings=lambda **k: None, MeshRasterizer=lambda **k: None)
    G.stub("pytorch3d.renderer.cameras", look_at_view_transform=lambda *a: (None, None),
           OrthographicCameras=lambda **k: None)
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_coloring_utils", os.path.join(G.UTILS, "coloring_utils.py"))
    cu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cu)

    import uv_ref as R
    from drawingspinup_amd.nsr import uv as U
    rng = np.random.default_rng(7)
    out = {}
    for name in ("character", "helicoid"):
        verts, faces = R.meshes()[name]
        vm, ind, uvs = U.parametrize(verts, faces, SIZE, 2, backend=R.RefBackend())
        A = rng.uniform(-0.4, 0.4, (3, 2))
        lo = np.minimum(A, 0).sum(1)
        hi = np.maximum(A, 0).sum(1)
        b = 0.05 - lo + rng.uniform(0, 1, 3) * (0.9 - (hi - lo))
        col = (uvs.astype(np.float64) @ A.T + b).astype(np.float32)
        assert col.min() >= 0 and col.max() <= 1
        img = np.array(cu.compute_interpolation_map(uvs, col, shape=(SIZE, SIZE)))
        out.update({f"{name}_uvs": uvs, f"{name}_indices": ind.astype(np.int32), f"{name}_colours": col,
                    f"{name}_image": img, f"{name}_A": A, f"{name}_b": b})
    path = os.path.join(HERE, "uv_reference.npz")
    np.savez_compressed(path, **out)
    import test_uv_host as T
    try:
        rep = T.check_against_reference_fixture(lambda u, i, c, s: R.bake(u, i, c, s)[:2])
    except AssertionError:
        os.remove(path)
        raise
    print("wrote uv_reference.npz", os.path.getsize(path), "bytes; (compared, excused) per mesh:", rep)


if __name__ == "__main__":
    main()
