"""dsu_set_onewave_grid_cap counts CUs: the pipelined geometry backward (two workgroups resident
per CU at 4..6 active levels) launches 2 x cap workgroups.  Any grid must give the same gradients
up to the order of the float sums (per-workgroup partial vectors, float atomics of the scatter)."""
import pytest
import torch

from drawingspinup_amd import _lib, ops

pytestmark = pytest.mark.gpu
CFG = ops.HashGridConfig()


def test_sdf_fd_bwd_same_gradients_at_every_cap(dev):
    g = torch.Generator().manual_seed(71)
    n, active, eps, radius = 5000, 5, 0.027, 1.0
    tab = ((torch.rand(CFG.n_entries, 2, generator=g) * 2 - 1) * 0.5).half().to(dev)
    mlp = [(torch.randn(64, 23, generator=g) * 0.3).to(dev), (torch.randn(64, generator=g) * 0.05).to(dev),
           (torch.randn(13, 64, generator=g) * 0.2).to(dev), (torch.randn(13, generator=g) * 0.1).to(dev)]
    pts = (torch.rand(n, 3, generator=g) * 2 - 1).to(dev)
    d = [torch.randn(n, generator=g).to(dev), (torch.randn(n, 3, generator=g) * 0.1).to(dev),
         torch.randn(n, 13, generator=g).to(dev), (torch.randn(n, generator=g) * 1e-3).to(dev)]
    fwd = ops.sdf_fd_fwd(CFG, tab, mlp, pts, radius, eps, active, enc_cache=True)
    lib = _lib.lib()
    out = {}
    try:
        for cap in (0, 1, 3):       # 20 workgroups (one per 256 points), 2 and 6
            assert lib.dsu_set_onewave_grid_cap(cap) == 0
            gt, gm = ops.sdf_fd_bwd(CFG, tab, mlp, pts, radius, eps, active, *d, enc_cache=fwd[4])
            torch.cuda.synchronize()
            out[cap] = (gt.clone(), [m.clone() for m in gm])
    finally:
        assert lib.dsu_set_onewave_grid_cap(0) == 0
    gt0, gm0 = out[0]
    scale = float(gt0.abs().max())
    assert scale > 0
    for cap in (1, 3):
        gt1, gm1 = out[cap]
        # the bounds tests/test_gpu_hashgrid.py uses for two summation orders of the same terms
        assert float((gt0 - gt1).abs().max()) < 5e-5 * scale, cap
        for a_, b_ in zip(gm0, gm1):
            assert float((a_ - b_).abs().max()) < 1e-4 * (float(a_.abs().max()) + 1e-12), cap
