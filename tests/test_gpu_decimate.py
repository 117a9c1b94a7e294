"""Device rounds of the quadric decimation (csrc/mesh_decimate_gpu.hip, nsr.mesh.remesh on device
tensors) held to the contracts the serial host queue is held to in tests/test_export_host.py: exact
face count, closed 2-manifold of the same genus, orientation, vertices on the input surface, faces
spent where the surface bends, boundary outline kept, deterministic — plus an export-scale mesh
(marching cubes of a 384^3 volume, ~0.8 M triangles) with the time of the call."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from drawingspinup_amd import _lib
from drawingspinup_amd.nsr import mesh as M
from oracle import decimate_rounds_ref as R
from tests.test_decimate_rounds_host import (FRAGILE_CAP, MESHES, compact, decimation_meshes, round_budget,
                                             seeded_finish_matches_the_oracle)
from tests.test_export_host import _edge_counts, _grid, _signed_volume, _uv_sphere

pytestmark = pytest.mark.gpu


def _dev(v, f, dev):
    return torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)


def test_parallel_remesh_sphere_contract(dev):
    v, f = _uv_sphere(320, 240)                                       # 153 k triangles
    v2, f2 = M.remesh(*_dev(v, f, dev), 3000)
    st = dict(M.last_remesh_stats)
    assert st["input_faces"] == len(f) and 3000 <= st["device_faces"] <= 12000 and st["rounds"] >= 5
    assert f2.shape == (3000, 3) and f2.dtype == np.int64 and v2.dtype == np.float64
    assert f2.min() == 0 and f2.max() == v2.shape[0] - 1 and len(np.unique(f2)) == v2.shape[0]
    u, c = _edge_counts(f2)
    assert np.all(c == 2)                                             # closed 2-manifold ...
    assert v2.shape[0] - u.shape[0] + f2.shape[0] == 2                # ... of genus 0
    d = np.concatenate([f2[:, [0, 1]], f2[:, [1, 2]], f2[:, [2, 0]]])
    assert len(np.unique(d, axis=0)) == len(d)                        # consistent orientation
    n = np.cross(v2[f2[:, 1]] - v2[f2[:, 0]], v2[f2[:, 2]] - v2[f2[:, 0]])
    assert np.all(np.einsum("ij,ij->i", n, v2[f2].mean(1)) > 0)       # outward, none flipped
    r = np.linalg.norm(v2, axis=1)
    assert abs(r - 0.5).max() < 1e-3                                  # within 0.2 % of the radius
    assert abs(_signed_volume(v2, f2) / _signed_volume(v, f) - 1) < 5e-3
    v3, f3 = M.remesh(*_dev(v, f, dev), 3000)                         # deterministic
    assert np.array_equal(v2, v3) and np.array_equal(f2, f3)
    # the serial queue alone from the same input: same quality class (volume, radius), not the
    # same mesh (the collapse order differs)
    hv, hf = M.remesh(v, f, 3000)
    assert abs(np.linalg.norm(hv, axis=1) - 0.5).max() < 1e-3
    print("sphere: device stats", st, "radius error device %.2e host %.2e"
          % (abs(r - 0.5).max(), abs(np.linalg.norm(hv, axis=1) - 0.5).max()))


def test_parallel_remesh_spends_faces_where_the_surface_bends(dev):
    bump = lambda x, y: 0.2 * np.exp(-(x * x + y * y) / (2 * 0.05 ** 2))
    v, f = _grid(301, bump)                                           # 180 k triangles, open surface
    v2, f2 = M.remesh(*_dev(v, f, dev), 1500)
    assert f2.shape[0] in (1499, 1500)
    assert np.abs(v2[:, 2] - bump(v2[:, 0], v2[:, 1])).max() < 4e-3
    rad = np.linalg.norm(v2[f2].mean(1)[:, :2], axis=1)
    assert (rad < 0.15).sum() > (rad >= 0.15).sum()
    assert np.allclose(v2[:, :2].min(0), -0.5, atol=1e-6) and np.allclose(v2[:, :2].max(0), 0.5, atol=1e-6)
    a = v2[f2]
    p, q = a[:, 1, :2] - a[:, 0, :2], a[:, 2, :2] - a[:, 0, :2]
    assert abs(0.5 * np.abs(p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]).sum() - 1.0) < 1e-3
    u, c = _edge_counts(f2)
    assert set(np.unique(c)) <= {1, 2}


def test_parallel_remesh_at_export_scale(dev):
    """A marching-cubes mesh of the size class the export produces (a blobby shape on a 384^3
    lattice), down to the reference's face_count = 50 000."""
    n = 384
    c = torch.linspace(-1, 1, n, device=dev)
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    vol = 0.9 - torch.sqrt((x / 0.95) ** 2 + (y / 0.8) ** 2 + (z / 0.9) ** 2) \
        + 0.08 * torch.sin(9 * x) * torch.sin(7 * y + 1) * torch.sin(8 * z + 2)
    v, f = M.marching_cubes(vol.double(), 0.0)
    assert f.shape[0] > 600000
    torch.cuda.synchronize()
    t0 = time.time()
    v2, f2 = M.remesh(v, f, 50000)
    dt = time.time() - t0
    st = dict(M.last_remesh_stats)
    print("export scale: %d -> %d faces in %.3f s; device stats %s" % (f.shape[0], f2.shape[0], dt, st))
    assert f2.shape[0] in (49999, 50000)
    u, cnt = _edge_counts(f2)
    assert np.all(cnt == 2)                                           # closed manifold kept
    vin, fin = v.cpu().numpy(), f.cpu().numpy()
    chi_in = vin.shape[0] - _edge_counts(fin)[0].shape[0] + fin.shape[0]
    assert v2.shape[0] - u.shape[0] + f2.shape[0] == chi_in           # same Euler characteristic
    assert abs(_signed_volume(v2, f2) / _signed_volume(vin, fin) - 1) < 2e-3
    # every output vertex lies on the input iso-surface to a fraction of a lattice cell
    pts = torch.from_numpy(v2).to(dev).float()
    g = (pts / (n - 1.0) * 2 - 1)[None, None, None][..., [2, 1, 0]]
    val = torch.nn.functional.grid_sample(vol[None, None], g, mode="bilinear", align_corners=True).flatten()
    grad = 0.5 * (n - 1) / 2                                          # |d vol / d lattice unit| ~ 1/128 .. : bound below
    assert float(val.abs().max()) < 0.02
    assert dt < 2.0


# ------------------------------------------------------------------------------------------------
# The rounds themselves, collapse by collapse, against oracle/decimate_rounds_ref.py: the initial
# quadrics entry by entry, every round held to the rule set (check_round recovers the collapses
# from the mesh before and after; which admissible independent subset the device took is free),
# the small-mesh paths remesh never routes to the device, and the hand-over to the seeded queue.
# ------------------------------------------------------------------------------------------------
EINVAL = -1


def _rounds(v, f, dev, stop, floor, bw=1.0, keep=True, max_rounds=200, workspace=None):
    out = M.decimate_parallel(torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(np.array(f)).to(dev),
                              stop, floor, bw, keep, max_rounds, workspace)
    return tuple(t.cpu().numpy() for t in out)


def _chi(f):
    return len(np.unique(f)) - len(_edge_counts(f)[0]) + len(f) if len(f) else 0


@pytest.mark.parametrize("name", MESHES)
def test_initial_quadrics_match_the_definition(dev, name):
    worst = 0.0
    for v, f in decimation_meshes(name):
        a, b, c = int(f[0, 0]), int(f[0, 1]), int(f[-1, 2])
        n = len(v)
        v2 = np.concatenate([v, v[a][None], v[a][None]])               # two more vertices on top of `a`
        f2 = np.concatenate([f[:len(f) // 2], [[a, a, b]], f[len(f) // 2:], [[c, c, c]], [[a, n, n + 1]]])
        live = np.concatenate([f, [[a, n, n + 1]]])                     # degenerate rows dropped, order kept
        for bw in (0.0, 1.0):
            want, bound, need = R.init_quadrics_bound(v2, f2, bw)
            for stop, max_rounds in ((0, 0), (len(f2), 200)):            # no round allowed / none needed
                gv, gf, gq, st = _rounds(v2, f2, dev, stop, 0, bw, True, max_rounds)
                assert st.tolist() == [0, 0, 0]
                assert np.array_equal(gf, live) and gf.dtype == np.int32
                assert np.array_equal(gv.view(np.int64), v2.view(np.int64))
                ratio = float((np.abs(gq - want) / np.maximum(bound, 1e-300)).max())
                worst = max(worst, ratio * max(1.0, 4 * need))
                assert ratio <= 1.0, (name, bw, ratio)
    print("initial quadrics %s: largest error / (16 eps sum|terms|) = %.3f" % (name, worst))


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", MESHES)
def test_every_round_keeps_the_rules(dev, name, keep):
    n_collapses = n_fragile = n_checked = n_reported = 0
    worst = 0.0
    ranks = []
    for v, f in decimation_meshes(name):
        stop, floor = round_budget(len(f))
        full = _rounds(v, f, dev, stop, floor, 1.0, keep)
        K = min(int(full[3][0]), 8)
        n_reported += int(full[3][0])
        state = _rounds(v, f, dev, stop, floor, 1.0, keep, 0)
        want, bound, _ = R.init_quadrics_bound(v, f, 1.0)
        assert np.all(np.abs(state[2] - want) <= bound)
        manifold = name != "pinched" and set(R.edge_multiplicity(f)) <= {1, 2}
        applied = 0
        for k in range(1, K + 1):
            nxt = _rounds(v, f, dev, stop, floor, 1.0, keep, k)
            assert int(nxt[3][0]) == k
            if R.has_twin_faces(state[1]):                               # see has_twin_faces: not recoverable
                break
            cs, nfr = R.check_round(*state[:3], *nxt[:3], floor_faces=floor, keep_manifold=keep,
                                    remembered=int(state[3][2]))
            applied += len(cs)
            n_checked += 1
            ranks.append("%d/%d" % R.candidacy_rank(state[1], floor, int(state[3][2])))
            assert int(nxt[3][1]) == applied
            if manifold and keep:               # the link test is what keeps a manifold one (without it a
                assert set(R.edge_multiplicity(nxt[1])) <= {1, 2}     # pocket may fold flat: edges with 4 faces);
                assert _chi(nxt[1]) == _chi(f)                         # `pinched`: its fan may fold away whole
            n_collapses += len(cs)
            n_fragile += nfr
            worst = max([worst] + [c.ratio for c in cs])
            state = nxt
        if K == int(full[3][0]) and not R.has_twin_faces(state[1]):
            assert np.array_equal(state[1], full[1]) and np.array_equal(state[3], full[3])
    print("rounds %s keep_manifold=%s: %d of %d rounds checked, %d collapses, %d fragile, largest target error / "
          "bound = %.3g, candidacy rank / edges per round: %s"
          % (name, keep, n_checked, n_reported, n_collapses, n_fragile, worst, " ".join(ranks)))
    assert n_fragile <= FRAGILE_CAP * n_collapses


def test_a_tetrahedron_with_the_link_test_rejects_everything(dev):
    v, f = decimation_meshes("tiny")[0]
    gv, gf, gq, st = _rounds(v, f, dev, 2, 0, 1.0, True)
    assert st[0] == 4 and st[1] == 0 and st[2] > 0                       # four stalled rounds, then it gives up
    assert np.array_equal(gf, f) and np.array_equal(gv.view(np.int64), v.view(np.int64))


def _raw(dev, v, f, stop, floor, bw=1.0, flags=0, max_rounds=200, ws_short=0, null_out=False):
    lib = _lib.lib()
    tv = torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(f, np.int32).reshape(-1, 3)).to(dev)
    nb = int(lib.dsu_mesh_decimate_parallel_workspace_bytes(len(v), len(tf)))
    ws = torch.empty(max(nb - ws_short, 1), dtype=torch.uint8, device=dev)
    q = torch.empty(max(len(v), 1), 10, dtype=torch.float64, device=dev)
    out_nf, stats = C.c_int64(-7), (C.c_int32 * 3)(-7, -7, -7)
    rc = lib.dsu_mesh_decimate_parallel(tv.data_ptr(), len(v), tf.data_ptr(), len(tf), stop, floor, bw, flags, max_rounds,
                                        q.data_ptr(), None if null_out else C.byref(out_nf), stats, ws.data_ptr(),
                                        nb - ws_short, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc, out_nf.value, list(stats), tv.cpu().numpy(), tf.cpu().numpy()


def test_all_degenerate_and_empty_meshes(dev):
    v = decimation_meshes("tiny")[0][0]
    rc, nf, st, _, _ = _raw(dev, v, [[0, 0, 1], [2, 2, 2], [3, 1, 3]], 0, 0)
    assert rc == 0 and nf == 0 and st == [0, 0, 0]
    rc, nf, st, _, _ = _raw(dev, v, np.zeros((0, 3)), 0, 0)
    assert rc == 0 and nf == 0 and st == [0, 0, 0]
    rc, nf, st, _, _ = _raw(dev, np.zeros((0, 3)), np.zeros((0, 3)), 0, 0)
    assert rc == 0 and nf == 0 and st == [0, 0, 0]


def test_parallel_argument_validation_returns_before_any_launch(dev):
    v, f = decimation_meshes("tiny")[1]
    ok = _raw(dev, v, f, 4, 2)
    assert ok[0] == 0
    for kw in (dict(ws_short=1), dict(stop=1, floor=2), dict(max_rounds=-1), dict(bw=float("nan")),
               dict(bw=-1.0), dict(floor=-1), dict(null_out=True)):
        a = dict(stop=4, floor=2)
        a.update(kw)
        rc, nf, st, gv, gf = _raw(dev, v, f, **a)
        assert rc == EINVAL, kw
        assert np.array_equal(gv, v) and np.array_equal(gf, f), kw       # nothing ran


@pytest.mark.parametrize("name", ["sphere", "lattice"])
def test_result_does_not_depend_on_what_the_workspace_held(dev, name):
    v, f = decimation_meshes(name)[0]
    stop, floor = round_budget(len(f))
    nb = int(_lib.lib().dsu_mesh_decimate_parallel_workspace_bytes(len(v), len(f)))
    a = _rounds(v, f, dev, stop, floor, workspace=torch.full((nb,), 0xAB, dtype=torch.uint8, device=dev))
    b = _rounds(v, f, dev, stop, floor, workspace=torch.zeros(nb, dtype=torch.uint8, device=dev))
    assert a[3][1] > 0
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", ["sphere", "bump"])
def test_hand_over_to_the_seeded_queue(dev, name):
    """what remesh does after the rounds: compact, then dsu_mesh_decimate_quadric_q with the
    accumulated quadrics — against the naive restatement started from the same arrays"""
    v, f = decimation_meshes(name)[0]
    target = 300
    gv, gf, gq, st = _rounds(v, f, dev, int(1.25 * target), target)
    assert target <= len(gf) < len(f) and st[1] > 0
    print("hand-over %s: %d faces after %d rounds" % (name, len(gf), st[0]))
    for keep in (True, False):
        assert seeded_finish_matches_the_oracle(*compact(gv, gf.astype(np.int64), gq), target, keep) <= target
