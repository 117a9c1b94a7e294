"""The device decimation rounds (csrc/mesh_decimate_gpu.hip) give the bytes they gave before their
selection kernels were reworked for speed (one stamp per vertex, per-wave counters, per-round
candidate records, pass-tagged marks): SHA-256 of the returned vertices, faces and quadrics and the
three stats, recorded from the earlier library by tests/golden/make_decimate_rounds_parent.py, for
every mesh of the round tests, with and without the link test, after 1, 2 and all rounds.

The rounds are deterministic (test_result_does_not_depend_on_what_the_workspace_held), so equal
digests are the whole statement: same collapses, same arithmetic.

One mesh of the export's size (a million faces) is recorded too: only there do several rejections of
one round fall into one slot of the rejection table often enough for the count of rejections to
show whether a candidate the table forgot inside a round is tested again."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from drawingspinup_amd import _lib
from drawingspinup_amd.nsr import mesh as M
from tests.test_decimate_rounds_host import MESHES, decimation_meshes, round_budget

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decimate_rounds_parent.json")
GOLDEN_LARGE = os.path.join(os.path.dirname(GOLDEN), "decimate_rounds_parent_large.json")
MAX_ROUNDS = (1, 2, 200)


def run_case(dev, v, f, keep, max_rounds, workspace=None):
    """-> {"verts", "faces", "quadrics": sha256 hex, "stats": [rounds, collapses, rejected]}"""
    stop, floor = round_budget(len(f))
    out = M.decimate_parallel(torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(np.array(f)).to(dev),
                              stop, floor, 1.0, keep, max_rounds, workspace)
    gv, gf, gq, st = (t.cpu().numpy() for t in out)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return {"verts": sha(gv), "faces": sha(gf), "quadrics": sha(gq), "stats": [int(x) for x in st]}


def large_case(dev, res=768):
    """marching cubes of an analytic blob on a res^3 lattice (1.05 M faces), down to the export's
    stop / floor of 62 500 / 56 000 faces"""
    c = torch.linspace(-1, 1, res, dtype=torch.float64, device=dev)
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    vol = 0.62 - torch.sqrt((x / 0.8) ** 2 + (y / 0.6) ** 2 + (z / 0.7) ** 2) \
        + 0.05 * torch.sin(9 * x + 0.3) * torch.sin(7 * y + 1.1) * torch.sin(8 * z + 2.0)
    del x, y, z
    v, f = M.marching_cubes(vol, 0.0)
    del vol
    out = M.decimate_parallel(v / (res - 1.0), f, 62500, 56000, 1.0, True, 200)
    gv, gf, gq, st = (t.cpu().numpy() for t in out)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return {"input_faces": int(f.shape[0]), "verts": sha(gv), "faces": sha(gf), "quadrics": sha(gq),
            "stats": [int(x) for x in st]}


def case_key(name, part, keep, max_rounds):
    return "%s[%d] keep_manifold=%d max_rounds=%d" % (name, part, int(keep), max_rounds)


def workspace_cases(dev):
    """the lattice mesh with a pre-filled and with a zeroed workspace"""
    v, f = decimation_meshes("lattice")[0]
    nb = int(_lib.lib().dsu_mesh_decimate_parallel_workspace_bytes(len(v), len(f)))
    return {"lattice[0] workspace=0xAB": run_case(dev, v, f, True, 200,
                                                  torch.full((nb,), 0xAB, dtype=torch.uint8, device=dev)),
            "lattice[0] workspace=zeros": run_case(dev, v, f, True, 200,
                                                   torch.zeros(nb, dtype=torch.uint8, device=dev))}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", MESHES)
def test_rounds_give_the_recorded_bytes(dev, golden, name, keep):
    n_applied = 0
    for part, (v, f) in enumerate(decimation_meshes(name)):
        for max_rounds in MAX_ROUNDS:
            key = case_key(name, part, keep, max_rounds)
            got = run_case(dev, v, f, keep, max_rounds)
            assert got == golden["cases"][key], key
            n_applied += got["stats"][1]
    # every mesh but the tetrahedron's set applies collapses: the digests are of decimated meshes
    assert n_applied > 0


def test_recorded_bytes_do_not_depend_on_the_workspace(dev, golden):
    got = workspace_cases(dev)
    for key, want in golden["workspace"].items():
        assert got[key] == want, key
    assert got["lattice[0] workspace=0xAB"] == got["lattice[0] workspace=zeros"]
    assert got["lattice[0] workspace=zeros"] == golden["cases"][case_key("lattice", 0, True, 200)]


def test_rounds_give_the_recorded_bytes_on_a_mesh_of_the_exports_size(dev):
    with open(GOLDEN_LARGE) as fh:
        want = json.load(fh)
    got = large_case(dev)
    print("large mesh: %d faces, stats %s (recorded %s)" % (got["input_faces"], got["stats"], want["stats"]))
    assert got == want


def test_the_recorded_cases_reach_the_reworked_paths(golden):
    """what the record itself shows of the cases: every case is there, the tetrahedron rejects
    everything, and on the five larger meshes the first, the second and the later rounds each apply
    collapses"""
    c = golden["cases"]
    assert set(c) == {case_key(n, p, k, r) for n in MESHES for p in range(len(decimation_meshes(n)))
                      for k in (True, False) for r in MAX_ROUNDS}
    tet = c[case_key("tiny", 0, True, 200)]["stats"]
    assert tet[1] == 0 and tet[2] > 0
    for name in ("sphere", "bump", "lattice", "torus", "pinched"):
        one, two, full = (c[case_key(name, 0, True, r)]["stats"] for r in MAX_ROUNDS)
        assert one[0] == 1 and two[0] == 2 and full[0] > 2
        assert 0 < one[1] < two[1] < full[1]
