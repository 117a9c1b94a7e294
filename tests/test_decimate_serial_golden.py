"""The serial decimation queue (csrc/mesh_decimate.hip) gives the bytes it gave while it carried its
own copy of the quadric arithmetic, before that arithmetic moved into csrc/decimate_quadric.h (one
text for the queue and the device rounds): SHA-256 of the returned vertices and faces, recorded from
the earlier library by tests/golden/make_decimate_serial_parent.py, for every mesh of the round
tests, with and without the link test, down to a quarter of the faces:

  * `dsu_mesh_decimate_quadric` at boundary_weight 0 (no boundary planes);
  * `dsu_mesh_decimate_quadric` at boundary_weight 1 on the meshes WITHOUT a boundary edge: the
    queue adds its boundary planes in the hash order of an unordered_map, which is the standard
    library's and no part of a committed record;
  * `dsu_mesh_decimate_quadric_q` seeded with the initial quadrics of the definition at weight 1
    (oracle/decimate_rounds_ref.py): a seeded call adds no planes of its own.

The queue is deterministic, so equal digests are the whole statement: same collapses, same
arithmetic."""
import hashlib
import json
import os

import numpy as np
import pytest

from drawingspinup_amd.nsr import mesh as M
from oracle import decimate_rounds_ref as R
from tests.test_decimate_rounds_host import MESHES, decimation_meshes
from tests.test_export_host import _edge_counts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decimate_serial_parent.json")
MODES = ("unseeded bw=0", "unseeded bw=1", "seeded bw=1")


def has_boundary(f):
    return bool((_edge_counts(f)[1] == 1).any())


def case_key(name, part, keep, mode):
    return "%s[%d] keep_manifold=%d %s" % (name, part, int(keep), mode)


def all_cases():
    """-> [(name, part, keep, mode)] in the order of the record"""
    return [(name, part, keep, mode) for name in MESHES for part, (v, f) in enumerate(decimation_meshes(name))
            for keep in (True, False) for mode in MODES if mode != "unseeded bw=1" or not has_boundary(f)]


def run_case(name, part, keep, mode):
    """-> {"verts", "faces": sha256 hex, "n_faces"}"""
    v, f = decimation_meshes(name)[part]
    v = np.ascontiguousarray(v)
    f32 = np.ascontiguousarray(f.astype(np.int32))
    quadrics = np.ascontiguousarray(R.init_quadrics(v, f, 1.0)[0]) if mode == "seeded bw=1" else None
    gv, gf = M._remesh_host(v, f32, len(f) // 4, 0.0 if mode == "unseeded bw=0" else 1.0, keep, quadrics=quadrics)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return {"verts": sha(gv), "faces": sha(gf), "n_faces": int(len(gf))}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", MESHES)
def test_queue_gives_the_recorded_bytes(golden, name, keep):
    n_removed = 0
    for n, part, k, mode in all_cases():
        if n != name or k != keep:
            continue
        key = case_key(n, part, k, mode)
        got = run_case(n, part, k, mode)
        assert got == golden["cases"][key], key
        n_removed += len(decimation_meshes(n)[part][1]) - got["n_faces"]
    # every set of meshes loses faces somewhere: the digests are of decimated meshes
    assert n_removed > 0


def test_the_record_holds_the_cases_and_no_open_mesh_at_weight_one(golden):
    assert golden["case_list"] == [case_key(*c) for c in all_cases()]
    assert set(golden["cases"]) == set(golden["case_list"])
    for name in MESHES:
        for part, (v, f) in enumerate(decimation_meshes(name)):
            for keep in (True, False):
                assert (case_key(name, part, keep, "unseeded bw=1") in golden["cases"]) == (not has_boundary(f))
                assert case_key(name, part, keep, "unseeded bw=0") in golden["cases"]
                assert case_key(name, part, keep, "seeded bw=1") in golden["cases"]
    # both kinds of mesh are there: closed ones at weight 1, open ones left out
    closed = {n for n in MESHES for _, f in decimation_meshes(n) if not has_boundary(f)}
    assert {"sphere", "lattice", "torus"} <= closed and "bump" not in closed
