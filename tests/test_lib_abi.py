"""CPU: the C-ABI library loads and exports every symbol include/dsu_hip.h declares (no
compute calls: there is no GPU here), the binding derived from that header is complete, strict and
laid out as the host compiler lays it out, and the product path fails loudly without a device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "dsu_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dsu_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from drawingspinup_amd import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(h, n), f"{n} declared in include/dsu_hip.h but not exported"
    # and the ctypes prototype table covers the header (a new function cannot be forgotten)
    missing = [n for n in names if n not in _lib._PROTOS and n != "dsu_strerror"]
    assert not missing, missing
    # ... and names nothing the header does not declare (a removed function cannot linger)
    undeclared = [n for n in _lib._PROTOS if n not in names]
    assert not undeclared, undeclared
    lib = _lib.lib()
    assert lib.dsu_abi_version() == _lib.ABI_VERSION
    assert lib.dsu_strerror(-1).decode() == "invalid argument"


def test_loader_refuses_a_library_of_another_abi_version(monkeypatch):
    """A stale libdsu_hip.so under a newer prototype table would take arguments in the wrong places."""
    from drawingspinup_amd import _lib
    _lib.lib()
    monkeypatch.setattr(_lib, "_lib", None)                 # the cached handle; both restored afterwards
    monkeypatch.setattr(_lib, "ABI_VERSION", _lib.ABI_VERSION + 1)
    built, bound = _lib.ABI_VERSION - 1, _lib.ABI_VERSION
    with pytest.raises(_lib.DsuError, match=rf"version {built}\b.*version {bound}\b.*rebuild") as e:
        _lib.lib()
    assert _lib.LIB_PATH in str(e.value) and _lib._lib is None


def test_host_only_entry_point_matches_oracle():
    from drawingspinup_amd import ops
    from oracle import hashgrid as oh
    for kw in (dict(), dict(n_levels=12), dict(n_levels=16, base_resolution=16, per_level_scale=1.5)):
        cfg = ops.HashGridConfig(**kw)
        lv = cfg.levels()
        ref = oh.make_levels(cfg.n_levels, cfg.log2_hashmap_size, cfg.base_resolution,
                             cfg.per_level_scale)
        assert lv["offsets"] == ref["offsets"] and lv["resolution"] == ref["resolution"]
        assert lv["hashed"] == ref["hashed"] and lv["scale"] == [float(s) for s in ref["scale"]]


def test_argument_validation_without_gpu():
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    cfg = _lib.HashGridCfg(10, 3, 19, 32, 1.3195079107728942)          # 3 features: unsupported
    lv = _lib.HashGridLevels()
    assert lib.dsu_hashgrid_make_levels(ctypes.byref(cfg), ctypes.byref(lv)) == -3
    cfg = _lib.HashGridCfg(0, 2, 19, 32, 1.3)
    assert lib.dsu_hashgrid_make_levels(ctypes.byref(cfg), ctypes.byref(lv)) == -1
    # NULL pointers are rejected before any launch
    cfg = _lib.HashGridCfg(10, 2, 19, 32, 1.3195079107728942)
    assert lib.dsu_hashgrid_encode_fwd(ctypes.byref(cfg), None, None, 5, 4, None, None) == -1
    assert lib.dsu_ric_offsets(0, 4, None, None) == -1


def test_process_wide_knobs_validate_their_ranges():
    """include/dsu_hip.h: the grid caps of the NSR step's kernels and the priority of the step driver's side stream
    (1 high = the default, 2 normal, 0 low) — all restored to their defaults here."""
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    assert lib.dsu_set_onewave_grid_cap(257) == -1 and lib.dsu_set_onewave_grid_cap(-1) == -1
    assert lib.dsu_set_onewave_grid_cap(192) == 0 and lib.dsu_set_onewave_grid_cap(0) == 0
    assert lib.dsu_set_scatter_grid_cap(4097) == -1 and lib.dsu_set_scatter_grid_cap(0) == 0
    for level, rc in ((-1, -1), (3, -1), (0, 0), (2, 0), (1, 0)):
        assert lib.dsu_set_nsr_side_stream_priority(level) == rc, level
    assert lib.dsu_set_nsr_side_stream_pooling(2) == -1 and lib.dsu_set_nsr_side_stream_pooling(1) == 0
    assert lib.dsu_set_nsr_side_stream_pooling(0) == 0


def test_style_training_host_side_sizes():
    """Host-only planning of the training kernels: workspace of the sliced weight gradient and
    the sampling-table size; argument checks return before any launch."""
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    assert lib.dsu_deform_tap_table_bytes(32, 32) == 32 * 32 * 9 * 32
    assert lib.dsu_deform_tap_table_bytes(0, 32) == 0
    # resnet level of the shipped config: 40 x 128 x 8 x 8, 128 -> 128 deformable: 19 column
    # tiles of 7 channels, 20 chunks of 128 pixels -> 10 slices of 2 chunks
    per_slice = 128 * 128 * 9 * 4
    assert lib.dsu_conv2d_wgrad_workspace_bytes(1, 40, 128, 128, 8, 8, 3) == 10 * per_slice
    # upconv1 (192 -> 128 at 32x32): 28 tiles -> 18 slices = 504 workgroups, two full rounds
    assert lib.dsu_conv2d_wgrad_workspace_bytes(1, 40, 192, 128, 32, 32, 3) == \
        18 * 128 * 192 * 9 * 4
    # plain 7x7: flattened (channel, tap) columns in tiles of 64
    n = lib.dsu_conv2d_wgrad_workspace_bytes(0, 40, 166, 64, 32, 32, 7)
    assert n > 0 and n % (64 * 166 * 49 * 4) == 0
    assert lib.dsu_conv2d_wgrad_workspace_bytes(0, 0, 3, 3, 8, 8, 3) == 0
    assert lib.dsu_conv2d_wgrad(None, None, None, 1, 1, 8, 8, 1, 3, 1, 1, None, None, 0, None) == -1
    cfg = _lib.NormCfg(4, 8, 64, 0, 7, 1, 1e-5, 0.1)                     # act 7: invalid
    assert lib.dsu_norm_train_fwd(ctypes.byref(cfg), None, None, None, None, None, None, None,
                                  None, None) == -1
    assert lib.dsu_maxpool2_fwd(None, None, 1, 8, 8, None) == -1
    assert lib.dsu_pair_loss(None, None, 0.0, 4, 0, 1.0, None, None, None) == -1


def test_variant_library_override(tmp_path):
    """DSU_HIP_LIB points a process at a variant library (A/B measurements of kernel builds)."""
    import shutil
    import subprocess
    import sys
    from drawingspinup_amd import _lib
    alt = tmp_path / "libdsu_hip_alt.so"
    shutil.copy(_lib.LIB_PATH, alt)
    code = ("from drawingspinup_amd import _lib; assert _lib.lib().dsu_abi_version() == _lib.ABI_VERSION; "
            "print(_lib.LIB_PATH)")
    env = dict(os.environ, DSU_HIP_LIB=str(alt), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().endswith("libdsu_hip_alt.so")
    env["DSU_HIP_LIB"] = str(tmp_path / "missing.so")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert out.returncode != 0 and "missing" in out.stderr       # fails loudly, no fallback


def test_no_cpu_fallback():
    from drawingspinup_amd import ops, _lib
    cfg = ops.HashGridConfig()
    with pytest.raises(_lib.DsuError):
        ops.hashgrid_encode_fwd(cfg, torch.zeros(cfg.n_entries, 2, dtype=torch.float16),
                                torch.zeros(4, 3), 4)
    with pytest.raises(_lib.DsuError):
        ops.conv2d(torch.zeros(1, 3, 8, 8), torch.zeros(4, 3, 3, 3))


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under drawingspinup_amd/ may import it."""
    pkg = os.path.join(ROOT, "drawingspinup_amd")
    bad = []
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M):
                    bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_round2_entry_points_validate_before_launching():
    """Host-side planning and argument checks of the round-2 entry points (no GPU here: every call
    must return before a launch)."""
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    # Morton sort: counters (8^bits) + block sums + keys / ranks
    assert lib.dsu_spatial_sort_workspace_bytes(1000, 6) == (262144 + 256 + 2 * 1000) * 4
    assert lib.dsu_spatial_sort_workspace_bytes(0, 4) == (4096 + 4) * 4
    assert lib.dsu_spatial_sort_workspace_bytes(10, 3) == -1 and lib.dsu_spatial_sort_workspace_bytes(10, 8) == -1
    assert lib.dsu_spatial_sort(None, 5, 1.0, 6, None, None, None, 0, None) == -1
    assert lib.dsu_spatial_sort(None, 0, 1.0, 6, None, None, None, 0, None) == 0          # empty: nothing to do
    assert lib.dsu_spatial_sort_dev(None, 5, None, 0, 1.0, 6, None, None, None, 0, None) == -1
    assert lib.dsu_points_tail(None, 0, None, None, None, 0, 0.01, None) == -1
    # optimizers
    assert lib.dsu_table_adamw(None, None, None, None, None, 6, 1e-3, 0.9, 0.99, 1e-15, 0.01, 0.1, 0.1, None) == -1  # n % 4
    assert lib.dsu_table_adamw(None, None, None, None, None, 0, 1e-3, 0.9, 0.99, 1e-15, 0.01, 0.1, 0.1, None) == 0
    assert lib.dsu_table_decay(None, None, 8, 0.5, None) == -1
    assert lib.dsu_adamw_multi(None, 3, 0.9, 0.99, 1e-15, 0.01, None) == -1
    assert lib.dsu_adamw_multi(None, 0, 0.9, 0.99, 1e-15, 0.01, None) == 0
    assert lib.dsu_adamw_multi(None, _lib.ADAMW_MAX_TENSORS + 1, 0.9, 0.99, 1e-15, 0.01, None) == -1
    # export smoothing
    assert lib.dsu_smooth_energy_partials() == 1024
    assert lib.dsu_smooth_iterate(None, 5, None, None, 0.5, 10, None, None, None) == -1
    assert lib.dsu_smooth_iterate(None, 0, None, None, 0.5, 10, None, None, None) == 0
    # TELEA: host function, runs here
    import numpy as np
    img = np.full((5, 6, 3), 9, np.uint8)
    out = np.zeros_like(img)
    m = np.zeros((5, 6), np.uint8)
    m[2, 3] = 1
    P = ctypes.c_void_p
    assert lib.dsu_inpaint_telea_u8c3(P(img.ctypes.data), P(m.ctypes.data), 5, 6, 3, P(out.ctypes.data)) == 0
    # a one-pixel hole in a constant image: Ia / s + 0.5 = 9.5, rounded to even = 10 (OpenCV's
    # formula adds 0.5 AND rounds); everything else untouched
    assert out[2, 3].tolist() == [10, 10, 10]
    out[2, 3] = 9
    assert (out == 9).all()
    assert lib.dsu_inpaint_telea_u8c3(P(img.ctypes.data), P(m.ctypes.data), 2, 6, 3, P(out.ctypes.data)) == -3


def test_texture_partial_map_is_a_bijection_onto_the_gradient_block():
    """Host-only: every parameter of the texture MLP receives exactly one element of the partial
    vector, the padding elements none."""
    import numpy as np
    from drawingspinup_amd import ops
    m = ops.texture_partial_map()
    n_tex = 64 * 16 + 64 + 64 * 64 + 64 + 3 * 64 + 3
    dst = m[m >= 0]
    assert dst.size == n_tex and np.array_equal(np.sort(dst), np.arange(n_tex))
    assert (m < 0).sum() == m.size - n_tex


def test_occgrid_refresh_host_side():
    """Workspace planning and argument checks of the native occupancy refresh (no launch)."""
    import ctypes as C
    from drawingspinup_amd import _lib
    lib = _lib.lib()
    n = 128 ** 3
    need = lib.dsu_occgrid_refresh_workspace_bytes(128)
    # iota + occupied + cells (int32), points (3 f32) + sdf (f32): 7 words per cell at least
    assert 7 * 4 * n <= need < 9 * 4 * n
    assert lib.dsu_occgrid_refresh_workspace_bytes(0) == -1
    assert lib.dsu_occgrid_refresh_workspace_bytes(2048) == -1          # 2^33 cells
    a = _lib.OccRefreshArgs()
    assert lib.dsu_occgrid_refresh(C.byref(a), None) == -1              # NULL pointers
    assert lib.dsu_occgrid_refresh(None, None) == -1
    assert lib.dsu_nsr_driver_occ_refresh(None, C.byref(a), None) == -1


# ------------------------------------------------------------------ the binding is derived from the header
def test_reader_returns_every_declared_function():
    """The strict reader against this file's own regex scan: a declaration it dropped silently would
    leave the function without argument types."""
    from drawingspinup_amd import _header, _lib
    h = _header.read()
    assert sorted(h.protos) == _declared() and len(h.protos) >= 166
    assert set(_lib._PROTOS) == set(h.protos)
    assert all(_lib._PROTOS[n] is args for n, (_, args) in _lib._HEADER.protos.items())
    assert sorted(_lib._STRUCT_NAMES) == sorted(h.structs) and len(h.structs) == 12
    for c_name, py_name in _lib._STRUCT_NAMES.items():
        cls = getattr(_lib, py_name)
        assert cls is _lib._HEADER.structs[c_name] and cls.__name__ == py_name
    assert h.opaque == {"dsu_nsr_driver"}
    assert _lib.ABI_VERSION == h.defines["DSU_ABI_VERSION"] == 3
    assert _lib.MAX_LEVELS == h.defines["DSU_MAX_LEVELS"]
    assert _lib.ADAMW_MAX_TENSORS == h.defines["DSU_ADAMW_MAX_TENSORS"]


def test_header_missing_is_an_error(tmp_path):
    from drawingspinup_amd import _header
    with pytest.raises(_header.DsuError, match=r"dsu_hip\.h is missing"):
        _header.read(str(tmp_path / "include" / "dsu_hip.h"))


_WELL_FORMED = """
/* every accepted form */
#ifndef DSU_X_H
#define DSU_X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define DSU_N 4
#define DSU_NEG (-2)   /* trailing comment */
typedef struct { uint32_t a; double b; } dsu_a;   // line comment
typedef struct dsu_b {
  int32_t x, y;
  const float* p;
  float *q, *r;
  uint64_t v[DSU_N + 1];
  float* t[3];
  dsu_a inner;
  int64_t z[2];
  int i; float f;
} dsu_b;
typedef struct dsu_h dsu_h;
const char* dsu_name(int code);
void dsu_free(dsu_h* h);
dsu_h* dsu_make(const dsu_b* cfg, dsu_h** out, void* stream);
int64_t dsu_bytes(int64_t n, uint32_t k, float f, double d, uint64_t s, const uint8_t* m,
                  int32_t* out, dsu_a* a);
int32_t dsu_count(void);
int dsu_rc(const uint16_t *w);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_maps_every_accepted_form():
    import ctypes as C
    from drawingspinup_amd import _header
    h = _header.parse(_WELL_FORMED)
    assert h.defines == {"DSU_N": 4, "DSU_NEG": -2} and h.opaque == {"dsu_h"}
    a, b = h.structs["dsu_a"], h.structs["dsu_b"]
    assert list(h.structs) == ["dsu_a", "dsu_b"] and issubclass(b, C.Structure)
    assert a._fields_ == [("a", C.c_uint32), ("b", C.c_double)]
    assert b._fields_ == [("x", C.c_int32), ("y", C.c_int32), ("p", C.c_void_p), ("q", C.c_void_p),
                          ("r", C.c_void_p), ("v", C.c_uint64 * 5), ("t", C.c_void_p * 3), ("inner", a),
                          ("z", C.c_int64 * 2), ("i", C.c_int), ("f", C.c_float)]
    assert h.protos == {
        "dsu_name": (C.c_char_p, [C.c_int]),
        "dsu_free": (None, [C.c_void_p]),
        "dsu_make": (C.c_void_p, [C.POINTER(b), C.c_void_p, C.c_void_p]),
        "dsu_bytes": (C.c_int64, [C.c_int64, C.c_uint32, C.c_float, C.c_double, C.c_uint64, C.c_void_p,
                                  C.c_void_p, C.POINTER(a)]),
        "dsu_count": (C.c_int32, []),
        "dsu_rc": (C.c_int, [C.c_void_p]),
    }
    assert b(1, 2).y == 2                                  # positional construction in the header's order


@pytest.mark.parametrize("snippet, offending", [
    ("int dsu_f(int (*cb)(int), void* s);", r"\(\*cb\)"),                                  # function pointer
    ("typedef struct { union { int a; float b; } u; } dsu_s;", "union"),                   # union
    ("typedef union { int a; float b; } dsu_s;", "union"),
    ("typedef struct { int32_t a : 3; } dsu_s;", "a : 3"),                                 # bit-field
    ("typedef struct { struct { int a; } in; int b; } dsu_s;", r"struct \{ int a; \}"),   # anonymous nested struct
    ("typedef struct { size_t n; } dsu_s;", "size_t"),                                     # unknown type words
    ("int dsu_f(size_t n);", "size_t"),
    ("int dsu_f(const dsu_missing* p);", "dsu_missing"),
    ("typedef struct { unsigned int n; } dsu_s;", "unsigned int n"),
    ("float dsu_f(void);", "float"),
    ("int dsu_f(float v[3]);", r"v\[3\]"),                                                 # array parameter
    ("int dsu_f(int n, ...);", r"\.\.\."),                                                 # variadic list
    ("int dsu_f();", r"dsu_f\(\)"),                                                        # no prototype
    ("int dsu_f(int32_t);", r"dsu_f\(int32_t\)"),                                          # unnamed parameter
    ("typedef struct dsu_h dsu_h; int dsu_f(dsu_h h);", "dsu_h h"),                        # opaque by value
    ("typedef struct { float a[DSU_UNSEEN]; } dsu_s;", "DSU_UNSEEN"),                      # extent not yet read
    ("typedef struct { int32_t a } dsu_s;", "int32_t a"),                                  # no `;`
    ("typedef int dsu_t;", "typedef int dsu_t"),
    ("#define DSU_SCALE 1.5\n", "DSU_SCALE 1.5"),                                          # not an integer
    ("#define DSU_TWICE(x) (2 * (x))\n", "DSU_TWICE"),                                     # function-like macro
    ("#pragma pack(1)\n", "pragma pack"),
    ("int dsu_f(void); int dsu_f(void);", "dsu_f"),                                        # declared twice
    ("static inline int dsu_f(void) { return 0; }", "static inline"),                      # a definition
    ("int dsu_f(void)", r"dsu_f\(void\)"),                                                 # no final `;`
    ("int other_f(void);", "other_f"),                                                     # not a dsu_ name
])
def test_reader_raises_on_what_is_outside_its_grammar(snippet, offending):
    """Never skipped, never guessed: the error carries the offending text."""
    from drawingspinup_amd import _header
    with pytest.raises(_header.DsuError, match=offending):
        _header.parse(snippet)


def _host_cc():
    """cc, or the clang that stands beside hipcc in the ROCm tree."""
    import shutil
    from drawingspinup_amd import build
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc())))
    for c in (shutil.which("cc"), os.path.join(rocm, "lib", "llvm", "bin", "clang"),
              os.path.join(rocm, "llvm", "bin", "clang")):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no host C compiler (cc, or clang of the ROCm tree)")


def test_struct_layouts_and_defines_match_the_host_compiler(tmp_path):
    """A stand-alone C program that includes dsu_hip.h prints sizeof of every struct, offsetof of every
    field and the value of every #define; the generated ctypes classes and DEFINES must say the same."""
    import subprocess
    from drawingspinup_amd import _lib
    h = _lib._HEADER
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "dsu_hip.h"', "int main(void) {"]
    for name, cls in h.structs.items():
        lines.append(f'  printf("S {name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("F {name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines += [f'  printf("D {d} %lld\\n", (long long)({d}));' for d in h.defines]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([_host_cc(), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    want = {}
    for name, cls in h.structs.items():
        want[f"S {name}"] = ctypes.sizeof(cls)
        want.update({f"F {name}.{f}": getattr(cls, f).offset for f, _ in cls._fields_})
    want.update({f"D {d}": v for d, v in h.defines.items()})
    got = {k: int(v) for k, v in (ln.rsplit(" ", 1) for ln in out.splitlines())}
    assert len(h.structs) == 12 and len(got) == len(out.splitlines())
    diff = {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    assert not diff, diff
    assert got["S dsu_nsr_step_args"] == 248 and got["F dsu_nsr_step_args.terms_out"] == 240
    # the defines the library's own sources use, as the compiler sees them
    for d in ("DSU_ABI_VERSION", "DSU_MAX_LEVELS", "DSU_RAY_LOSS_MAX_RAYS", "DSU_ADAMW_MAX_TENSORS",
              "DSU_OK", "DSU_EINVAL", "DSU_ELAUNCH", "DSU_EUNSUP"):
        assert got[f"D {d}"] == _lib.DEFINES[d]


def test_ops_constants_are_the_headers():
    from drawingspinup_amd import _lib, ops
    D = _lib.DEFINES
    assert ops.RAY_LOSS_MAX_RAYS == D["DSU_RAY_LOSS_MAX_RAYS"] == 8192
    assert (ops.RENDER_COUNT, ops.RENDER_FILL, ops.RENDER_RASTER) == \
        (D["DSU_RENDER_COUNT"], D["DSU_RENDER_FILL"], D["DSU_RENDER_RASTER"])
    assert (ops.UV_COUNT, ops.UV_FILL, ops.UV_RASTER) == (D["DSU_UV_COUNT"], D["DSU_UV_FILL"], D["DSU_UV_RASTER"])
    assert (ops.SKIN_COUNT, ops.SKIN_FILL, ops.SKIN_RUN) == (D["DSU_SKIN_COUNT"], D["DSU_SKIN_FILL"], D["DSU_SKIN_RUN"])
    assert ops.TEXTURE_FILTERS == {"nearest": D["DSU_TEX_NEAREST"], "bilinear": D["DSU_TEX_BILINEAR"],
                                   "trilinear": D["DSU_TEX_TRILINEAR"]}
    # each binned plan passes its own entry point's stage constants
    assert (ops.MeshRenderPlan.COUNT, ops.MeshRenderPlan.FILL) == (ops.RENDER_COUNT, ops.RENDER_FILL)
    assert (ops.UvBakePlan.COUNT, ops.UvBakePlan.FILL) == (ops.UV_COUNT, ops.UV_FILL)
    assert (ops.BoneVisibilityPlan.COUNT, ops.BoneVisibilityPlan.FILL) == (ops.SKIN_COUNT, ops.SKIN_FILL)
