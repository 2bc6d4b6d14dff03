"""CPU suite: the C-ABI library builds, loads and exports every symbol include/ssd_hip.h declares
(no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    text = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\b(ssd_[a-z0-9_]+)\s*\(", text)
    return sorted(set(names))


def test_library_exports_every_declared_symbol():
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    names = declared_functions()
    assert len(names) >= 8
    for n in names:
        assert hasattr(L, n), "missing export: " + n
    assert set(_lib._SIGNATURES) == set(names), set(_lib._SIGNATURES) ^ set(names)
    assert L.ssd_hip_abi_version() >= 1
    assert L.ssd_status_string(0) == b"ok"


def test_host_side_argument_checks():
    """Entry points validate on the host before any launch: callable without a GPU."""
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    hw = (ctypes.c_int * 12)(38, 38, 19, 19, 10, 10, 5, 5, 3, 3, 1, 1)
    roff = (ctypes.c_int * 7)(0, 1, 3, 5, 7, 8, 9)
    assert L.ssd_priors_count(hw, 6, roff) == 8732                     # models/ssd_model.py:221
    assert L.ssd_priors_count(hw, 0, roff) == _lib.SSD_ERR_VALUE
    assert L.ssd_match_encode_workspace_bytes(64, 8732, 500) > 0
    # thresh <= 0 and n_t > A are the reference's asserts (utils/bbox.py:50-51)
    args = [None, None, None, 1, 0, 0, None, None, 8732, None]
    assert L.ssd_match_encode(*args, 0.0, None, None, None, None, None, 0, None) == _lib.SSD_ERR_ASSERT
    args[5] = 9000
    assert L.ssd_match_encode(*args, 0.5, None, None, None, None, None, 0, None) == _lib.SSD_ERR_ASSERT


def test_round4_entries_refuse_on_the_host():
    """ssd_conv_chain / ssd_chain_pack_weights / ssd_conv2d_bwd_weight_batched / ssd_heads_bwd_data_sparse_levels decide on the
    host whether they serve a call -- SSD_ERR_VALUE / SSD_ERR_UNSUPPORTED come back before anything touches a device."""
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    dummy = ctypes.c_void_p(0x1000)                                     # never dereferenced on these paths
    assert L.ssd_conv_chain(None, None, 0, 1, None) == _lib.SSD_ERR_VALUE
    lay = (_lib.ChainLayer * 2)()

    def fill(d, hi, kc, ho, n, k=1):
        d.w, d.out = dummy, dummy
        d.Hi, d.Wi, d.Kc, d.Ho, d.Wo, d.N, d.ksize, d.mul, d.div, d.pad_t, d.pad_l = hi, hi, kc, ho, ho, n, k, 1, 1, 0, 0

    fill(lay[0], 19, 256, 19, 128)                                      # 361 pixels: not an LDS-resident map
    assert L.ssd_conv_chain(dummy, lay, 1, 4, None) == _lib.SSD_ERR_UNSUPPORTED
    fill(lay[0], 4, 64, 4, 128)                                         # 64 input channels: not a multiple of 128
    assert L.ssd_conv_chain(dummy, lay, 1, 4, None) == _lib.SSD_ERR_UNSUPPORTED
    fill(lay[0], 4, 128, 4, 128)
    fill(lay[1], 4, 256, 4, 128)                                        # does not read what layer 0 writes
    assert L.ssd_conv_chain(dummy, lay, 2, 4, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_conv_chain(dummy, lay, _lib.SSD_CHAIN_MAX_LAYERS + 1, 4, None) == _lib.SSD_ERR_VALUE
    packs = (_lib.ChainPack * 1)()
    assert L.ssd_chain_pack_weights(packs, 0, None) == _lib.SSD_ERR_VALUE
    packs[0].src, packs[0].dst, packs[0].N, packs[0].K = dummy, dummy, 24, 64          # N not a multiple of 16
    assert L.ssd_chain_pack_weights(packs, 1, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_chain_prefetch(packs, _lib.SSD_CHAIN_PACK_MAX + 1, None) == _lib.SSD_ERR_VALUE
    items = (_lib.WgradItem * 9)()
    assert L.ssd_conv2d_bwd_weight_batched(None, 1, None, 0, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_conv2d_bwd_weight_batched(items, 9, dummy, 1 << 30, None) == _lib.SSD_ERR_UNSUPPORTED    # more than 8 layers
    it = items[0]
    it.x, it.dy, it.dw = dummy, dummy, dummy
    it.B, it.H, it.W, it.Cin, it.Cout, it.ldy, it.ksize, it.stride, it.pad_t, it.pad_l, it.Ho, it.Wo = 64, 19, 19, 1024, 1024, 1024, 1, 1, 0, 0, 19, 19
    assert L.ssd_conv2d_bwd_weight_batched(items, 1, None, 0, None) == _lib.SSD_ERR_WORKSPACE
    need = L.ssd_conv2d_bwd_weight_batched_workspace_bytes(items, 1)
    assert need > 0
    assert L.ssd_conv2d_bwd_weight_batched(items, 1, dummy, need, None) == _lib.SSD_ERR_UNSUPPORTED       # the 256-wide tile kernel's layer
    assert L.ssd_heads_bwd_data_sparse_levels(None, None, 4, 3, None, 0, None) != _lib.SSD_OK


def test_every_declared_function_has_a_derived_prototype():
    """The binding is parsed from the header: no prototype may be lost on the way."""
    from ssd_object_detection_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssd_hip.h")).read(), flags=re.S)
    assert len(_lib._SIGNATURES) == len(re.findall(r"\b(ssd_[a-z0-9_]+)\s*\(", text)) == len(declared_functions())
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "ssd_hip.h"))
    assert (_lib.SSD_OK, _lib.SSD_ERR_ASSERT, _lib.SSD_ERR_VALUE, _lib.SSD_ERR_WORKSPACE, _lib.SSD_ERR_LAUNCH,
            _lib.SSD_ERR_UNSUPPORTED) == (0, -1, -2, -3, -4, -5)
    assert (_lib.SSD_MAX_LEVELS, _lib.SSD_CHAIN_MAX_LAYERS, _lib.SSD_CHAIN_PACK_MAX) == (8, 8, 16)
    assert _lib.SSD_GRID_VERIFIED == 0x5D5D0001 and _lib.SSD_LOSS_MAX_CLASSES == 303          # a hex and a decimal #define
    from ssd_object_detection_amd import ops
    assert (ops.AUG_PHOTO, ops.AUG_EXPAND, ops.AUG_CROP, ops.AUG_FLIP, ops.AUG_ALL) == (1, 2, 4, 8, 15)


def test_pinned_signatures():
    """Entry points spelled out by hand, one or more for every row of the type map and of the pointer rule."""
    from ssd_object_detection_amd import _lib
    VP, I, F, D, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    P = ctypes.POINTER
    want = {
        "ssd_adam_step": (I, [VP, VP, VP, VP, VP, ctypes.c_longlong, VP, VP, F, F, F, F, F, VP]),
        "ssd_match_encode": (I, [VP, VP, VP, I, I, I, VP, VP, I, P(_lib.PriorGrid), D, VP, VP, VP, VP, VP, Z, VP]),
        "ssd_augment_plan": (I, [VP, VP, VP, VP, I, I, I, ctypes.c_uint64, ctypes.c_int64, VP, VP, VP, VP, VP]),
        "ssd_heads_bwd_data_sparse_levels": (I, [P(_lib.HeadGrads), P(_lib.HeadLayers), I, ctypes.c_uint, VP, Z, VP]),
        "ssd_conv2d_bwd_weight_workspace_bytes": (Z, [I] * 7),
        "ssd_dev_mfma_calibration_flops": (D, [I]),
        "ssd_status_string": (ctypes.c_char_p, [I]),
        "ssd_conv2d_fwd": (I, [VP, VP, VP, VP, I, I, I, I, I, I, I, I, I, I, I, I, VP, Z, VP]),
        "ssd_priors": (I, [VP, I, VP, VP, VP, D, VP, VP]),                      # host arrays: addresses like any other
        "ssd_dev_knob": (I, [ctypes.c_char_p, I]),
        "ssd_conv_chain": (I, [VP, P(_lib.ChainLayer), I, I, VP]),
        "ssd_hip_abi_version": (I, []),
    }
    for name, (res, args) in want.items():
        got_res, got_args = _lib._SIGNATURES[name]
        assert got_res is res, (name, got_res)
        assert got_args == args, (name, got_args)
    fn = _lib.lib().ssd_adam_step
    assert fn.restype is I and list(fn.argtypes) == want["ssd_adam_step"][1]


LAYOUT_STRUCTS = (("ssd_prior_grid", "PriorGrid"), ("ssd_head_grads", "HeadGrads"), ("ssd_head_layers", "HeadLayers"),
                  ("ssd_chain_layer", "ChainLayer"), ("ssd_chain_pack", "ChainPack"), ("ssd_wgrad_item", "WgradItem"),
                  ("ssd_augment_params", "AugmentParams"))


def test_struct_layouts_equal_the_compilers(tmp_path):
    """sizeof and every offsetof as the host C++ compiler lays the header's structs out, against the derived ctypes classes
    and the numpy record of ssd_augment_params."""
    import subprocess
    from ssd_object_detection_amd import _lib, ops
    assert set(_lib.STRUCTS) == {c for c, _ in LAYOUT_STRUCTS}
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "ssd_hip.h"', 'int main() {']
    for cname, pyname in LAYOUT_STRUCTS:
        cls = getattr(_lib, pyname)
        assert cls is _lib.STRUCTS[cname]
        lines.append('    std::printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('    std::printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                         % (cname, field, cname, field, cname, field))
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = {}
    for row in subprocess.check_output([str(exe)], text=True).split("\n"):
        if row:
            cname, key, *nums = row.split()
            seen.setdefault(cname, {})[key] = tuple(int(v) for v in nums)
    for cname, pyname in LAYOUT_STRUCTS:
        cls = getattr(_lib, pyname)
        got = {"sizeof": (ctypes.sizeof(cls),)}
        got.update({f: (getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_})
        assert got == seen[cname], (cname, got, seen[cname])
    # the field names the six hand-written classes had
    assert [f for f, _ in _lib.PriorGrid._fields_] == ["levels", "grid_h", "grid_w", "per_cell", "verified"]
    assert [f for f, _ in _lib.HeadGrads._fields_] == ["levels", "hw", "per_cell", "npad", "rows", "row_of_pixel", "pixel_of_row",
                                                       "count"]
    assert [f for f, _ in _lib.HeadLayers._fields_] == ["levels", "H", "W", "Cin", "cout", "x", "w_tap", "relu_bits", "relu_src",
                                                        "dx", "dw", "dbias"]
    assert [f for f, _ in _lib.ChainLayer._fields_] == ["w", "bias", "out", "mask_bits", "mask_src", "relu_bits", "Hi", "Wi", "Kc",
                                                        "Ho", "Wo", "N", "ksize", "mul", "div", "pad_t", "pad_l", "relu", "accumulate"]
    assert [f for f, _ in _lib.ChainPack._fields_] == ["src", "dst", "N", "K"]
    assert [f for f, _ in _lib.WgradItem._fields_] == ["x", "dy", "dw", "dbias", "B", "H", "W", "Cin", "Cout", "ldy", "ksize", "stride",
                                                       "pad_t", "pad_l", "Ho", "Wo"]
    # the numpy record of ssd_augment_params: the compiler's size and offsets, arrays flattened
    aug = seen["ssd_augment_params"]
    dt = ops.AUG_PARAM_DTYPE
    assert dt.itemsize == aug["sizeof"][0] == 80
    assert ops.AUG_PARAM_FIELDS == ("stages", "mode", "trial", "photo", "canvas_w", "canvas_h", "off_x", "off_y", "patch_x",
                                    "patch_y", "patch_w", "patch_h", "flip", "n_boxes", "reserved0", "reserved1", "delta", "alpha",
                                    "saturation", "hue") == dt.names
    for name in dt.names:
        want = aug["reserved"][0] + 4 * int(name[-1]) if name.startswith("reserved") else aug[name][0]
        assert dt.fields[name][1] == want, name
        assert dt.fields[name][0] == (np.float32 if name in ("delta", "alpha", "saturation", "hue") else np.int32), name


PARSER_FRAGMENT = """
#define SSD_N 3   /* a bound */
typedef enum { SSD_A = 2, SSD_B, SSD_C = 0x10 } ssd_e;
typedef struct {
    int a, b[SSD_N];     /* a comma list with an array in it */
    const void* p;
    float* q[2], *r;
    int32_t c;
} ssd_t;
int ssd_f(const ssd_t* t, long long n,
          const float* x, size_t bytes);
size_t ssd_g(void);
"""


def test_parser_reads_the_headers_idioms_and_refuses_the_rest():
    import pytest
    from ssd_object_detection_amd import _lib
    VP = ctypes.c_void_p
    constants, structs, signatures = _lib.parse_header(PARSER_FRAGMENT)
    assert constants == {"SSD_N": 3, "SSD_A": 2, "SSD_B": 3, "SSD_C": 16}
    assert list(structs) == ["ssd_t"]
    assert structs["ssd_t"]._fields_ == [("a", ctypes.c_int), ("b", ctypes.c_int * 3), ("p", VP), ("q", VP * 2), ("r", VP),
                                         ("c", ctypes.c_int32)]
    assert signatures == {"ssd_f": (ctypes.c_int, [ctypes.POINTER(structs["ssd_t"]), ctypes.c_longlong, VP, ctypes.c_size_t]),
                          "ssd_g": (ctypes.c_size_t, [])}
    for bad in ("int ssd_x(short a);",                                    # a scalar outside the type map
                "short ssd_x(int a);",                                    # ... as the return type
                "int ssd_x(unsigned int a);",                             # a spelling the header does not use
                "typedef struct { int a; short b; } ssd_s;",              # a member outside the type map
                "typedef struct { int a[SSD_UNKNOWN]; } ssd_s;",          # a bound that is no literal and no #define
                "typedef struct { int (*fn)(int); } ssd_s;",              # not a plain member
                "int ssd_ok(int a); static int x = 3;"):                  # not a prototype at all
        with pytest.raises(TypeError, match="ssd_hip.h"):
            _lib.parse_header(bad)


def test_a_missing_header_is_reported(monkeypatch):
    import pytest
    from ssd_object_detection_amd import _lib
    monkeypatch.setattr(_lib, "HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(RuntimeError, match="ssd_hip.h is missing"):
        _lib._read_header()


def test_check_maps_statuses_to_exceptions():
    import pytest
    from ssd_object_detection_amd import _lib
    with pytest.raises(ValueError):
        _lib.check(_lib.SSD_ERR_UNSUPPORTED)
    with pytest.raises(NotImplementedError) as e:
        _lib.check(_lib.SSD_ERR_UNSUPPORTED, unsupported="m")
    assert e.value.args == ("m",)
    with pytest.raises(ValueError):
        _lib.check(_lib.SSD_ERR_VALUE, unsupported="m")
    with pytest.raises(AssertionError):
        _lib.check(_lib.SSD_ERR_ASSERT, unsupported="m")
    with pytest.raises(RuntimeError):
        _lib.check(_lib.SSD_ERR_WORKSPACE, unsupported="m")
    assert _lib.check(_lib.SSD_OK, unsupported="m") is None and _lib.check(_lib.SSD_OK) is None


def test_synthetic_generator_matches_fixture_inputs():
    from ssd_object_detection_amd.data_loaders.synthetic import synth_gt
    z = np.load(os.path.join(ROOT, "tests", "golden", "match_synth.npz"))
    for i in range(24):
        cls, box = synth_gt(i)
        assert np.array_equal(cls, z["mix%02d_gt_cls" % i]) and np.array_equal(box, z["mix%02d_gt_box" % i])
    cls, box = synth_gt(1000 + 14, 93)
    assert np.array_equal(box, z["fix14_gt_box"])
