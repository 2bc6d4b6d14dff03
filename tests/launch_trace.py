"""Launch recorder: the sequence of C-ABI launches an engine makes, each with its operands, in a form that does not depend on
where the allocator put things.  tests/test_launch_trace_gpu.py compares it against tests/golden/launch_trace.json, which
was recorded BEFORE the host-side MX-fp8 bookkeeping was restructured: a refactor of the Python around the kernels must
reproduce it call by call.

A call is canonicalised as [entry point, argument, ...] without the trailing stream:
  scalar                   its value
  pointer                  0 for null, else the index (from 1) of that address's first appearance in the scenario's trace:
                           wiring and aliasing are recorded, addresses are not
  pointer to a host struct of include/ssd_hip.h (one, or a ctypes array of them)
                           field by field, by the same rules
Recorded are the entry points whose last parameter is `stream`: the launching ones (the size / plan queries are not)."""
import ctypes
import hashlib
import json
import re

import torch

from ssd_object_detection_amd import _lib


def launching_entry_points():
    """Names of the prototypes of include/ssd_hip.h whose last parameter is `stream`."""
    text = re.sub(r"/\*.*?\*/", " ", _lib._read_header(), flags=re.S)
    names = [m.group(1) for m in re.finditer(r"\b(ssd_\w+)\s*\(([^()]*)\)\s*;", text, re.S)
             if re.search(r"\bstream\s*$", m.group(2))]
    assert names and all(n in _lib._SIGNATURES for n in names)
    return names


class Recorder:
    """`with Recorder() as rec: ...` wraps the launching entry points on the loaded library object for the block;
    rec.calls is the canonical trace, rec.lines() its `name:digest` form."""

    def __init__(self):
        self.calls, self._index, self._saved = [], {}, {}

    def __enter__(self):
        L = _lib.lib()
        for name in launching_entry_points():
            fn = getattr(L, name)
            self._saved[name] = fn
            setattr(L, name, self._wrap(name, fn, _lib._SIGNATURES[name][1]))
        return self

    def __exit__(self, *exc):
        L = _lib.lib()
        for name, fn in self._saved.items():
            setattr(L, name, fn)
        return False

    def _wrap(self, name, fn, argtypes):
        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            self.calls.append([name] + [self._arg(a, t) for a, t in zip(args[:-1], argtypes[:-1])])
            return fn(*args)
        return call

    def _pointer(self, v):
        v = getattr(v, "value", v)                     # c_void_p, int or None
        if not v:
            return 0
        assert isinstance(v, int), "not an address: %r" % (v,)
        return self._index.setdefault(int(v), len(self._index) + 1)

    def _arg(self, a, ctype):
        if ctype is ctypes.c_void_p:
            if isinstance(a, ctypes.Array):            # a host array handed over by address: its values
                return [x for x in a]
            return {"p": self._pointer(a)}
        if isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer):
            obj = getattr(a, "_obj", a)                # ctypes.byref(struct), a struct or an array of structs
            if obj is None:
                return 0
            items = list(obj) if isinstance(obj, ctypes.Array) else [obj]
            return [self._struct(s) for s in items]
        if isinstance(a, bytes):
            return a.decode()
        return a

    def _field(self, v, ctype):
        if issubclass(ctype, ctypes.Array):
            return [self._field(x, ctype._type_) for x in v]
        if ctype is ctypes.c_void_p:
            return {"p": self._pointer(v)}
        return v

    def _struct(self, s):
        return {name: self._field(getattr(s, name), ctype) for name, ctype in s._fields_}

    def lines(self):
        return ["%s:%s" % (c[0], hashlib.sha256(json.dumps(c[1:], sort_keys=True).encode()).hexdigest()[:10])
                for c in self.calls]


def _image(B, S, seed):
    from ssd_object_detection_amd import ops
    img = torch.rand((B, S, S, 3), generator=torch.Generator().manual_seed(seed)).cuda()
    return ops.image_prep(img, normalize=True)


def _heads(eng, B, seed):
    """The compact head gradient of a seeded dense (dloc, dconf): prepared outside the recording window."""
    g = torch.Generator().manual_seed(seed)
    dloc = (torch.randn((B, eng.A, 4), generator=g) * 1e-3).cuda().bfloat16()
    dconf = (torch.randn((B, eng.A, eng.classes), generator=g) * 1e-3).cuda().bfloat16()
    return eng.heads_from_dense(dloc, dconf)


def _resnet(batchnorm=None):
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    return ResNet50SSDEngine(classes=81, in_size=256, seed=0, batchnorm=batchnorm), 2, 256


def _ssd300(l2norm=None):
    from ssd_object_detection_amd.engine import SSDEngine
    return SSDEngine(classes=81, seed=0, l2norm=l2norm), 1, 300


def _fwd(*a, **kw):
    return lambda eng, x, heads: eng.forward(x, *a, **kw)


def _fwd_bwd(*a, bwd=None, **kw):
    def run(eng, x, heads):
        out = eng.forward(x, *a, **kw)
        eng.backward(None, None, heads=heads, **(bwd or {}))
        return out
    return run


# name -> (engine factory, its arguments, the run, whether it needs a head gradient)
SCENARIOS = {
    "a_resnet_bf16_fwd_bwd": (_resnet, {}, _fwd_bwd(), True),
    "b_resnet_mxfp8_fwd": (_resnet, {}, _fwd("mxfp8"), False),
    "c_resnet_mxfp8_train_fwd_bwd": (_resnet, {}, _fwd_bwd("mxfp8", train=True), True),
    "d_resnet_mxfp8_train_fwd_bwd_bf16_dgrad": (_resnet, {}, _fwd_bwd("mxfp8", train=True, bwd=dict(dgrad_precision="bf16")), True),
    "e_resnet_bn_train_fwd_bwd": (_resnet, dict(batchnorm=True), _fwd_bwd(train=True), True),
    "f_resnet_bn_infer_fwd": (_resnet, dict(batchnorm=True), _fwd(), False),
    "g_ssd300_bf16_fwd": (_ssd300, {}, _fwd(), False),
    "h_ssd300_mxfp8_fwd": (_ssd300, {}, _fwd("mxfp8"), False),
    "i_ssd300_l2norm_bf16_fwd": (_ssd300, dict(l2norm=True), _fwd(), False),
}


def record(name):
    """(recorder, engine, (loc, conf)) of scenario `name`: a fresh engine runs it twice and the SECOND run is recorded, so
    that learned fallbacks and workspace growth have settled."""
    factory, kw, run, needs_heads = SCENARIOS[name]
    eng, B, S = factory(**kw)
    x = _image(B, S, seed=1)
    heads = _heads(eng, B, seed=2) if needs_heads else None
    run(eng, x, heads)
    torch.cuda.synchronize()
    with Recorder() as rec:
        out = run(eng, x, heads)
    torch.cuda.synchronize()
    return rec, eng, out
