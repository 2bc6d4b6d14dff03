"""Write down the host program of the training step: every library call, event and cross-stream wait in program order.

    python tools_dev/schedule_trace.py --out trace.txt [--engine FILE]

Bitwise tests cannot see a dropped wait that happens not to race; two traces can.  One line per call: the name, the stream it
went to (main / side / tail / s3 ... by first appearance), events numbered by creation, shapes and dtypes of tensor arguments,
other objects (workspaces, gradient rows) numbered by first appearance per type.  Wrapped: every public function of the ops
module, the engine's per-bucket optimizer steps, torch.cuda.Event.record, torch.cuda.Stream.wait_event / wait_stream and the
on_ready / on_dgrad callbacks of SSDEngine.backward.

--engine FILE loads FILE as ssd_object_detection_amd.engine: two versions of engine.py run in the same tree against the same
library, and a refactor of the schedule is checked with `diff` on the two outputs.  Every section starts the labels afresh."""
import argparse
import importlib.util
import inspect
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                           # noqa: E402


class Trace:
    def __init__(self):
        self.lines = []
        self.section("start")

    def section(self, name):
        self.streams, self.events, self.objects = {}, {}, {}
        self.lines.append("== " + name)

    def stream(self, s=None):
        s = torch.cuda.current_stream() if s is None else s
        key = s.cuda_stream
        if key not in self.streams:
            n = len(self.streams)
            self.streams[key] = ("main", "side", "tail")[n] if n < 3 else "s%d" % n
        return self.streams[key]

    def event(self, ev):
        key = id(ev)
        if key not in self.events:
            self.events[key] = (len(self.events), ev)  # (the reference keeps the id from being reused)
        return "ev%d" % self.events[key][0]

    def show(self, v):
        if isinstance(v, torch.Tensor):
            return "%s%s" % (str(v.dtype).replace("torch.", ""), list(v.shape))
        if isinstance(v, (list, tuple)):
            return "[" + ", ".join(self.show(u) for u in v) + "]"
        if isinstance(v, dict):
            return "{" + ", ".join("%s=%s" % (k, self.show(u)) for k, u in v.items()) + "}"
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v)
        if isinstance(v, torch.cuda.Event):
            return self.event(v)
        if isinstance(v, torch.cuda.Stream):
            return self.stream(v)
        kind = self.objects.setdefault(type(v).__name__, {})
        if id(v) not in kind:
            kind[id(v)] = (len(kind), v)
        return "%s#%d" % (type(v).__name__, kind[id(v)][0])

    def call(self, name, args, kwargs, defaults={}):
        text = [self.show(a) for a in args] + ["%s=%s" % (k, self.show(v)) for k, v in kwargs.items()
                                               if not (k in defaults and v is defaults[k])]
        self.lines.append("%s @%s (%s)" % (name, self.stream(), ", ".join(text)))

    def wrap(self, name, fn):
        # a keyword argument that restates the function's default (None, True, False) is the same call: not written
        defaults = {k: p.default for k, p in inspect.signature(fn).parameters.items()
                    if p.default is None or isinstance(p.default, bool)}

        def traced(*args, **kwargs):
            self.call(name, args, kwargs, defaults)
            return fn(*args, **kwargs)
        traced.__wrapped__ = fn
        return traced


def install(trace, ops, engine_mod):
    for name, fn in list(vars(ops).items()):
        if not name.startswith("_") and inspect.isfunction(fn) and fn.__module__ == ops.__name__:
            setattr(ops, name, trace.wrap(name, fn))
    for name in ("adam_range", "sgd_range", "refresh_weights"):
        fn = getattr(engine_mod.SSDEngine, name)
        setattr(engine_mod.SSDEngine, name,
                (lambda n, f: lambda self, *a, **k: (trace.call(n, a, k), f(self, *a, **k))[1])(name, fn))
    Event, Stream = torch.cuda.Event, torch.cuda.Stream
    new, record, wait_event, wait_stream = Event.__new__, Event.record, Stream.wait_event, Stream.wait_stream

    def traced_new(cls, *args, **kwargs):
        ev = new(cls, *args, **kwargs)
        trace.event(ev)
        return ev

    def traced_record(ev, stream=None):
        trace.lines.append("record %s on %s" % (trace.event(ev), trace.stream(stream)))
        return record(ev) if stream is None else record(ev, stream)

    def traced_wait_event(stream, ev):
        trace.lines.append("wait_event %s <- %s" % (trace.stream(stream), trace.event(ev)))
        return wait_event(stream, ev)

    def traced_wait_stream(stream, other):
        trace.lines.append("wait_stream %s <- %s" % (trace.stream(stream), trace.stream(other)))
        return wait_stream(stream, other)

    Event.__new__ = staticmethod(traced_new)
    Event.record, Stream.wait_event, Stream.wait_stream = traced_record, traced_wait_event, traced_wait_stream


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--engine", help="load this file as ssd_object_detection_amd.engine")
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--dense-batch", type=int, default=46)
    a = ap.parse_args()
    import ssd_object_detection_amd                    # noqa: F401
    if a.engine:
        spec = importlib.util.spec_from_file_location("ssd_object_detection_amd.engine", a.engine)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        ssd_object_detection_amd.engine = mod
    import ssd_object_detection_amd.engine as engine_mod
    import ssd_object_detection_amd.ops as ops
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    SSDEngine = engine_mod.SSDEngine
    tr = Trace()
    install(tr, ops, engine_mod)

    def inputs(B, seed):
        g = torch.Generator().manual_seed(seed)
        x = ops.image_prep(torch.rand((B, 300, 300, 3), generator=g).cuda())
        dloc = (torch.randn((B, 8732, 4), generator=g) * 1e-3).bfloat16().cuda()
        dconf = (torch.randn((B, 8732, 81), generator=g) * 1e-3).bfloat16().cuda()
        return x, dloc, dconf

    def fwd_bwd(eng, name, data, **switches):
        saved = {k: getattr(eng, k) for k in switches}
        for k, v in switches.items():
            setattr(eng, k, v)
        try:
            tr.section(name)
            x, dloc, dconf = data
            eng.forward(x)
            eng.backward(dloc, dconf,
                         on_ready=lambda tensors: tr.lines.append("on_ready @%s %s" % (tr.stream(), list(tensors))),
                         on_dgrad=lambda node: tr.lines.append("on_dgrad @%s %s" % (tr.stream(), node)))
            torch.cuda.synchronize()
        finally:
            for k, v in saved.items():
                setattr(eng, k, v)

    # two fused-Adam train steps: the first learns the fallbacks, the second uses them
    B = a.batch
    model = SSDObjectDetectionModel(classes=80, log_dir=tempfile.mkdtemp(), timestamp_dir=False, seed=2)
    opt = optimizers.Adam(1e-3)
    gen = torch.Generator(device="cuda").manual_seed(64)
    img = torch.rand((B, 300, 300, 3), generator=gen, device="cuda")
    cls_l, box_l = synth_batch_gt(6400, B)
    gt = ops.pack_gt(box_l, cls_l)
    for step in (1, 2):
        tr.section("train step %d, batch %d" % (step, B))
        model._train_step(ops.image_prep(img, normalize=True), *model.match_async(gt), opt)
        torch.cuda.synchronize()
    del model

    eng = SSDEngine(classes=81, seed=11)
    data = inputs(B, 41)
    fwd_bwd(eng, "forward + backward, batch %d, first call" % B, data)
    fwd_bwd(eng, "forward + backward, batch %d" % B, data)
    for name, value in [("overlap_heads", False), ("wgrad_group", 1), ("batch_chain_wgrads", False), ("split_heads_dgrad", 0),
                        ("split_heads_dgrad", 1), ("chain_heads_split", False), ("chain_prefetch", False), ("pack_side", False),
                        ("tail_stream", False)]:
        fwd_bwd(eng, "%s=%r" % (name, value), data, **{name: value})
    del eng

    eng = SSDEngine(classes=81, seed=11, l2norm=True)
    fwd_bwd(eng, "l2norm, first call", data)
    fwd_bwd(eng, "l2norm", data)
    fwd_bwd(eng, "l2norm, overlap_heads=False", data, overlap_heads=False)
    del eng

    B = a.dense_batch
    eng = SSDEngine(classes=81, seed=13, sparse_heads=False)
    data = inputs(B, 43)
    fwd_bwd(eng, "dense heads, batch %d, first call" % B, data)
    fwd_bwd(eng, "dense heads, batch %d" % B, data)
    for name in ("big_heads_side", "pack_side", "overlap_heads"):
        fwd_bwd(eng, "dense heads, %s=False" % name, data, **{name: False})

    with open(a.out, "w") as f:
        f.write("\n".join(tr.lines) + "\n")
    print("%d lines -> %s" % (len(tr.lines), a.out))


if __name__ == "__main__":
    main()
