"""GPU: the MX-fp8 training backward of ResNet50SSDEngine -- forward(x, "mxfp8", train=True), then backward() with its 37 fp8
data gradients and 36 fp8 gradient maps -- as a composition, against the teacher-forced float64 oracle in its mx= mode
(tests/forced_oracle.py).  Masks, routes and weight-gradient operands come from the engine's own fp8 forward as in
tests/test_resnet_forced_gpu.py; the fp8 gradient map a data gradient reads is forced too (the engine's stored map,
dequantised by the CPU rule), the fp8 filters are the oracle's own quantisation of the bf16 filters, and which map a launch
reads -- root(i) -- the oracle derives itself.  What is forced is pinned first: every stored fp8 map is bitwise the CPU
quantisation of the bf16 map the engine left, the fp8 filters that of w_t, w_t the flipped transpose of the filters.  The bound
of a tensor is the bf16 one, 3 * rel_l2(R, T) + 1e-3: only bf16 storage noise is left.  Every activation is NaN before the
forward; every gradient, fp8 map and fp8 filter poisoned before backward().  Seeded defects on the oracle's side, and two
mutations of the engine's real run (a launch handed another root's fp8 map; an accumulate dropped) that check() must refuse."""
import copy

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict as S                                        # noqa: E402
from tests import forced_oracle as FO                                # noqa: E402
from tests import test_resnet_forced_gpu as BF                       # noqa: E402

CLASSES = 81
RESULTS = {}


class Forced(BF.Forced):
    mutation = None                    # ("wrong_dy", node, other root) | ("no_accumulate", node): how the NEXT run() is bent

    def run_forward(self, engine, x):
        for a in engine._acts(self.B)["acts"][1:]:
            a.fill_(float("nan"))
        engine.forward(x, "mxfp8", train=True)

    def run(self):
        import ssd_object_detection_amd.ops as ops
        e, orig = self.engine, ops.conv2d_bwd_data_mxfp8
        order = sorted(e.mx_dgrad, reverse=True)                        # backward() walks the nodes from the last to the first
        self.launches = launches = []
        mutation = self.mutation or (None, None)

        def counted(dyq, dys, wtq, wts, relu_src, x_shape, *args, accumulate=False, **kw):
            i = order[len(launches)]
            assert tuple(x_shape) == tuple(e._acts(self.B)["acts"][e.nodes[i]["src"] + 1].shape), (i, x_shape)
            launches.append((i, accumulate))
            if mutation[0] == "wrong_dy" and mutation[1] == i:
                other = e.mxfp8_grads(self.B)[mutation[2]]               # written and final by now: a later node's map
                assert other[0].shape == dyq.shape and other[0].data_ptr() != dyq.data_ptr()
                dyq, dys = other
            if mutation[0] == "no_accumulate" and mutation[1] == i:
                assert accumulate, "node %d does not accumulate" % i
                accumulate = False
            return orig(dyq, dys, wtq, wts, relu_src, x_shape, *args, accumulate=accumulate, **kw)

        ops.conv2d_bwd_data_mxfp8 = counted
        try:
            super().run()
        finally:
            ops.conv2d_bwd_data_mxfp8 = orig

    def mx_operands(self):
        """The forced operands, and -- while the engine's state is at hand -- what they are forced FROM, each compared on the CPU
        with the rule it must follow (the mismatches are kept for check_forward_state)"""
        e, c = self.engine, self.c
        self.state_errors = err = []
        g8 = {r: (q.cpu(), sc.cpu()) for r, (q, sc) in e.mxfp8_grads(self.B).items()}
        if set(g8) != set(e.mx_gmaps) or len(g8) != 36:
            err.append("fp8 gradient maps %s" % sorted(g8))
        for r, (q, sc) in g8.items():
            q_ref, s_ref = S.ref_quantize_mx(c["gacts"][r + 1].cpu())
            if not (torch.equal(q, q_ref) and torch.equal(sc, s_ref)):
                err.append("fp8 gradient map %d is not the quantisation of gact%d" % (r, r + 1))
        wt = {}
        for i in sorted(e.mx_dgrad):
            w = self.weights["conv%d/kernel" % i]
            w_t = e.w_t[i].cpu()
            if not torch.equal(w_t.to(FO.F64), FO.flipped_transpose(w)):
                err.append("w_t[%d] is not the flipped transpose of the bf16 filters" % i)
            q_ref, s_ref = S.ref_quantize_mx(w_t)
            q, sc = e.mxfp8_wt(i)
            if not (torch.equal(q.cpu(), q_ref) and torch.equal(sc.cpu(), s_ref)):
                err.append("fp8 transposed filters of node %d are not the quantisation of w_t" % i)
            wt[i] = FO.mx_filters(w)
        return dict(dgrad=set(e.mx_dgrad), dy={r: S.ref_dequantize_mx(q, sc).to(FO.F64) for r, (q, sc) in g8.items()}, wt=wt)

    def oracle(self, **kw):
        trace = {}
        out = super().oracle(trace=trace, **kw)
        if not kw.get("first_node") and not kw.get("defect"):
            self.roots = trace["root"]
        return out

    def check_forward_state(self):
        e = self.engine
        read = {nd["src"] + 1 for nd in e.nodes if nd["kind"] == "conv"}                   # operands and masks of the convolutions
        read |= {i + 1 for i, nd in enumerate(e.nodes) if nd["feature"]}                   # the heads' operands and masks
        read |= {nd["src"][1] + 1 for nd in e.nodes if nd["kind"] == "add" and e.nodes[nd["src"][1]]["relu"]}   # identity masks
        for a in sorted(read):
            assert bool(torch.isfinite(self.stored[a].float()).all()), "activation %d: the training-mode fp8 forward did not write it" % a
        super().check_forward_state()                                                      # the pooled map and its codes
        assert not self.state_errors, self.state_errors
        assert self.roots == list(e.mx_groot), "the oracle's roots are not the engine's plan"
        assert [i for i, _ in self.launches] == sorted(e.mx_dgrad, reverse=True) and len(self.launches) == 37, self.launches
        assert any(acc for _, acc in self.launches) and not all(acc for _, acc in self.launches)


def result(key):
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    if key not in RESULTS:
        if key == "full":
            RESULTS[key] = Forced(ResNet50SSDEngine(classes=CLASSES, seed=5), 1, 21)
        else:
            e = ResNet50SSDEngine(classes=CLASSES, seed=6, in_size=256)
            assert e.grids == ((32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1), (1, 1))
            RESULTS[key] = Forced(e, 3, 23, level_scale=(1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 32.0))
    return RESULTS[key]


def test_full_geometry():
    r = result("full")
    assert r.engine.A == 24564
    r.check("ResNet-50 SSD512 batch 1, MX-fp8 training backward")


def test_reduced_geometry():
    r = result("reduced")
    r.check("ResNet-50 SSD at 256, batch 3, MX-fp8 training backward")


def _graph():
    from ssd_object_detection_amd.resnet_engine import resnet50_ssd512_graph
    nodes = [dict(nd, kind=nd["op"]) for nd in resnet50_ssd512_graph()]
    return (nodes,) + BF._adds(nodes) + ([i for i, nd in enumerate(nodes) if nd["feature"]],)


def defects():
    """The bf16 file's list under mx, and the fp8 wiring errors: (defect, first_node) on the node list, which needs no device"""
    nodes, proj, ident, fm = _graph()
    wide, deep = nodes[ident[0]]["src"][0], nodes[ident[-1]]["src"][0]   # the 1x1 expands of a conv2_x and of a conv4_x block
    for i in (wide, deep):
        assert nodes[i]["k"] == 1 and not nodes[i]["relu"] and nodes[i]["cout"] == 4 * nodes[i]["cin"]
    assert nodes[fm[0]]["kind"] == "add" and ident[-2] not in fm
    return BF.defects() + [(("mx_wrong_dy", wide), wide - 6), (("mx_wrong_dy", deep), deep - 6),
                           (("mx_stale_dy", fm[0]), fm[0] - 8), (("mx_stale_dy", ident[-2]), ident[-2] - 8)]


@pytest.mark.parametrize("defect,first_node", defects(), ids=lambda v: str(v).replace(" ", ""))
def test_seeded_defect_exceeds_twice_the_bound(defect, first_node):
    r = result("reduced")
    D = r.oracle(defect=defect, first_node=first_node)
    hit = FO.moved(r.T, D, r.bound)
    print(defect, sorted(hit, key=lambda v: -v[1] / v[2])[:5])
    assert hit, (defect, "moves no tensor to twice its bound")


def mutations():
    """An identity block of conv4_x: its 1x1 expand reads the fp8 map of its add, and is handed the next add's instead (same
    shape; every writer of that map ran earlier in the walk); its first 1x1 accumulates onto the block's input, which the
    identity shortcut wrote just before, and is told to overwrite."""
    nodes, _, ident, _ = _graph()
    add, other = ident[-2], ident[-1]
    expand = nodes[add]["src"][0]
    first = expand - 2
    assert nodes[first]["src"] == nodes[add]["src"][1] and nodes[add]["cout"] == nodes[other]["cout"]
    return [("wrong_dy", expand, other), ("no_accumulate", first)]


@pytest.mark.parametrize("mutation", mutations(), ids=lambda v: str(v).replace(" ", ""))
def test_engine_mutation_fails_the_check(mutation):
    """The engine's REAL run, bent at one launch (same shapes, valid buffers): the stored operands are fetched again, T and R
    computed again, and the bound must refuse what came out -- the bound, not a precondition and not a NaN."""
    m = copy.copy(result("reduced"))                                     # run() rebinds what it fetches: the clean result stays
    m.mutation = mutation
    m.run()
    assert mutation[1] in [i for i, _ in m.launches]
    with pytest.raises(AssertionError, match="beyond 3 \\* rel_l2"):
        m.check("ResNet-50 SSD at 256, batch 3, mutation %s" % (mutation,))
