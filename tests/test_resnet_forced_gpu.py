"""GPU: ResNet50SSDEngine.backward as a composition, against the teacher-forced float64 oracle (tests/forced_oracle.py), as
tests/test_engine_forced_gpu.py does for the VGG-style engine: masks, routes and operands from the engine's own bf16 forward, the
bound of a tensor 3 * rel_l2(R, T) + 1e-3 from the oracle's storage model, every gradient NaN and the padding patterned before
backward().  The walk has aliased maps at the adds (block output and projection shortcut read the add's gradient in place),
identity shortcuts that accumulate and feature maps that feed a head, the next block and its shortcut: the seeded defects are
those, on a 256 x 256 input at batch 3 (levels 32, 16, 8, 4, 2, 1, 1)."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict as S                                        # noqa: E402
from tests import forced_oracle as FO                                # noqa: E402

CLASSES = 81
RESULTS = {}


class Forced(FO.Forced):
    def written_maps(self):
        # the two linear inputs of an add read the add's gradient in place: their own buffers stay as they were
        e = self.engine
        return [a for a in range(1, len(e.nodes) + 1) if e.mx_groot[a - 1] == a - 1]

    def stored_forward(self):
        c = self.c
        return [t.cpu() for t in c["acts"]], {i: FO.unpack_codes(w.cpu()) for i, w in c["pool3_code"].items()}, None

    def walk(self, *args, **kw):
        return FO.backward_graph(*args, **kw)

    def check_forward_state(self):
        e, c = self.engine, self.c
        assert not e.bits_valid and e.relu_bits is None                 # every mask of this engine comes from a stored bf16 map
        for p, nd in enumerate(e.nodes):
            if nd["kind"] == "pool3":
                y, want = S.ref_pool(self.stored[nd["src"] + 1].float(), 3, 2, nd["pt"], nd["pl"], nd["hout"], nd["hout"], 15)
                assert torch.equal(self.stored[p + 1].float(), y), "pooled map of node %d" % p
                assert torch.equal(c["pool3_code"][p].cpu(), S.pack_codes(want)), "winner codes of node %d" % p


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
    r.check("ResNet-50 SSD512 batch 1")


def test_reduced_geometry():
    r = result("reduced")
    r.check("ResNet-50 SSD at 256, batch 3")


def _adds(nodes):
    proj = [i for i, nd in enumerate(nodes) if nd["kind"] == "add" and not nodes[nd["src"][1]]["relu"]]
    ident = [i for i, nd in enumerate(nodes) if nd["kind"] == "add" and nodes[nd["src"][1]]["relu"]]
    return proj, ident


def defects():
    """(defect, first_node) on ResNet50SSDEngine's node list, which needs no device"""
    from ssd_object_detection_amd.resnet_engine import resnet50_ssd512_graph
    nodes = [dict(nd, kind=nd["op"]) for nd in resnet50_ssd512_graph()]
    proj, ident = _adds(nodes)
    fm = [i for i, nd in enumerate(nodes) if nd["feature"]]
    out = [(("no_head", lvl), max(0, fm[lvl] - 8)) for lvl in range(len(fm))]
    a3 = ident[3]                                                        # an identity block of conv3_x
    conv3x3 = nodes[a3]["src"][0] - 1                                    # its 3x3: reads a ReLU output
    wide, deep = nodes[ident[0]]["src"][0] - 1, nodes[ident[-1]]["src"][0] - 1   # 3x3 / stride 1, cin == cout, behind a ReLU: conv2_x, conv4_x
    for c3 in (wide, deep):
        assert nodes[c3]["k"] == 3 and nodes[c3]["stride"] == 1 and nodes[c3]["cin"] == nodes[c3]["cout"] and nodes[nodes[c3]["src"]]["relu"]
    out += [(("mask_output", wide), wide - 3), (("mask_output", deep), deep - 3), (("no_mask", wide), wide - 3),
            (("no_mask", conv3x3), conv3x3 - 3), (("no_mask", fm[1] + 1), fm[1] - 3), (("pool_first", 1), 0),
            (("wgrad_before_head", 2), fm[2] - 1),
            (("no_identity", ident[-1]), ident[-1] - 8), (("no_identity", ident[0]), ident[0] - 8),
            (("no_projection", proj[-1]), proj[-1] - 8), (("no_projection", proj[0]), 0),
            (("no_shortcut_mask", ident[-1]), ident[-1] - 8), (("no_shortcut_mask", a3), a3 - 8)]
    # feature map 0 (the last add of conv3_x) feeds the head, conv4_x's projection shortcut and its first 1x1, which comes last
    # in the walk: overwriting there loses the other two
    consumers = [i for i, nd in enumerate(nodes) if nd["kind"] == "conv" and nd["src"] == fm[0]]
    assert len(consumers) == 2
    out += [(("overwrite", (fm[0] + 1, consumers[0])), fm[0] - 4), (("overwrite", (fm[1] + 1, fm[1] + 1)), fm[1] - 4)]
    return out


@pytest.mark.parametrize("defect,first_node", defects(), ids=lambda v: str(v).replace(" ", ""))
def test_seeded_defect_exceeds_twice_the_bound(defect, first_node):
    r = result("reduced")
    D = r.oracle(defect=defect, first_node=first_node)
    hit = FO.moved(r.T, D, r.bound)
    print(defect, sorted(hit, key=lambda v: -v[1] / v[2])[:5])
    assert hit, (defect, "moves no tensor to twice its bound")
