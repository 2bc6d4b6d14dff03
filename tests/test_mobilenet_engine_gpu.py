"""GPU: SSDEngine on the MobileNet-v1 SSD300 graph (engine.MOBILENET_V1_SSD300_TRUNK), forward and backward, against
tests/mobilenet_oracle.py.

Forward: the rule tests/test_engine_gpu.py applies to SSD300 -- rel_l2 < 1e-2 of loc and conf against the bf16-emulating CPU
forward run on the engine's own bf16 filters -- at the full geometry (batch 1) and at the five-level geometry 140 (batch 2: maps
70, 35, 18, 9, 5, 3, 2, 1, so the stride-2 depthwise nodes see even and odd maps).

Backward: teacher-forced, as tests/test_engine_forced_gpu.py does it.  Every data-dependent decision is taken from the
engine's own forward (the stored maps are the masks; the sign bytes must equal them), gradient maps and tensors are NaN and the
padding between tensors a fixed pattern before backward(); each parameter gradient and each gradient map must lie within
3 * rel_l2(R, T) + 1e-3 (forced_oracle.bounds).  Feature map 0 feeds a head AND a stride-2 depthwise node: its gradient is head
first, the depthwise data gradient accumulated onto it.  The three wiring errors this graph invites -- that data gradient
overwrites the head's part, the head's part is missing, a 1x1 layer's data gradient is not masked by the depthwise ReLU in front
of it -- are shown to move a named tensor beyond twice its bound."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict as S                                        # noqa: E402
from tests import forced_oracle as FO                                # noqa: E402
from tests import mobilenet_oracle as MO                             # noqa: E402

CLASSES = 81
RESULTS = {}
GRIDS = {300: (19, 10, 5, 3, 2, 1), 140: (9, 5, 3, 2, 1)}


def build(size, sparse_heads=None, seed=7):
    from ssd_object_detection_amd.engine import SSDEngine, MOBILENET_V1_SSD300_TRUNK as T, MOBILENET_V1_SSD300_NUM_PRIORS as P
    trunk, pri = (T, P) if size == 300 else (T[:-2], P[:5])
    e = SSDEngine(classes=CLASSES, seed=seed, in_size=size, trunk=trunk, num_priors=pri, sparse_heads=sparse_heads)
    assert e.grids == tuple((h, h) for h in GRIDS[size])
    return e


def plain(e):
    e.overlap_heads, e.chain, e.relu_bits, e.fuse_unpool, e.fuse_first, e.skip_fullres = False, set(), None, None, False, False
    return e


class Forced(FO.Forced):
    def written_maps(self):
        return list(range(1, len(self.engine.nodes) + 1))

    def stored_forward(self):
        c = self.c
        return [c["acts"][a].cpu() for a in range(len(self.engine.nodes) + 1)], {}, None

    def walk(self, *args, **kw):
        return MO.backward_chain(*args, **kw)

    def check_forward_state(self):
        """exact preconditions: the sign bytes are those of the stored maps, the depthwise outputs' included"""
        e, c = self.engine, self.c
        dw_out = {i + 1 for i, nd in enumerate(e.nodes) if nd["kind"] == "dwconv"}
        if e.relu_bits is not None:
            assert dw_out <= e.bits_valid, "every depthwise node writes sign bytes"
        for a in sorted(e.bits_valid):
            assert torch.equal(c["rbits"][a].cpu(), S.pack_bits(self.stored[a] > 0)), "sign bytes of activation %d" % a
        alive = {a: float((self.stored[a] > 0).float().mean()) for a in range(1, len(e.nodes) + 1)}
        assert min(alive.values()) >= 0.1, sorted(alive.items(), key=lambda kv: kv[1])[:3]


def result(key):
    if key not in RESULTS:
        scale = (1.0, 2.0, 4.0, 8.0, 16.0)        # the deeper levels' few pixels weigh as much as level 0's (see test_engine_forced_gpu.py)
        if key == "140":
            RESULTS[key] = Forced(build(140), 2, 17, level_scale=scale)
        elif key == "140-off":
            RESULTS[key] = Forced(plain(build(140, sparse_heads=False)), 2, 17, level_scale=scale)
        else:
            raise KeyError(key)
    return RESULTS[key]


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("size,B", [(300, 1), (140, 2)])
def test_forward_against_the_oracle(size, B):
    import ssd_object_detection_amd.ops as ops
    e = build(size, seed=3)
    x = ops.image_prep(torch.rand((B, size, size, 3), generator=torch.Generator().manual_seed(1)).cuda())
    loc, conf = e.forward(x)
    torch.cuda.synchronize()
    A = sum(h * h * n for h, n in zip(GRIDS[size], e.num_priors))
    assert loc.shape == (B, A, 4) and conf.shape == (B, A, CLASSES) and (size != 300 or A == 2268)
    w = {k: v.float() for k, v in FO.engine_weights(e).items()}
    keep = {}
    loc_r, conf_r = MO.forward(e.trunk, e.num_priors, CLASSES, w, x.float().cpu(), keep=keep)
    assert min(MO.alive(keep).values()) >= 0.1
    el, ec = FO.rel_l2(loc.float().cpu(), loc_r), FO.rel_l2(conf.float().cpu(), conf_r)
    print("forward %d batch %d: rel_l2 loc %.3e conf %.3e" % (size, B, el, ec))
    assert el < 1e-2 and ec < 1e-2, (el, ec)
    c = e._acts(B)
    for a in sorted(e.bits_valid):
        assert torch.equal(c["rbits"][a].cpu(), S.pack_bits(c["acts"][a].cpu() > 0)), "sign bytes of activation %d" % a
    assert {i + 1 for i, nd in enumerate(e.nodes) if nd["kind"] == "dwconv"} <= e.bits_valid
    with pytest.raises(NotImplementedError, match="depthwise"):
        e.forward(x, "mxfp8")
    assert e.last_forward == "bf16"                                          # refused before anything ran: backward() still allowed


def test_full_geometry_chain_and_launch_trace():
    """One forward + backward at 300: the planned chain (nodes 28 .. 34) is what launches -- nothing was refused, and the trace
    names the chain once per direction with seven layers; node 27 is an ordinary launch."""
    import ssd_object_detection_amd.ops as ops
    from tests.launch_trace import Recorder
    e = build(300, seed=3)
    g = torch.Generator().manual_seed(2)
    x = ops.image_prep(torch.rand((1, 300, 300, 3), generator=g).cuda())
    dloc = (torch.randn((1, e.A, 4), generator=g) * 1e-3).bfloat16().cuda()
    dconf = (torch.randn((1, e.A, CLASSES), generator=g) * 1e-3).bfloat16().cuda()
    assert e.chain_start == 28 and e.sparse_heads
    with Recorder() as rec:
        e.forward(x)
        e.backward(dloc, dconf)
        torch.cuda.synchronize()
    assert e.chain == {"fwd", "bwd"}
    chains = [call for call in rec.calls if call[0] == "ssd_conv_chain"]
    assert [call[3] for call in chains] == [7, 7], [call[3:] for call in chains]
    names = [call[0] for call in rec.calls]
    n_dw = sum(1 for nd in e.nodes if nd["kind"] == "dwconv")
    assert names.count("ssd_dwconv3x3_fwd_relubits") == n_dw == 13 and names.count("ssd_dwconv3x3_fwd") == 0
    assert names.count("ssd_dwconv3x3_bwd_weight") == 13
    assert names.count("ssd_dwconv3x3_bwd_data_bits") + names.count("ssd_dwconv3x3_bwd_data") == 13
    assert bool(torch.isfinite(e.grad).all())


# ---------------------------------------------------------------- teacher-forced backward
def test_reduced_140_default_switches():
    r = result("140")
    e = r.engine
    assert e.chain_start == 27 and e.chain == {"fwd", "bwd"} and e.sparse_heads and e.overlap_heads and e.relu_bits is not None
    assert [(nd["hin"], nd["hout"]) for nd in e.nodes if nd["kind"] == "dwconv" and nd["stride"] == 2] == [(70, 35), (35, 18), (18, 9), (9, 5)]
    r.check("MobileNet-v1 trunk[:-2] at 140, batch 2")


def test_reduced_140_everything_off():
    r = result("140-off")
    e = r.engine
    assert not e.sparse_heads and e.head_grad_buffers(2) is None
    assert e.overlap_heads is False and not e.chain and e.relu_bits is None and not e.bits_valid
    r.check("MobileNet-v1 trunk[:-2] at 140, batch 2, everything off")


def test_sign_byte_and_relu_src_paths_give_equal_bits():
    """Default switches: the depthwise data gradients masked from the sign bytes and from the bf16 maps give the same bits."""
    r = result("140")
    e, c = r.engine, r.c
    runs, default = [], e.dw_dgrad_bits
    for bits in (True, False):
        e.dw_dgrad_bits = bits
        e.forward(r.x)
        e.backward(r.dloc.cuda(), r.dconf.cuda())
        torch.cuda.synchronize()
        runs.append(FO.engine_grads(e, c, r.maps)[0])
    e.dw_dgrad_bits = default
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]), [k for k in runs[0] if not torch.equal(runs[0][k], runs[1][k])]


# feature map 0 is activation 23 (node 22's output), read by head 0 and by node 23 (depthwise, stride 2); node 24 is the 1x1 layer
# behind it: its data gradient flows into activation 24, masked by node 23's ReLU
DEFECTS = [(("overwrite", (23, 23)), 20, "gact23"), (("no_head", 0), 20, "gact23"), (("no_mask", 24), 20, "gact24")]


@pytest.mark.parametrize("defect,first_node,named", DEFECTS, ids=lambda v: str(v).replace(" ", ""))
def test_seeded_defect_exceeds_twice_the_bound(defect, first_node, named):
    r = result("140")
    assert r.engine.fm[0][0] == 22 and r.engine.nodes[23]["kind"] == "dwconv" and r.engine.nodes[24]["k"] == 1
    D = r.oracle(defect=defect, first_node=first_node)
    hit = FO.moved(r.T, D, r.bound)
    print(defect, sorted(hit, key=lambda v: -v[1] / v[2])[:5])
    assert named in [h[0] for h in hit], (defect, "does not move %s to twice its bound" % named)


def test_two_backward_calls_give_the_same_bits():
    r = result("140")
    e, c = r.engine, r.c
    e.forward(r.x)
    runs = []
    for _ in range(2):
        e.backward(r.dloc.cuda(), r.dconf.cuda())
        torch.cuda.synchronize()
        runs.append([e.grad.clone().view(torch.int32)] + [c["gacts"][a].clone().view(torch.int16) for a in r.maps])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    got, _ = FO.engine_grads(e, c, r.maps)
    assert all(torch.equal(got[k], r.got[k]) for k in got), "differs from the first (poisoned) run"
