"""CPU suite: the plan of the ResNet-50 SSD512 trunk's fp8 data gradients after a training-mode fp8 forward
(resnet_engine.mxfp8_bwd_plan, mxfp8_plan(train=True)) and the host-side refusals of ssd_conv2d_bwd_data_mxfp8 -- no device is
touched."""
import ctypes


def _graph():
    from ssd_object_detection_amd.resnet_engine import resnet50_ssd512_graph
    return resnet50_ssd512_graph()


def _plan():
    from ssd_object_detection_amd.resnet_engine import mxfp8_bwd_plan
    g = _graph()
    return g, *mxfp8_bwd_plan(g)


def _flops(g):
    from ssd_object_detection_amd import ops
    size, flops = {-1: 512}, {}
    for i, nd in enumerate(g):
        src = nd["src"][0] if nd["op"] == "add" else nd["src"]
        ho = size[src] if nd["op"] not in ("conv", "pool3") else ops.same_pad(size[src], nd["k"], nd["stride"])[0]
        size[i] = ho
        if nd["op"] == "conv":
            flops[i] = ho * ho * nd["cout"] * nd["k"] * nd["k"] * nd["cin"]          # per image; a data gradient costs the same
    return flops


def test_plan_selects_the_37_data_gradients_of_the_rule():
    g, dgrad, _, _ = _plan()
    nonstem = [i for i, nd in enumerate(g) if nd["op"] == "conv" and nd["src"] >= 0]
    assert len(nonstem) == 52
    want = {i for i in nonstem if g[i]["stride"] == 1 and g[i]["k"] in (1, 3) and g[i]["cout"] % 128 == 0 and g[i]["cin"] % 32 == 0}
    assert dgrad == want and len(dgrad) == 37
    # four conv2_x layers (64 -> 256: the three expands and the projection shortcut) whose forward stays bf16
    from ssd_object_detection_amd.resnet_engine import mxfp8_plan
    fwd8 = mxfp8_plan(g)[0]
    assert sorted((g[i]["cin"], g[i]["cout"]) for i in dgrad - fwd8) == [(64, 256)] * 4
    # no stride-2 layer, no 64-wide reduce / 3x3 (conv2_x) among them
    assert all(g[i]["stride"] == 1 and g[i]["cout"] != 64 for i in dgrad)
    flops = _flops(g)
    share = sum(flops[i] for i in dgrad) / sum(flops[i] for i in nonstem)
    assert 0.68 <= share <= 0.74, share


def test_aliases():
    g, _, root, _ = _plan()
    for k, nd in enumerate(g):
        if nd["op"] != "add":
            continue
        a, sc = nd["src"]
        assert root[a] == k and root[k] == k
        assert root[sc] == (k if g[sc]["op"] == "conv" and not g[sc]["relu"] else sc)
    assert sum(1 for i in range(len(g)) if root[i] != i) == 13 + 3         # 13 expands, 3 projection shortcuts


# the maps whose fp8 form needs a standalone quantise pass: (map, its last writer, a bf16 kernel)
STANDALONE = {
    6: ("dgrad", 7), 10: ("dgrad", 11),                       # conv2_x adds: last read by the next 256 -> 64 reduce (Cout 64)
    15: ("dgrad", 16), 32: ("dgrad", 33),                     # first reduce of conv3_x / conv4_x: read by the 3x3/2
    57: ("dgrad", 58), 59: ("dgrad", 60), 61: ("dgrad", 62),  # the extra stages' 1x1: read by their 3x3/2
    63: ("dgrad", 64), 65: ("dgrad", 66),
}


def test_every_fp8_map_has_exactly_one_fp8_writer():
    g, dgrad, root, maps = _plan()
    assert set(maps) == {root[i] for i in dgrad}
    # every map an fp8 data gradient reads gets its fp8 form once: in the epilogue of its last writer, or in one standalone pass
    fused = {r: w for r, (kind, w) in maps.items() if kind == "fp8"}
    standalone = {r: (kind, w) for r, (kind, w) in maps.items() if kind != "fp8"}
    assert standalone == STANDALONE
    assert len(maps) == 36 and len(fused) == 27                    # 37 readers: conv2_x's first add feeds two
    writers = [w for w in fused.values()]
    assert len(writers) == len(set(writers)), "one data gradient writes two fp8 maps"
    for r, w in fused.items():
        assert w in dgrad and g[w]["src"] == r
    for r, (kind, w) in standalone.items():
        nd = g[w]
        assert kind == "dgrad" and nd["src"] == r and w not in dgrad and (nd["stride"] == 2 or nd["cout"] % 128), r
    # the writer is the LAST one of the reverse walk: the consumer with the lowest index (feature maps: heads write first)
    for r, (kind, w) in maps.items():
        consumers = [c for c, nd in enumerate(g) if (nd["src"] == r if nd["op"] != "add" else r in nd["src"])]
        writers = [c for c in consumers if not (g[c]["op"] == "add" and g[c]["src"][0] == r)]
        assert w == min(writers), (r, w, writers)
        assert all(w > i for i in dgrad if root[i] == r), "fp8 form written after its reader"


def test_train_forward_writes_every_bf16_map_backward_reads():
    from ssd_object_detection_amd.resnet_engine import mxfp8_plan
    g = _graph()
    fp8, inf = mxfp8_plan(g)
    fp8t, train = mxfp8_plan(g, train=True)
    assert fp8t == fp8
    conv_inputs = {nd["src"] for nd in g if nd["op"] == "conv" and nd["src"] >= 0}
    for i in range(len(g)):
        assert inf[i] <= train[i] and ("fp8" in train[i]) == ("fp8" in inf[i])
        assert train[i] == inf[i] | ({"bf16"} if i in conv_inputs else set()), i
        if g[i]["op"] == "add" or g[i]["feature"]:
            assert "bf16" in train[i]
    # what the training mode adds: the bf16 maps of the reduces / 3x3s that only fp8 layers read
    added = [i for i in range(len(g)) if train[i] != inf[i]]
    assert added and all(inf[i] == {"fp8"} for i in added)


def _lib():
    from ssd_object_detection_amd import _lib as L
    return L, L.lib()


def test_conv2d_bwd_data_mxfp8_refuses_on_the_host():
    L, lib = _lib()
    d = ctypes.c_void_p(0x1000)                                       # never dereferenced on these paths

    def call(dx=d, dx8=None, dxs=None, B=2, H=16, W=16, Cin=256, Cout=256, k=3, pt=1, pl=1, Ho=16, Wo=16, acc=0, dy8=d, wt8=d):
        return lib.ssd_conv2d_bwd_data_mxfp8(dy8, d, wt8, d, None, dx, dx8, dxs, B, H, W, Cin, Cout, k, pt, pl, Ho, Wo, acc, None)

    assert call(dx=None) == L.SSD_ERR_VALUE                          # no output
    assert call(dx=None, dx8=d, dxs=d, acc=1) == L.SSD_ERR_VALUE     # accumulate onto nothing
    assert call(dx8=d) == L.SSD_ERR_VALUE                            # q without its scales
    assert call(dxs=d) == L.SSD_ERR_VALUE
    assert call(dy8=None) == L.SSD_ERR_VALUE
    assert call(wt8=None) == L.SSD_ERR_VALUE
    assert call(B=0) == L.SSD_ERR_VALUE
    assert call(Ho=0) == L.SSD_ERR_VALUE
    assert call(pt=3) == L.SSD_ERR_VALUE                             # pads beyond the filter
    assert call(pt=-1) == L.SSD_ERR_VALUE
    assert call(H=40) == L.SSD_ERR_VALUE                             # windows beyond the map
    assert call(Cout=64) == L.SSD_ERR_UNSUPPORTED                    # the GEMM's K: whole 128-channel k-steps
    assert call(Cout=192) == L.SSD_ERR_UNSUPPORTED
    assert call(Cin=48) == L.SSD_ERR_UNSUPPORTED                     # whole 32-channel blocks
    assert call(Cin=48, dx=None, dx8=d, dxs=d) == L.SSD_ERR_UNSUPPORTED
    assert call(k=5, pt=2, pl=2) == L.SSD_ERR_UNSUPPORTED
    assert call(k=7, pt=3, pl=3) == L.SSD_ERR_UNSUPPORTED
    assert call(B=64, H=256, W=256, Cin=512, Ho=256, Wo=256) == L.SSD_ERR_UNSUPPORTED      # 2^31-byte dy8
    assert call(B=32, H=256, W=256, Cin=512, Cout=128, Ho=256, Wo=256) == L.SSD_ERR_UNSUPPORTED   # 2^31-byte bf16 dx
    assert call(Cout=16384, Cin=131072, k=1, pt=0, pl=0, B=1, H=1, W=1, Ho=1, Wo=1) == L.SSD_ERR_UNSUPPORTED
