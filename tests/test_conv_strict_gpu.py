"""GPU: the convolution, pooling, element-wise and MX-fp8 entry points under the strict harness (tests/strict.py).

Operands are small integers, so every expected output is exact whatever the rounding mode, summation order or split count:
each comparison below is torch.equal against the torch CPU fp32 reference (tests/test_strict_cpu.py asserts the regime of
every case used here, and fp32 == float64 for the small ones).  Inputs, outputs and workspace live in strict.Arena: 1 MiB guards
touching each tensor, a workspace of exactly the bytes asked for, every operation run under two poisons -- a store outside the
documented extent, an element never written, an input modified, a read of a guard or of unwritten scratch that reaches the
result are all failures, and the message names the tensor and the element.  Where an entry point refuses a shape by contract the
refusal is the expected result of that case and is asserted (through the dispatch query, a host function)."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                                                         # noqa: E402
from tests.conv_cases import CASES, FULL_SIZE_CASES, RESNET_CASES, WS_BYTES, plan_name, plan_names   # noqa: E402

BF, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


def _tensors(r):
    for v in r.values() if isinstance(r, dict) else r:
        if torch.is_tensor(v):
            yield v
        elif isinstance(v, (dict, list)):
            yield from _tensors(v)


def arena_for(r, *ws_bytes):
    """an arena that holds every operand and output of the reference dict `r` (outputs are at most as large as their fp32
    references), the workspaces, and the guards of up to 128 tensors"""
    total = sum(t.numel() * t.element_size() for t in _tensors(r))
    return strict.Arena("cuda", 2 * total + sum(ws_bytes) + 128 * (2 * strict.GUARD + 2 * strict.ALIGN))


class knobs:
    """Set development knobs for a block and put their defaults back."""
    DEFAULTS = {"SSD_CONV_PATCH_FLAT": 1, "SSD_CONV_PATCH_ROWFLAT": 1, "SSD_CONV_P512": 1, "SSD_WGRAD_PATCH_SHAPE": -1}

    def __init__(self, L, **kv):
        self.L, self.kv = L, kv

    def __enter__(self):
        for k, v in self.kv.items():
            assert self.L.ssd_dev_knob(k.encode(), v) == 0

    def __exit__(self, *exc):
        for k in self.kv:
            self.L.ssd_dev_knob(k.encode(), self.DEFAULTS[k])


# ---------------------------------------------------------------- forward, data gradient, weight gradient, transpose
def run_conv_case(ops, L, case, r=None, forward=True, dgrad=True, wgrad=True):
    B, H, W, Cin, Cout, k, stride, mode = case[:8]
    if r is None:
        r = strict.conv_reference(case)
        strict.check_conv_regime(case, r)
    Ho, Wo, pt, pl = r["geom"]
    cp = (Cout + 7) // 8 * 8
    a = arena_for(r, 2 * WS_BYTES, 2 * L.ssd_conv2d_bwd_weight_workspace_bytes(B, Ho, Wo, Cin, Cout, cp, k))
    x, w, bias = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias")
    dyp, mask = a.put(r["dy_pad"], "dy"), a.put(r["mask_src"], "relu_src")
    ws = a.workspace()
    if forward:
        y = a.out((B, Ho, Wo, Cout), BF, "y")
        for relu in (True, False):
            a.run(lambda: ops.conv2d_fwd(x, w, bias, stride, pt, pl, Ho, Wo, relu, out=y, ws=ws),
                  [(y, r["y_relu" if relu else "y"].to(BF))])
        wt_out = a.out((Cin, k, k, cp), BF, "w_t")
        a.run(lambda: ops.weight_transpose(w, cp, out=wt_out), [(wt_out, r["w_t"])])
    if dgrad:
        w_t = a.put(r["w_t"], "w_t (operand)")
        dx = a.out((B, H, W, Cin), BF, "dx")
        a.run(lambda: ops.conv2d_bwd_data(dyp, w_t, None, (B, H, W, Cin), stride, pt, pl, out=dx, ws=ws), [(dx, r["dx"].to(BF))])
        acc = a.inout(r["base"], "dx (accumulated onto)")
        a.run(lambda: ops.conv2d_bwd_data(dyp, w_t, mask, (B, H, W, Cin), stride, pt, pl, accumulate=True, out=acc, ws=ws),
              [(acc, r["dx_acc"].to(BF))])
    if wgrad:
        dw, db = a.out((Cout, k, k, Cin), F32, "dw"), a.out((Cout,), F32, "dbias")
        a.run(lambda: ops.conv2d_bwd_weight(x, dyp, Cout, k, stride, pt, pl, dw=dw, dbias=db, ws=ws), [(dw, r["dw"]), (db, r["dbias"])])
        a.run(lambda: ops.conv2d_bwd_weight(x, dyp, Cout, k, stride, pt, pl, dw=dw, want_bias=False, ws=ws), [(dw, r["dw"])])


@pytest.mark.parametrize("case", CASES, ids=[str(c[:8]) for c in CASES])
def test_conv_strict(ops, L, case):
    assert plan_names(case[:8]) == case[8], "the dispatch rules moved: this case no longer tests the kernels it names"
    run_conv_case(ops, L, case)


@pytest.mark.parametrize("case", FULL_SIZE_CASES, ids=[str(c[:8]) for c in FULL_SIZE_CASES])
def test_conv_strict_large_problem_kernels(ops, L, case):
    """k_pw_gemm, k_conv_igemm_8ph, the 256-row LDS-DMA tiles, k_conv_wgrad_tile with and without the wide reduction: at the
    smallest batch for which the dispatch query still names them."""
    B = strict.smallest_batch(case)
    print("batch used for %s: %d" % (str(case[:8]), B))
    case = (B,) + tuple(case[1:])
    assert plan_names(case[:8]) == case[8]
    run_conv_case(ops, L, case)


@pytest.mark.parametrize("case", RESNET_CASES, ids=[str(c[:8]) for c in RESNET_CASES])
def test_conv_strict_resnet_shapes(ops, L, case):
    """The regimes of the ResNet-50 SSD512 trunk (tests/conv_cases.py: the 7x7 stem, 1x1 stride 2, one- and two-tile k loops
    of the 8-phase kernel, the 512-pixel kernel in plain block mode, the extras' 4x4 .. 1x1 maps).  The engine never asks for
    the stem's data gradient; the entry point documents no limit on the kernel size, so it is run here all the same.  A case
    whose data gradient the library refuses names the refusal ("error -2": SSD_ERR_VALUE, a bad argument, before any launch)
    where the others name a kernel; the call must then raise and write nothing."""
    assert plan_names(case[:8]) == case[8], "the dispatch rules moved: this case no longer tests the kernels it names"
    refused = case[8][1].startswith("error")
    run_conv_case(ops, L, case, dgrad=not refused)
    if refused:
        from ssd_object_detection_amd._lib import SSD_ERR_VALUE
        assert case[8][1] == "error %d" % SSD_ERR_VALUE
        B, H, W, Cin, Cout, k, stride, mode = case[:8]
        r = strict.conv_reference(case)
        a = arena_for(r, 2 * WS_BYTES)
        dyp, w_t, ws = a.put(r["dy_pad"], "dy"), a.put(r["w_t"], "w_t"), a.workspace()
        dx = a.out((B, H, W, Cin), BF, "dx")

        def call():
            with pytest.raises(ValueError):
                ops.conv2d_bwd_data(dyp, w_t, None, (B, H, W, Cin), stride, r["geom"][2], r["geom"][3], out=dx, ws=ws)
        a.run(call, [])


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_wgrad_patch_block_shapes_strict(ops, L, shape):
    case = (2, 23, 45, 64, 80, 3, 1, "same")
    with knobs(L, SSD_WGRAD_PATCH_SHAPE=shape):
        name = plan_name(L, L.ssd_conv2d_bwd_weight_plan(2, 23, 45, 64, 80, 80, 3, 1, 1, 1, 23, 45))
        assert name.startswith("k_conv3x3_wgrad_patch<%s>" % ("16,2", "6,5", "10,3")[shape]), name
        run_conv_case(ops, L, case, forward=False, dgrad=False)


@pytest.mark.parametrize("case", [(2, 30, 30, 64, 64), (3, 17, 23, 128, 96), (1, 38, 38, 64, 136)], ids=str)
def test_patch_strip_blocks_forced_strict(ops, L, case):
    B, H, W, Cin, Cout = case
    with knobs(L, SSD_CONV_PATCH_FLAT=2):
        fwd = plan_name(L, L.ssd_conv2d_fwd_plan(B, H, W, Cin, Cout, 3, 1, 1, 1, H, W, 0, WS_BYTES))
        dg = plan_name(L, L.ssd_conv2d_bwd_data_plan(B, H, W, Cin, (Cout + 7) // 8 * 8, 3, 1, 1, 1, H, W, 1, WS_BYTES))
        # (the knob moves the patch kernels only: 64 -> 64 keeps its register-weight kernel, 96 in-channels the generic GEMM)
        assert fwd.endswith("+flat") or dg.endswith("+flat"), (fwd, dg)
        run_conv_case(ops, L, case + (3, 1, "same"), wgrad=False)


# ---------------------------------------------------------------- sign bytes
@pytest.mark.parametrize("case", [(2, 40, 40, 8, 64, 3, 1, "same"), (2, 30, 30, 64, 64, 3, 1, "same")], ids=str)
def test_relubits_strict(ops, L, case):
    B, H, W, Cin, Cout, k, stride, mode = case
    r = strict.conv_case(case)
    Ho, Wo, pt, pl = r["geom"]
    a = arena_for(r, 2 * WS_BYTES)
    x, w, bias, ws = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.workspace()
    y, bits = a.out((B, Ho, Wo, Cout), BF, "y"), a.out((B, Ho, Wo, Cout // 8), U8, "relu_bits")
    a.run(lambda: ops.conv2d_fwd_relubits(x, w, bias, stride, pt, pl, Ho, Wo, bits, out=y, ws=ws),
          [(y, r["y_relu"].to(BF)), (bits, r["y_bits"])])
    if Cin < 64:
        return                                              # no data gradient w.r.t. the image
    dyp, w_t, xbits = a.put(r["dy_pad"], "dy"), a.put(r["w_t"], "w_t"), a.put(r["x_bits"], "mask bits")
    dx = a.out((B, H, W, Cin), BF, "dx")
    a.run(lambda: ops.conv2d_bwd_data_bits(dyp, w_t, xbits, (B, H, W, Cin), stride, pt, pl, out=dx, ws=ws), [(dx, r["dx_masked"].to(BF))])
    acc = a.inout(r["base"], "dx (accumulated onto)")
    a.run(lambda: ops.conv2d_bwd_data_bits(dyp, w_t, xbits, (B, H, W, Cin), stride, pt, pl, accumulate=True, out=acc, ws=ws),
          [(acc, r["dx_acc"].to(BF))])


def test_relubits_refused_on_split_k_strict(ops, L):
    """3x3 VALID at 5x5 resolves to split-K + finalize, which carries no sign bytes: refused, and nothing is written"""
    case = (4, 5, 5, 128, 256, 3, 1, "valid")
    r = strict.conv_case(case)
    a = arena_for(r, 2 * WS_BYTES)
    x, w, bias, ws = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.workspace()
    y, bits = a.out((4, 3, 3, 256), BF, "y"), a.out((4, 3, 3, 32), U8, "relu_bits")

    def refused():
        with pytest.raises(NotImplementedError):
            ops.conv2d_fwd_relubits(x, w, bias, 1, 0, 0, 3, 3, bits, out=y, ws=ws)
    a.run(refused, [])


# ---------------------------------------------------------------- convolution + pooling in one call
def run_fwd_pool(ops, L, case, same, **kv):
    B, H, W, Cin, Cout, k, stride, mode = case
    r = strict.fwd_pool_case(case, same)
    Ho, Wo, pt, pl = r["geom"]
    Hp, Wp = r["yp"].shape[1:3]
    a = arena_for(r, 2 * WS_BYTES)
    x, w, bias, ws = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.workspace()
    y, yp, code = a.out((B, Ho, Wo, Cout), BF, "y"), a.out((B, Hp, Wp, Cout), BF, "y_pool"), a.out((B, Hp, Wp, Cout // 8), I32, "pool_code")
    want = [(y, r["y_relu"].to(BF)), (yp, r["yp"].to(BF)), (code, strict.pack_codes(r["code"]))]
    with knobs(L, **kv):
        fused = "poolfused" in plan_name(L, L.ssd_conv2d_fwd_plan(B, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo, 1, WS_BYTES))
        a.run(lambda: ops.conv2d_fwd_pool(x, w, bias, stride, pt, pl, Ho, Wo, True, same, out=y, pool_out=yp, code=code, ws=ws), want)
        if fused:               # y == NULL: the full-resolution map is not stored
            a.run(lambda: ops.conv2d_fwd_pool(x, w, bias, stride, pt, pl, Ho, Wo, True, same, pool_out=yp, code=code, ws=ws, pool_only=True),
                  want[1:])
        else:                   # no kernel pools this layer in its epilogue: refused before anything is launched
            def refused():
                with pytest.raises(ValueError):
                    ops.conv2d_fwd_pool(x, w, bias, stride, pt, pl, Ho, Wo, True, same, pool_out=yp, code=code, ws=ws, pool_only=True)
            a.run(refused, [])
    return fused


@pytest.mark.parametrize("case,same", [((1, 33, 33, 64, 96, 3, 1, "same"), True), ((2, 19, 19, 128, 128, 3, 1, "same"), False)], ids=str)
def test_conv_fwd_pool_strict(ops, L, case, same):
    run_fwd_pool(ops, L, case, same)


def test_conv_fwd_pool_p512_strict(ops, L):
    """SSD_CONV_P512=2: the 512-pixel kernel's pooling epilogue on a 64-channel layer, at the smallest map of its test"""
    with knobs(L, SSD_CONV_P512=2):
        assert plan_name(L, L.ssd_conv2d_fwd_plan(2, 33, 33, 64, 128, 3, 1, 1, 1, 33, 33, 1, WS_BYTES)).startswith("k_conv3x3_p512")
    assert run_fwd_pool(ops, L, (2, 33, 33, 64, 128, 3, 1, "same"), True, SSD_CONV_P512=2)


# ---------------------------------------------------------------- data gradient carried through the pooling
def test_bwd_data_unpool_strict(ops, L):
    B, Hf, Wf, C, Cout, same = 2, 37, 45, 64, 128, True
    r = strict.unpool_case(B, Hf, Wf, C, Cout, same)
    H, W = r["geom"][:2]
    a = arena_for(r, 2 * WS_BYTES)
    dy, w_t, mask, ws = a.put(r["dy_pad"], "dy"), a.put(r["w_t"], "w_t"), a.put(r["mask_src"], "relu_src"), a.workspace()
    code = a.put(strict.pack_codes(r["code"]), "pool_code")
    full, pooled = a.out((B, Hf, Wf, C), BF, "dx_full"), a.out((B, H, W, C), BF, "dx_pooled")
    a.run(lambda: ops.conv2d_bwd_data_unpool(dy, w_t, None, code, (B, Hf, Wf, C), out=full, ws=ws), [(full, r["dfull"].to(BF))])
    a.run(lambda: ops.conv2d_bwd_data_unpool(dy, w_t, mask, code, (B, Hf, Wf, C), out=full, ws=ws, pooled_out=pooled),
          [(full, r["dfull_masked"].to(BF)), (pooled, r["dx_masked"].to(BF))])


def test_bwd_weight_unpooled_strict(ops, L):
    B, H, W, Cin, Cout, same = 1, 16, 16, 64, 64, False
    r = strict.wgrad_unpooled_case(B, H, W, Cin, Cout, same)
    strict.check_regime(r)
    nbytes = L.ssd_conv2d_bwd_weight_unpooled_workspace_bytes(B, H, W, Cin, Cout, H // 2, W // 2)
    assert nbytes > 0
    a = arena_for(r, 2 * nbytes)
    x, dp, code, ws = a.put(r["x"], "x"), a.put(r["dp"], "dpool"), a.put(strict.pack_codes(r["code"]), "pool_code"), a.workspace()
    dw, db = a.out((Cout, 3, 3, Cin), F32, "dw"), a.out((Cout,), F32, "dbias")
    a.run(lambda: ops.conv2d_bwd_weight_unpooled(x, dp, code, dw=dw, dbias=db, ws=ws), [(dw, r["dw"]), (db, r["dbias"])])


@pytest.mark.parametrize("shape", [(3, 37, 52), (1, 16, 16)], ids=str)
def test_bwd_data_wgrad_first_strict(ops, L, shape):
    B, H, W = shape
    r = strict.wgrad_first_case(B, H, W)
    strict.check_regime(r)
    a = arena_for(r, 2 * L.ssd_conv2d_bwd_data_wgrad_first_workspace_bytes(B, H, W))
    dy, w_t, bits, img, ws = a.put(r["dy"], "dy"), a.put(r["w_t"], "w_t"), a.put(r["bits"], "relu_bits"), a.put(r["img"], "image"), a.workspace()
    dw, db = a.out((64, 3, 3, 8), F32, "dw0"), a.out((64,), F32, "dbias0")
    a.run(lambda: ops.conv2d_bwd_data_wgrad_first(dy, w_t, bits, img, dw=dw, dbias=db, ws=ws), [(dw, r["dw"]), (db, r["dbias"])])


def test_bwd_weight_batched_strict(ops, L):
    r = strict.wgrad_batched_case(16)
    strict.check_regime(r)
    a = arena_for(r, 1 << 26)
    ws, layers, want = a.workspace(), [], []
    for i, l in enumerate(r["layers"]):
        x, dy = a.put(l["x"], "x%d" % i), a.put(l["dy"], "dy%d" % i)
        dw, db = a.out(tuple(l["dw"].shape), F32, "dw%d" % i), a.out((l["cout"],), F32, "dbias%d" % i)
        layers.append((x, dy, l["cout"], l["k"], l["s"], l["pt"], l["pt"], dw, db))
        want += [(dw, l["dw"]), (db, l["dbias"])]
    a.run(lambda: ops.conv2d_bwd_weight_batched(layers, ws=ws), want)


# ---------------------------------------------------------------- heads
# the heads of the ResNet-50 SSD512's small maps (1x1, 2x2, 4x4: M = 2 .. 32 rows of a 128-row tile), of its 16x16 map, and a
# head wide and tall enough for the generic kernel WITHOUT split-K (>= 160 tiles of 128x128; 340 filters: EPI_HEAD's scattered
# epilogue over three channel tiles, the last one ragged), with the kernel each must reach
RESNET_HEADS = {(2, 1, 1, 256, 4, 1): "k_conv_igemm_dma<128,128>+splitk", (2, 2, 2, 256, 4, 1): "k_conv_igemm_dma<128,128>+splitk",
                (2, 4, 4, 256, 6, 1): "k_conv_igemm_dma<128,128>+splitk", (2, 16, 16, 512, 6, 1): "k_conv3x3_patch32<128>+flat",
                (2, 60, 58, 64, 4, 1): "k_conv_igemm_dma<128,128>"}


@pytest.mark.parametrize("shape", [(2, 5, 5, 64, 6, 1), (2, 19, 19, 256, 4, 1), (2, 19, 19, 1024, 6, 1), (3, 19, 19, 256, 6, 2)]
                         + list(RESNET_HEADS), ids=str)
def test_head_fwd_and_grad_pack_strict(ops, L, shape):
    """the three shapes of test_head_fwd_layout, SSD_CONV_P512=2 at the smallest map of its head test, and RESNET_HEADS"""
    B, H, W, Cin, n, p512 = shape
    if shape in RESNET_HEADS:
        assert plan_name(L, L.ssd_conv2d_head_fwd_plan(B, H, W, Cin, n, 81, WS_BYTES)) == RESNET_HEADS[shape], \
            "the dispatch rules moved: this head no longer tests the kernel it names"
    r = strict.head_case(B, H, W, Cin, n)
    strict.check_regime(r)
    C, off, npad, A = r["classes"], r["off"], r["npad"], r["loc"].shape[1]
    a = arena_for(r, 2 * WS_BYTES)
    x, w, bias, ws = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.workspace()
    loc, conf = a.out((B, A, 4), BF, "loc"), a.out((B, A, C), BF, "conf")
    with knobs(L, SSD_CONV_P512=p512):
        if p512 == 2:
            assert plan_name(L, L.ssd_conv2d_head_fwd_plan(B, H, W, Cin, n, C, WS_BYTES)) == "k_conv3x3_p512+flat"
        a.run(lambda: ops.conv2d_head_fwd(x, w, bias, loc, conf, n, C, off, ws=ws),
              [(loc, r["loc"].to(BF), r["loc_written"]), (conf, r["conf"].to(BF), r["conf_written"])])
    dloc, dconf = a.put(r["dloc"], "dloc"), a.put(r["dconf"], "dconf")
    packed = a.out((B, H * W, npad), BF, "packed head gradient")
    a.run(lambda: ops.head_grad_pack(dloc, dconf, H * W, n, C, npad, off, out=packed), [(packed, r["packed"])])
    w_tap = a.out((3, 3, Cin, npad), BF, "w_tap")                      # ssd_weight_transpose_batched, tap-major
    want = torch.zeros((3, 3, Cin, npad), dtype=BF)
    want[..., :n * (4 + C)] = r["w"].permute(1, 2, 3, 0)
    a.run(lambda: ops.weight_transpose_tap(w, npad, out=w_tap), [(w_tap, want)])


# ---------------------------------------------------------------- the chain of small layers
@pytest.mark.parametrize("B", [1, 5])
def test_conv_chain_strict(ops, L, B):
    r = strict.chain_case(B)
    strict.check_regime(r)
    a = arena_for(r)
    x = a.put(r["x"], "in0")
    fwd, want, want_pk, pairs, biases = [], [], [], [], []
    for i, l in enumerate(r["layers"]):
        w = a.put(l["w"], "w%d" % i)
        biases.append(a.put(l["bias"], "bias%d" % i))
        pk = a.out(tuple(l["w"].shape), BF, "packed w%d" % i)
        pairs.append((w, pk))
        want_pk.append((pk, pack_fragments(l["w"])))
    a.run(lambda: ops.chain_pack_weights(pairs), want_pk)
    pks = []
    for i, l in enumerate(r["layers"]):
        pk = a.put(want_pk[i][1], "packed w%d (operand)" % i)
        pks.append(pk)
        out = a.out(tuple(l["y"].shape), BF, "y%d" % i)
        rb = a.out(tuple(l["bits"].shape), U8, "relu_bits%d" % i)
        fwd.append(ops.chain_layer_fwd(l["w"], pk, biases[i], out, l["s"], l["pt"], l["pt"], relu=True, relu_bits=rb))
        want += [(out, l["y"].to(BF)), (rb, l["bits"])]
    a.run(lambda: ops.conv_chain(x, fwd), want)
    a.run(lambda: ops.chain_prefetch(pks), [])                           # reads only: nothing may change
    # data gradients from the last layer back, masked by each layer's input activation: as sign bytes on layers 0 and 4, as
    # the activation itself on the others; the maps that feed a head accumulate
    b = arena_for(r)
    g_last = b.put(r["layers"][-1]["gin"].to(BF), "g_last")
    bwd, want = [], []
    for i in range(len(r["layers"]) - 1, -1, -1):
        l = r["layers"][i]
        pk = b.put(pack_fragments(l["w_t"]), "packed w_t%d" % i)
        go = b.inout(l["head"], "g%d (accumulated onto)" % i) if l["head"] is not None else b.out(tuple(l["x"].shape), BF, "g%d" % i)
        use_bits = i % 4 == 0
        mask = b.put(strict.pack_bits(l["x"] > 0) if use_bits else l["x"].to(BF), "mask%d" % i)
        bwd.append(ops.chain_layer_dgrad(l["w_t"], pk, go, l["s"], l["pt"], l["pt"], accumulate=l["head"] is not None,
                                         mask_bits=mask if use_bits else None, mask_src=None if use_bits else mask))
        want.append((go, l["gout"].to(BF)))
    b.run(lambda: ops.conv_chain(g_last, bwd), want)


def pack_fragments(w):
    """ssd_chain_pack_weights, restated: filters [N][K] (k = (tap, channel) contiguous) -> packed[N/16][K/32][64][8] with element
    (lane, e) of fragment (nt, s) = w[16 nt + (lane & 15)][32 s + 8 (lane >> 4) + e]; returned in w's shape"""
    N = w.shape[0]
    K = w.numel() // N
    f = w.reshape(N // 16, 16, K // 32, 4, 8)                 # [nt][lane & 15][s][lane >> 4][e]
    return f.permute(0, 2, 3, 1, 4).contiguous().view(w.shape)


# ---------------------------------------------------------------- pooling and element-wise kernels
@pytest.mark.parametrize("case", [(2, 20, 20, 64, False), (2, 21, 23, 64, True), (2, 21, 23, 64, False)], ids=str)
def test_maxpool2x2_strict(ops, L, case):
    B, H, W, C, same = case
    r = strict.pool2x2_case(*case)
    strict.check_regime(r)
    Ho, Wo = r["y"].shape[1:3]
    a = arena_for(r)
    x, dy = a.put(r["x"], "x"), a.put(r["dy"], "dy")
    y, code, dx = a.out((B, Ho, Wo, C), BF, "y"), a.out((B, Ho, Wo, C // 8), I32, "code"), a.out((B, H, W, C), BF, "dx")
    a.run(lambda: ops.maxpool2x2_fwd_argmax(x, same=same, out=y, code=code), [(y, r["y"].to(BF)), (code, strict.pack_codes(r["code"]))])
    a.run(lambda: ops.maxpool2x2_fwd(x, same=same, out=y), [(y, r["y"].to(BF))])
    codes, yin = a.put(strict.pack_codes(r["code"]), "code (operand)"), a.put(r["y"].to(BF), "y (operand)")
    a.run(lambda: ops.maxpool2x2_bwd_argmax(codes, dy, (B, H, W, C), out=dx), [(dx, r["dx"].to(BF))])
    a.run(lambda: ops.maxpool2x2_bwd(x, yin, dy, out=dx), [(dx, r["dx"].to(BF))])


@pytest.mark.parametrize("H,W", [(9, 9), (37, 50)])
def test_maxpool3x3s2_strict(ops, L, H, W):
    B, C = 2, 64
    r = strict.pool3x3_case(B, H, W, C)
    strict.check_regime(r)
    Ho, Wo = r["geom"][:2]
    a = arena_for(r)
    x, dy = a.put(r["x"], "x"), a.put(r["dy"], "dy")
    y, code, dx = a.out((B, Ho, Wo, C), BF, "y"), a.out((B, Ho, Wo, C // 8), I32, "code"), a.out((B, H, W, C), BF, "dx")
    a.run(lambda: ops.maxpool3x3s2_fwd(x, out=y, code=code), [(y, r["y"].to(BF)), (code, strict.pack_codes(r["code"]))])
    codes = a.put(strict.pack_codes(r["code"]), "code (operand)")
    a.run(lambda: ops.maxpool3x3s2_bwd(codes, dy, (B, H, W, C), out=dx), [(dx, r["dx"].to(BF))])


def test_add_relu_and_relu_mask_strict(ops, L):
    shape = (3, 17, 19, 64)
    r = strict.eltwise_case(shape)
    strict.check_regime(r)
    a = arena_for(r)
    x, y, g, act = a.put(r["a"], "a"), a.put(r["b"], "b"), a.put(r["g"], "g"), a.put(r["out"].to(BF), "act")
    out = a.out(shape, BF, "out")
    a.run(lambda: ops.add_relu_fwd(x, y, out=out), [(out, r["out"].to(BF))])
    a.run(lambda: ops.relu_mask_bwd(g, act, out=out), [(out, r["masked"].to(BF))])
    acc = a.inout(r["base"], "out (accumulated onto)")
    a.run(lambda: ops.relu_mask_bwd(g, act, out=acc, accumulate=True), [(acc, r["acc"].to(BF))])


def test_cast_and_image_prep_strict(ops, L):
    g = torch.Generator().manual_seed(4)
    src = strict.ints(g, (5, 1031), (-3, -2, -1, 0, 1, 2, 3), scale=0.25, dtype=F32)
    img = strict.ints(g, (2, 9, 11, 3), (0, 1, 2, 3, 4), scale=0.25, dtype=F32)             # (x - 0.5) * 2 is exact
    want_img = torch.zeros((2, 9, 11, 8), dtype=BF)
    want_img[..., :3] = ((img - 0.5) * 2).to(BF)
    a = strict.Arena("cuda", 1 << 25)
    s, i = a.put(src, "src"), a.put(img, "image")
    d, o = a.out((5, 1031), BF, "dst"), a.out((2, 9, 11, 8), BF, "prepared image")
    a.run(lambda: ops.cast_bf16(s, dst=d), [(d, src.to(BF))])
    a.run(lambda: ops.image_prep(i, out=o), [(o, want_img)])


# ---------------------------------------------------------------- MX-fp8
def put_mx(ops, a, r, name, shape=None):
    """the reference's quantised operand in the arena -- after ssd_quantize_mx_fp8 (through the arena too) has reproduced its
    bytes and the bytes have been shown to stand for the integers exactly"""
    t = r[name] if name != "w_t" else r["w_t"][..., :r["w"].shape[0]].contiguous()
    src = a.put(t, name + " (bf16)")
    q, s = a.out(tuple(t.shape), U8, name + " q"), a.out(tuple(r[name + "_s"].shape), U8, name + " scale")
    a.run(lambda: ops.quantize_mx_fp8(src, q=q, scale=s), [(q, r[name + "_q"]), (s, r[name + "_s"])])
    assert torch.equal(ops.dequantize_mx_fp8(r[name + "_q"], r[name + "_s"]), t.float())
    return a.put(r[name + "_q"], name + " q (operand)"), a.put(r[name + "_s"], name + " scale (operand)")


def test_mxfp8_conv3x3_strict(ops, L):
    case = (2, 19, 19, 256, 256, 3, 1, "same")
    r = strict.mx_conv_case(case)
    a = arena_for(r)
    (xq, xs), (wq, wsc), bias = put_mx(ops, a, r, "x"), put_mx(ops, a, r, "w"), a.put(r["bias"], "bias")
    y = a.out((2, 19, 19, 256), BF, "y")
    for relu in (True, False):
        a.run(lambda: ops.conv3x3_fwd_mxfp8(xq, xs, wq, wsc, bias, relu=relu, out=y), [(y, r["y_relu" if relu else "y"].to(BF))])


def test_mxfp8_conv2d_fwd_strict(ops, L):
    case = (2, 19, 19, 256, 64, 1, 1, "same")
    B, H, W, Cin, Cout, k, stride, _ = case
    r = strict.mx_conv_case(case)
    Ho, Wo, pt, pl = r["geom"]
    a = arena_for(r)
    (xq, xs), (wq, wsc), bias = put_mx(ops, a, r, "x"), put_mx(ops, a, r, "w"), a.put(r["bias"], "bias")
    y, q, sc = a.out((B, Ho, Wo, Cout), BF, "y"), a.out((B, Ho, Wo, Cout), U8, "y8"), a.out((B, Ho, Wo, Cout // 32), U8, "yscale")
    for relu in (True, False):
        yr = r["y_relu" if relu else "y"].to(BF)
        qr, sr = strict.ref_quantize_mx(yr)
        args = (xq, xs, wq, wsc, bias, stride, pt, pl, Ho, Wo, relu)
        a.run(lambda: ops.conv2d_fwd_mxfp8(*args, want_bf16=True, want_fp8=True, out=y, out_q=q, out_scale=sc), [(y, yr), (q, qr), (sc, sr)])
        a.run(lambda: ops.conv2d_fwd_mxfp8(*args, want_bf16=False, want_fp8=True, out_q=q, out_scale=sc), [(q, qr), (sc, sr)])
        a.run(lambda: ops.conv2d_fwd_mxfp8(*args, out=y), [(y, yr)])


@pytest.mark.parametrize("same", [True, False], ids=["same", "valid"])
def test_mxfp8_conv2d_fwd_pool_strict(ops, L, same):
    case = (1, 7, 7, 128, 128, 3, 1, "same")
    B, H, W, Cin, Cout, k, stride, _ = case
    r = strict.mx_conv_case(case)
    Hp = (H + 1) // 2 if same else H // 2
    pr, _ = strict.ref_pool(r["y_relu"], 2, 2, 0, 0, Hp, Hp, 4)
    pr = pr.to(BF)
    qr, sr = strict.ref_quantize_mx(pr)
    a = arena_for(r)
    (xq, xs), (wq, wsc), bias = put_mx(ops, a, r, "x"), put_mx(ops, a, r, "w"), a.put(r["bias"], "bias")
    p, q, sc = a.out((B, Hp, Hp, Cout), BF, "y_pool"), a.out((B, Hp, Hp, Cout), U8, "y_pool8"), a.out((B, Hp, Hp, Cout // 32), U8, "y_pool_scale")
    args = (xq, xs, wq, wsc, bias, 1, 1, 1, H, W, True, same)
    a.run(lambda: ops.conv2d_fwd_pool_mxfp8(*args, want_bf16=True, want_fp8=True, out=p, out_q=q, out_scale=sc), [(p, pr), (q, qr), (sc, sr)])
    a.run(lambda: ops.conv2d_fwd_pool_mxfp8(*args, want_bf16=False, want_fp8=True, out_q=q, out_scale=sc), [(q, qr), (sc, sr)])
    a.run(lambda: ops.conv2d_fwd_pool_mxfp8(*args, out=p), [(p, pr)])


def test_mxfp8_conv2d_bwd_data_strict(ops, L):
    case = (2, 19, 19, 64, 256, 1, 1, "same")
    B, H, W, Cin, Cout, k, stride, _ = case
    r = strict.mx_conv_case(case)
    Ho, Wo, pt, pl = r["geom"]
    a = arena_for(r)
    (dyq, dys), (wtq, wts), mask = put_mx(ops, a, r, "dy"), put_mx(ops, a, r, "w_t"), a.put(r["mask_src"], "relu_src")
    dx, q, sc = a.out((B, H, W, Cin), BF, "dx"), a.out((B, H, W, Cin), U8, "dx8"), a.out((B, H, W, Cin // 32), U8, "dxscale")
    args = (dyq, dys, wtq, wts)
    for src, name in ((None, "dx"), (mask, "dx_masked")):
        want = r[name].to(BF)
        qr, sr = strict.ref_quantize_mx(want)
        a.run(lambda: ops.conv2d_bwd_data_mxfp8(*args, src, (B, H, W, Cin), 1, pt, pl, want_bf16=True, want_fp8=True, out=dx, out_q=q, out_scale=sc),
              [(dx, want), (q, qr), (sc, sr)])
        a.run(lambda: ops.conv2d_bwd_data_mxfp8(*args, src, (B, H, W, Cin), 1, pt, pl, want_bf16=False, want_fp8=True, out_q=q, out_scale=sc),
              [(q, qr), (sc, sr)])
    acc = a.inout(r["base"], "dx (accumulated onto)")
    want = r["dx_acc"].to(BF)
    qr, sr = strict.ref_quantize_mx(want)
    a.run(lambda: ops.conv2d_bwd_data_mxfp8(*args, mask, (B, H, W, Cin), 1, pt, pl, accumulate=True, want_bf16=True, want_fp8=True, out=acc,
                                            out_q=q, out_scale=sc), [(acc, want), (q, qr), (sc, sr)])

    def refused():                                          # stride 2 has no fp8 form
        with pytest.raises(NotImplementedError):
            ops.conv2d_bwd_data_mxfp8(*args, None, (B, H, W, Cin), 2, pt, pl, out=dx)
    a.run(refused, [])


def test_mxfp8_add_relu_strict(ops, L):
    shape = (3, 17, 19, 256)
    r = strict.eltwise_case(shape)
    strict.check_regime(r)
    want = r["out"].to(BF)
    qr, sr = strict.ref_quantize_mx(want)
    a = arena_for(r)
    x, y = a.put(r["a"], "a"), a.put(r["b"], "b")
    out, q, sc = a.out(shape, BF, "out"), a.out(shape, U8, "q"), a.out(shape[:-1] + (shape[-1] // 32,), U8, "scale")
    a.run(lambda: ops.add_relu_fwd_mxfp8(x, y, out=out, q=q, scale=sc), [(out, want), (q, qr), (sc, sr)])
