"""GPU: the SSD300 network's inference forward in block-scaled fp8 (MX: OCP e4m3 + one E8M0 scale per 32 channels) --
SSDEngine.forward(x, "mxfp8") on ssd_conv2d_fwd_mxfp8 and the pooled ssd_conv2d_fwd_pool_mxfp8 (block3_conv3 + its SAME pool),
and detect / evaluate(precision="mxfp8") on top of it.  No reference counterpart (fp32 TensorFlow convolutions).  Checked as
test_resnet_mxfp8_gpu.py checks the ResNet trunk:
  (a) the pooled kernel bitwise against conv2d_fwd_mxfp8 -> maxpool2x2_fwd -> quantize_mx_fp8, and against the fp32
      convolution of its own dequantised operands (2^-7 of the tensor maximum);
  (b) the network layer by layer on the operands the engine actually used, every fused fp8 map bitwise;
  (c) end to end against the bf16 forward and at model level against bf16 detection: the quantisation error STATED with a bound."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import torch.nn.functional as F                                      # noqa: E402


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def make_engine(seed):
    from ssd_object_detection_amd.engine import SSDEngine
    return SSDEngine(classes=81, seed=seed)


def image(ops, B, seed):
    g = torch.Generator().manual_seed(seed)
    return ops.image_prep(torch.rand((B, 300, 300, 3), generator=g).cuda())


def conv_ref(x, w, bias, stride, pt, pl, Ho, Wo, relu=True):
    """fp32 convolution of NHWC x with [Cout,k,k,Cin] w, explicit top / left pads (the rest of the window padded as needed)."""
    k = w.shape[1]
    H, W = x.shape[1], x.shape[2]
    pb, pr = max((Ho - 1) * stride + k - H - pt, 0), max((Wo - 1) * stride + k - W - pl, 0)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xp, w.permute(0, 3, 1, 2), bias, stride=stride)[:, :, :Ho, :Wo]
    y = y.relu() if relu else y
    return y.permute(0, 2, 3, 1)


def pool_ref(y, same):
    """2x2 / stride-2 max pool of NHWC y: TF-SAME (windows clipped at the bottom / right edge) or VALID."""
    t = y.permute(0, 3, 1, 2)
    if same:
        t = F.pad(t, (0, t.shape[3] % 2, 0, t.shape[2] % 2), value=float("-inf"))
    return F.max_pool2d(t, 2).permute(0, 2, 3, 1)


def check_bound(y, ya, what):
    err = (y.float() - ya).abs().max().item()
    assert err <= 2 ** -7 * max(1.0, ya.abs().max().item()), (what, err, ya.abs().max().item())


def rel_cos(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm()), float((a * b).sum() / (a.norm() * b.norm()))


# ---------------------------------------------------------------- (a) the pooled kernel
@pytest.mark.parametrize("cout", [128, 256, 512])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [75, 19, 8, 7])
@pytest.mark.parametrize("same", [True, False], ids=["same", "valid"])
def test_conv2d_fwd_pool_mxfp8(ops, same, H, B, cout):
    Cin = 256 if H == 19 else 128
    W = H
    g = torch.Generator(device="cuda").manual_seed(H * 7 + B + cout)
    x = torch.randn((B, H, W, Cin), generator=g, device="cuda").relu().bfloat16()
    w = (torch.randn((cout, 3, 3, Cin), generator=g, device="cuda") / (9 * Cin) ** 0.5).bfloat16()
    bias = torch.randn((cout,), generator=g, device="cuda") * 0.1
    xq, xs = ops.quantize_mx_fp8(x)
    wq, ws = ops.quantize_mx_fp8(w)
    args = (xq, xs, wq, ws, bias, 1, 1, 1, H, W, True)
    # the unfused chain this launch replaces
    y = ops.conv2d_fwd_mxfp8(*args)
    p_ref = ops.maxpool2x2_fwd(y, same=same)
    q_ref, s_ref = ops.quantize_mx_fp8(p_ref)
    Hp = (H + 1) // 2 if same else H // 2
    p, q, s = ops.conv2d_fwd_pool_mxfp8(*args, same, want_bf16=True, want_fp8=True)
    assert p.shape == (B, Hp, Hp, cout) and q.shape == p.shape and s.shape == (B, Hp, Hp, cout // 32)
    assert torch.equal(p, p_ref), "pooled bf16 map != maxpool2x2_fwd(conv2d_fwd_mxfp8(...))"
    assert torch.equal(q, q_ref) and torch.equal(s, s_ref), "pooled fp8 map != quantize_mx_fp8 of the pooled bf16 map"
    assert torch.equal(ops.conv2d_fwd_pool_mxfp8(*args, same), p), "bf16-only launch differs"
    q8, s8 = ops.conv2d_fwd_pool_mxfp8(*args, same, want_bf16=False, want_fp8=True)
    assert torch.equal(q8, q) and torch.equal(s8, s), "fp8-only launch differs"
    with torch.no_grad():
        ya = pool_ref(conv_ref(ops.dequantize_mx_fp8(xq, xs), ops.dequantize_mx_fp8(wq, ws), bias, 1, 1, 1, H, W), same)
    check_bound(p, ya, "pooled kernel vs fp32 on the dequantised operands")


# ---------------------------------------------------------------- (b) the network, layer by layer
@pytest.fixture(scope="module")
def engine():
    return make_engine(5)


def test_network_layer_by_layer(ops, engine):
    """Every fp8 node recomputed in fp32 from the fp8 input and filters the engine used; every fused fp8 map bitwise
    quantize_mx_fp8 of its bf16 twin; the standalone quantise of pooled map 5; the heads read the bf16 feature maps."""
    eng, B = engine, 8
    x = image(ops, B, 3)
    loc8, conf8 = (t.clone() for t in eng.forward(x, "mxfp8"))
    torch.cuda.synchronize()
    fp8, pooled, quant, writes = eng.vgg_mxfp8_plan()
    assert fp8 == {6, 7, 8, 10, 11, 12, 13, 14, 15, 16} and pooled == {9} and quant == {5}
    acts, mx = eng._acts(B)["acts"], eng.mxfp8_acts(B)
    with torch.no_grad():
        q_ref, s_ref = ops.quantize_mx_fp8(acts[6])
        assert torch.equal(mx[5][0], q_ref) and torch.equal(mx[5][1], s_ref), "standalone quantise of pooled map 5"
        for i in sorted(fp8):
            nd = eng.nodes[i]
            xq, xs = mx[i - 1]
            wq, ws = eng.mxfp8_weights(i)
            bias = eng.view(eng.conv_params[i][1], eng.param)
            args = (xq, xs, wq, ws, bias, nd["stride"], nd["pt"], nd["pl"], nd["hout"], nd["hout"], True)
            ya = conv_ref(ops.dequantize_mx_fp8(xq, xs), ops.dequantize_mx_fp8(wq, ws), bias, *args[5:10])
            o = i + 1 if i + 1 in pooled else i
            w = writes[o]
            if o != i:                                                # block3_conv3 + pool: the launch kept the fp8 map only
                same = eng.nodes[o]["hout"] * 2 != eng.nodes[o]["hin"]
                ya = pool_ref(ya, same)
                assert w == frozenset({"fp8"})
                y, q, sc = ops.conv2d_fwd_pool_mxfp8(*args, same, want_bf16=True, want_fp8=True)
                assert torch.equal(q, mx[o][0]) and torch.equal(sc, mx[o][1]), i
            elif "bf16" in w:
                y = acts[i + 1]
            else:                                                     # the engine kept only the fp8 map: relaunch for its bf16 twin
                y, q, sc = ops.conv2d_fwd_mxfp8(*args, want_bf16=True, want_fp8=True)
                assert torch.equal(q, mx[i][0]) and torch.equal(sc, mx[i][1]), i
            check_bound(y, ya, "node %d" % i)
            if "fp8" in w:
                q_ref, s_ref = ops.quantize_mx_fp8(y)
                assert torch.equal(mx[o][0], q_ref) and torch.equal(mx[o][1], s_ref), i
        # the heads read the bf16 feature maps of this forward
        loc_h, conf_h = torch.empty_like(loc8), torch.empty_like(conf8)
        for lvl, (ni, _, _) in enumerate(eng.fm):
            assert "bf16" in writes[ni]
            wt, bt = eng.head_params[lvl]
            ops.conv2d_head_fwd(acts[ni + 1], eng.view(wt, eng.param_bf16), eng.view(bt, eng.param), loc_h, conf_h,
                                eng.num_priors[lvl], eng.classes, eng.level_off[lvl])
        assert torch.equal(loc_h, loc8) and torch.equal(conf_h, conf8)
        # the fp8-free front equals a bf16 forward bit for bit (the maps of nodes 1 and 4 stay inside their pooled launches)
        front = {i: acts[i + 1].clone() for i in (0, 2, 3, 5)}
        eng.forward(x)
        for i, t in front.items():
            assert torch.equal(t, acts[i + 1]), i


# ---------------------------------------------------------------- (c) end to end
@pytest.mark.parametrize("B", [8, 64])
def test_network_end_to_end(ops, engine, B):
    eng = engine
    x = image(ops, B, 4 + B)
    loc, conf = (t.float().clone() for t in eng.forward(x))
    loc8, conf8 = (t.float().clone() for t in eng.forward(x, "mxfp8"))
    res = {"loc": rel_cos(loc8, loc), "conf": rel_cos(conf8, conf)}
    for name, (err, cos) in res.items():
        print("batch %d, mxfp8 vs bf16 forward, %s: relative L2 %.4f, cosine %.5f" % (B, name, err, cos))
    # the stated quantisation error of the 10 fp8 layers (seed-5 weights), measured at batch 8 and 64 alike: relative L2 0.113
    # (loc) / 0.079 (conf), cosine 0.9939 / 0.9969; bound = measured x ~1.8 on the error
    for name, (err, cos) in res.items():
        assert err <= 0.2 and cos >= 0.98, (B, name, err, cos)


# ---------------------------------------------------------------- determinism and isolation
def test_determinism_and_isolation(ops):
    eng = make_engine(7)
    B = 4
    x = image(ops, B, 8)
    loc_a, conf_a = (t.clone() for t in eng.forward(x))
    assert "mxfp8" not in eng._acts(B) and not eng.mx_filters.allocated, "a bf16-only run allocated fp8 buffers"
    loc8, conf8 = (t.clone() for t in eng.forward(x, "mxfp8"))
    loc8b, conf8b = eng.forward(x, "mxfp8")
    assert torch.equal(loc8, loc8b) and torch.equal(conf8, conf8b), "two fp8 forwards differ"
    assert not torch.equal(loc8, loc_a)
    loc_b, conf_b = eng.forward(x)
    assert torch.equal(loc_a, loc_b) and torch.equal(conf_a, conf_b), "a bf16 forward after an fp8 one differs"


def test_mode_switching_and_fresh_weights(ops):
    """backward() after an fp8 forward raises; after a bf16 forward it runs; after an Adam step the fp8 forward equals a
    fresh engine's loaded with the updated weights."""
    eng = make_engine(11)
    B = 2
    x = image(ops, B, 12)
    g = torch.Generator(device="cuda").manual_seed(13)
    loc0, _ = (t.clone() for t in eng.forward(x, "mxfp8"))
    dloc = (torch.randn(loc0.shape, generator=g, device="cuda") * 1e-3).bfloat16()
    dconf = (torch.randn((B, eng.A, eng.classes), generator=g, device="cuda") * 1e-3).bfloat16()
    with pytest.raises(RuntimeError):
        eng.backward(dloc, dconf)
    with pytest.raises(ValueError):
        eng.forward(x, "fp16")
    eng.forward(x)
    eng.backward(dloc, dconf)
    eng.clip_scales(0.01)
    eng.adam(1e-3, eng.grad, 1.0, True)
    loc1, conf1 = (t.clone() for t in eng.forward(x, "mxfp8"))
    assert not torch.equal(loc1, loc0), "the step did not reach the fp8 forward"
    fresh = make_engine(12)
    fresh.load_state_dict(eng.state_dict())
    assert torch.equal(fresh.param_bf16, eng.param_bf16)
    loc2, conf2 = fresh.forward(x, "mxfp8")
    assert torch.equal(loc1, loc2) and torch.equal(conf1, conf2)


# ---------------------------------------------------------------- model level
def test_model_detect_and_evaluate(tmp_path):
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt, synth_image
    from ssd_object_detection_amd.utils.metrics import iou_matrix
    model = SSDObjectDetectionModel(classes=80, log_dir=str(tmp_path), seed=1, timestamp_dir=False)
    B = 8
    cls_l, box_l = synth_batch_gt(700, B)
    imgs = [synth_image(700 + i) for i in range(B)]
    image_, (cls, loc, mask) = model.make_batch(imgs, cls_l, box_l)
    opt = optimizers.Adam(1e-3)
    for _ in range(30):
        model._train_step(image_, cls, loc, mask, opt)
    thresh = 0.3
    kept = {}
    for prec in ("bf16", "mxfp8"):
        score, dcls, box, keep = model.detect(image_, score_thresh=thresh, precision=prec)
        keep = keep.cpu().numpy().astype(bool)
        kept[prec] = [(dcls[i].cpu().numpy()[keep[i]], box[i].cpu().numpy()[keep[i]]) for i in range(B)]
    n16 = sum(len(c) for c, _ in kept["bf16"])
    n8 = sum(len(c) for c, _ in kept["mxfp8"])
    found = 0
    for (c16, b16), (c8, b8) in zip(kept["bf16"], kept["mxfp8"]):
        if len(c16) and len(c8):
            iou = iou_matrix(b16.astype(np.float64), b8.astype(np.float64))     # (cx, cy, w, h) pixels
            found += int(((iou >= 0.5) & (c16[:, None] == c8[None, :])).any(1).sum())
    share = found / max(n16, 1)
    print("kept detections: bf16 %d, mxfp8 %d; bf16 ones matched by an mxfp8 one (same class, IoU >= 0.5): %.3f"
          % (n16, n8, share))
    # measured: 225 bf16 / 222 fp8 detections kept, 0.982 of the bf16 ones matched; bound 0.9
    assert n16 > 0
    assert share >= 0.9, (share, n16, n8)
    samples = [(imgs[i], cls_l[i], box_l[i]) for i in range(B)]
    r16 = model.evaluate(samples, batch_size=B, precision="bf16")
    r8 = model.evaluate(samples, batch_size=B, precision="mxfp8")
    print("mAP bf16 %.4f, mxfp8 %.4f; AP50 %.4f / %.4f" % (r16["mAP"], r8["mAP"], r16["AP50"], r8["AP50"]))
    # measured: mAP 0.0465 bf16 / 0.0403 fp8 (30 steps on 8 images); bound: 0.02 apart
    assert abs(r8["mAP"] - r16["mAP"]) <= 0.02, (r16["mAP"], r8["mAP"])
    with pytest.raises(ValueError):
        model.detect(image_, precision="fp16")
    with pytest.raises(ValueError):
        model.evaluate(samples, batch_size=B, precision="fp16")
