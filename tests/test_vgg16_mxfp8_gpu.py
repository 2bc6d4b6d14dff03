"""GPU: the VGG-16 SSD300's inference forward in block-scaled fp8 -- SSDEngine(..., fp8_inference=True).forward(x, "mxfp8") on
ssd_conv2d_fwd_mxfp8, the pooled ssd_conv2d_fwd_pool_mxfp8, the dilated ssd_conv2d_atrous_fwd_mxfp8 (fc6) and the two
quantising poolings (pool4, pool5), and detect / evaluate(precision="mxfp8") on top of it.  No reference counterpart (fp32
TensorFlow layers).  Checked as tests/test_vgg_mxfp8_gpu.py checks SSD300:
  (a) the network layer by layer on the operands the engine actually used, every fused fp8 map bitwise;
  (b) the launches of the fp8 forward, by name and count;
  (c) end to end against the bf16 forward: the quantisation error STATED with a bound;
  (d) the engine's behaviour around the switch; (e) detection and evaluation from the model class."""
import collections

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import torch.nn.functional as F                                      # noqa: E402

from tests.test_vgg_mxfp8_gpu import check_bound, conv_ref, pool_ref, rel_cos       # noqa: E402

CLASSES = 81


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def make_engine(seed, classes=CLASSES, **kw):
    from ssd_object_detection_amd.engine import SSDEngine, VGG16_SSD300_TRUNK, VGG16_SSD300_NUM_PRIORS
    kw.setdefault("fp8_inference", True)
    return SSDEngine(classes=classes, seed=seed, trunk=VGG16_SSD300_TRUNK, num_priors=VGG16_SSD300_NUM_PRIORS, l2norm=True, **kw)


def image(ops, B, seed):
    g = torch.Generator().manual_seed(seed)
    return ops.image_prep(torch.rand((B, 300, 300, 3), generator=g).cuda())


@pytest.fixture(scope="module")
def engine():
    return make_engine(5)


def atrous_ref(x, w, bias, d):
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), bias, padding=d, dilation=d).relu()
    return y.permute(0, 2, 3, 1)


# ---------------------------------------------------------------- (a) the network, layer by layer
def test_network_layer_by_layer(ops, engine):
    """Every fp8 node, the dilated one included, recomputed in fp32 from the fp8 input and filters the engine used (2^-7 of the
    tensor maximum); every fused fp8 map bitwise quantize_mx_fp8 of its bf16 twin; both quantising poolings bitwise
    quantize_mx_fp8(maxpool(bf16 map)); the heads (L2Norm on level 0) bitwise from the stored bf16 feature maps; the fp8-free
    front bitwise the bf16 forward's."""
    eng, B = engine, 2
    x = image(ops, B, 3)
    assert not eng.bf16_only
    loc8, conf8 = (t.clone() for t in eng.forward(x, "mxfp8"))
    torch.cuda.synchronize()
    p = eng.mxfp8_plan()
    assert p.fp8 == {6, 7, 8, 10, 11, 12, 14, 15, 16, 18, 19, 20, 21} and p.pooled == {9} and p.qpool == {13, 17} and p.quant == {5}
    acts, mx = eng._acts(B)["acts"], eng.mxfp8_acts(B)
    assert set(mx) == {i for i, w in p.writes.items() if "fp8" in w} == {5, 6, 7, 9, 10, 11, 13, 14, 15, 17, 18, 19, 20}
    with torch.no_grad():
        q_ref, s_ref = ops.quantize_mx_fp8(acts[6])
        assert torch.equal(mx[5][0], q_ref) and torch.equal(mx[5][1], s_ref), "standalone quantise of pooled map 5"
        for i in sorted(p.fp8):
            nd = eng.nodes[i]
            xq, xs = mx[i - 1]
            wq, ws = eng.mxfp8_weights(i)
            bias = eng.view(eng.conv_params[i][1], eng.param)
            dx, dw = ops.dequantize_mx_fp8(xq, xs), ops.dequantize_mx_fp8(wq, ws)
            args = (xq, xs, wq, ws, bias, nd["stride"], nd["pt"], nd["pl"], nd["hout"], nd["hout"], True)
            if nd["dilation"] != 1:
                assert (i, nd["dilation"]) == (18, 6)
                ya = atrous_ref(dx, dw, bias, nd["dilation"])
            else:
                ya = conv_ref(dx, dw, bias, *args[5:10])
            o = i + 1 if i + 1 in p.pooled else i
            w = p.writes[o]
            if o != i:                                                # conv3_3 + pool3: the launch kept the fp8 map only
                same = eng.nodes[o]["hout"] * 2 != eng.nodes[o]["hin"]
                ya = pool_ref(ya, same)
                assert w == frozenset({"fp8"})
                y, q, sc = ops.conv2d_fwd_pool_mxfp8(*args, same, want_bf16=True, want_fp8=True)
                assert torch.equal(q, mx[o][0]) and torch.equal(sc, mx[o][1]), i
            elif "bf16" in w:
                y = acts[i + 1]
            elif nd["dilation"] != 1:                                 # fc6 kept only its fp8 map: relaunch for the bf16 twin
                y, q, sc = ops.conv2d_atrous_fwd_mxfp8(xq, xs, wq, ws, bias, nd["dilation"], True, want_bf16=True, want_fp8=True)
                assert torch.equal(q, mx[i][0]) and torch.equal(sc, mx[i][1]), i
            else:
                y, q, sc = ops.conv2d_fwd_mxfp8(*args, want_bf16=True, want_fp8=True)
                assert torch.equal(q, mx[i][0]) and torch.equal(sc, mx[i][1]), i
            check_bound(y, ya, "node %d" % i)
            if "fp8" in w:
                q_ref, s_ref = ops.quantize_mx_fp8(y)
                assert torch.equal(mx[o][0], q_ref) and torch.equal(mx[o][1], s_ref), i
        # the quantising poolings read the stored bf16 map in front of them
        for i in sorted(p.qpool):
            nd = eng.nodes[i]
            assert "bf16" in p.writes[i - 1] and p.writes[i] == frozenset({"fp8"})
            pooled = ops.maxpool3x3s1_fwd(acts[i])[0] if nd["kind"] == "pool3s1" else ops.maxpool2x2_fwd(acts[i], same=eng._pool_same(nd))
            q_ref, s_ref = ops.quantize_mx_fp8(pooled)
            assert torch.equal(mx[i][0], q_ref) and torch.equal(mx[i][1], s_ref), "quantising pooling %d" % i
        # the heads read the bf16 feature maps of this forward, level 0 through L2Norm
        loc_h, conf_h = torch.empty_like(loc8), torch.empty_like(conf8)
        for lvl, (ni, _, _) in enumerate(eng.fm):
            assert "bf16" in p.writes[ni]
            wt, bt = eng.head_params[lvl]
            src = acts[ni + 1]
            if lvl == 0:
                src = ops.l2norm_fwd(src, eng.view(eng.l2norm_scale, eng.param), eps=eng.l2norm.eps)
            ops.conv2d_head_fwd(src, eng.view(wt, eng.param_bf16), eng.view(bt, eng.param), loc_h, conf_h,
                                eng.num_priors[lvl], eng.classes, eng.level_off[lvl])
        assert torch.equal(loc_h, loc8) and torch.equal(conf_h, conf8)
        # the fp8-free front equals a bf16 forward bit for bit (the maps of nodes 1 and 4 stay inside their pooled launches)
        front = {i: acts[i + 1].clone() for i in (0, 2, 3, 5)}
        eng.forward(x)
        for i, t in front.items():
            assert torch.equal(t, acts[i + 1]), i


# ---------------------------------------------------------------- (b) what the fp8 forward launches
BF16_TRUNK = ("ssd_conv2d_fwd", "ssd_conv2d_fwd_relubits", "ssd_conv2d_fwd_pool", "ssd_conv2d_atrous_fwd", "ssd_maxpool2x2_fwd",
              "ssd_maxpool2x2_fwd_argmax", "ssd_maxpool3x3s1_fwd", "ssd_maxpool3x3s2_fwd")
FP8_CONVS = ("ssd_conv2d_fwd_mxfp8", "ssd_conv2d_fwd_pool_mxfp8", "ssd_conv2d_atrous_fwd_mxfp8", "ssd_conv3x3_fwd_mxfp8")


def test_launch_trace(ops, engine):
    from tests.launch_trace import Recorder
    eng, B = engine, 2
    x = image(ops, B, 3)
    traces = {}
    for prec in ("bf16", "mxfp8"):
        eng.forward(x, prec)                                          # (learned fallbacks and buffers settle)
        torch.cuda.synchronize()
        with Recorder() as rec:
            eng.forward(x, prec)
        torch.cuda.synchronize()
        traces[prec] = collections.Counter(c[0] for c in rec.calls)
    t16, t8 = traces["bf16"], traces["mxfp8"]
    p = eng.mxfp8_plan()
    quant = next(iter(p.quant))
    front = sum(1 for nd in eng.nodes[:quant + 1] if nd["kind"] == "conv")
    assert sum(t8[n] for n in FP8_CONVS) == len(p.fp8) == 13, t8
    assert (t8["ssd_conv2d_fwd_pool_mxfp8"], t8["ssd_conv2d_atrous_fwd_mxfp8"], t8["ssd_conv2d_fwd_mxfp8"]) == (1, 1, 11), t8
    assert (t8["ssd_maxpool2x2_fwd_mxfp8"], t8["ssd_maxpool3x3s1_fwd_mxfp8"]) == (1, 1), t8
    assert t8["ssd_quantize_mx_fp8"] == 2, t8                        # the filters' one launch + the activation of node 5
    # no bf16 convolution or pooling behind the quantised node: what is left of them is the front's (its pools run inside
    # their convolutions' calls)
    assert sum(t8[n] for n in BF16_TRUNK) == front == 4, t8
    assert sum(t16[n] for n in BF16_TRUNK) == front + len(p.fp8) + 1 and t16["ssd_maxpool3x3s1_fwd"] == 1, t16
    assert not any(t16[n] for n in FP8_CONVS + ("ssd_quantize_mx_fp8", "ssd_maxpool2x2_fwd_mxfp8", "ssd_maxpool3x3s1_fwd_mxfp8"))
    # chain, heads and L2Norm are the bf16 forward's
    for name in ("ssd_conv_chain", "ssd_conv2d_head_fwd", "ssd_l2norm_fwd"):
        assert t8[name] == t16[name] > 0, (name, t8[name], t16[name])
    assert (t8["ssd_conv2d_head_fwd"], t8["ssd_l2norm_fwd"], t8["ssd_conv_chain"]) == (6, 1, 1)


# ---------------------------------------------------------------- (c) end to end
# The stated quantisation error of the 13 fp8 layers and the two quantising poolings, measured on one MI355X with random
# (Glorot) filters, (relative L2, cosine) of loc | conf against the bf16 forward of the same engine:
#   seed  5: batch 2  0.0692, 0.99771 | 0.0779, 0.99697     batch 8  0.0693, 0.99769 | 0.0779, 0.99696
#   seed  7: batch 2  0.0766, 0.99711 | 0.0942, 0.99556     batch 8  0.0766, 0.99712 | 0.0940, 0.99558
#   seed 11: batch 2  0.0854, 0.99647 | 0.0740, 0.99728     batch 8  0.0859, 0.99643 | 0.0741, 0.99727
# E2E holds the worst of each: the bound is 1.5 x the worst error, and 1.5 x the worst (1 - cosine) -- the sibling tests'
# convention, which covers the seed-to-seed variation seen above.
E2E = dict(loc=(0.0859, 0.99643), conf=(0.0942, 0.99556))


def test_network_end_to_end(ops, engine):
    eng, B = engine, 8
    x = image(ops, B, 4 + B)
    loc, conf = (t.float().clone() for t in eng.forward(x))
    loc8, conf8 = (t.float().clone() for t in eng.forward(x, "mxfp8"))
    assert not torch.equal(loc8, loc) and not torch.equal(conf8, conf), "the fp8 forward returned the bf16 forward's outputs"
    res = {"loc": rel_cos(loc8, loc), "conf": rel_cos(conf8, conf)}
    for name, (err, cos) in res.items():
        print("batch %d, mxfp8 vs bf16 forward, %s: relative L2 %.4f, cosine %.5f" % (B, name, err, cos))
    for name, (err, cos) in res.items():
        worst_err, worst_cos = E2E[name]
        assert err <= 1.5 * worst_err and 1.0 - cos <= 1.5 * (1.0 - worst_cos), (name, err, cos)


# ---------------------------------------------------------------- (d) the engine around the switch
def test_determinism_isolation_and_fresh_weights(ops):
    """Two fp8 forwards are equal; a bf16 forward before and after is bitwise unchanged; nothing fp8 is allocated before the
    first fp8 forward; backward() after an fp8 forward raises until a bf16 forward; after an optimizer step the fp8 forward
    equals a fresh engine's loaded from state_dict()."""
    eng = make_engine(7)
    B = 2
    x = image(ops, B, 8)
    loc_a, conf_a = (t.clone() for t in eng.forward(x))
    assert "mxfp8" not in eng._acts(B) and not eng.mx_filters.allocated, "a bf16-only run allocated fp8 buffers"
    loc8, conf8 = (t.clone() for t in eng.forward(x, "mxfp8"))
    assert eng.last_forward == "mxfp8" and eng.mx_filters.allocated
    loc8b, conf8b = eng.forward(x, "mxfp8")
    assert torch.equal(loc8, loc8b) and torch.equal(conf8, conf8b), "two fp8 forwards differ"
    assert not torch.equal(loc8, loc_a)
    g = torch.Generator(device="cuda").manual_seed(13)
    dloc = (torch.randn(loc8.shape, generator=g, device="cuda") * 1e-3).bfloat16()
    dconf = (torch.randn((B, eng.A, eng.classes), generator=g, device="cuda") * 1e-3).bfloat16()
    with pytest.raises(RuntimeError, match="mxfp8"):
        eng.backward(dloc, dconf)
    loc_b, conf_b = (t.clone() for t in eng.forward(x))
    assert torch.equal(loc_a, loc_b) and torch.equal(conf_a, conf_b), "a bf16 forward after an fp8 one differs"
    eng.backward(dloc, dconf)
    eng.clip_scales(0.01)
    eng.sgd_momentum(1e-3, eng.grad, 1.0, True, 0.9, False, None)
    loc1, conf1 = (t.clone() for t in eng.forward(x, "mxfp8"))
    assert not torch.equal(loc1, loc8), "the step did not reach the fp8 forward"
    fresh = make_engine(12)
    fresh.load_state_dict(eng.state_dict())
    assert torch.equal(fresh.param_bf16, eng.param_bf16)
    loc2, conf2 = fresh.forward(x, "mxfp8")
    assert torch.equal(loc1, loc2) and torch.equal(conf1, conf2)


def test_without_the_switch_the_engine_still_refuses(ops):
    eng = make_engine(7, fp8_inference=False)
    x = image(ops, 1, 8)
    assert eng.bf16_only
    eng.forward(x)
    with pytest.raises(NotImplementedError, match="VGG-16"):
        eng.forward(x, "mxfp8")
    assert eng.last_forward == "bf16" and not eng.mx_filters.allocated


# ---------------------------------------------------------------- (e) model level
MODEL_CLASSES, MODEL_B = 20, 2
# Four steps leave the class scores of this randomly initialised network between 0.05 and 0.30 (median 0.048, 99th percentile
# 0.27): detect()'s default threshold 0.3 keeps 2 detections, too few to measure a share on; 0.2 is the next step down and keeps
# 507 (bf16) / 553 (mxfp8).  Measured on one MI355X: 0.795 of the bf16 detections are matched by an mxfp8 one.  That is below
# the 0.98 of the trained-longer SSD300 sibling test: with every score inside a band of 0.07, the quantisation error decides
# which class wins a box.  The threshold was chosen by the bf16 count alone; the bound is the measured share minus
# max(0.05, 5 / bf16 detections).
SCORE_THRESH = 0.2
SHARE = 0.795


def make_model(log_dir, seed=17, **kw):
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    return SSDObjectDetectionModel(classes=MODEL_CLASSES, log_dir=str(log_dir), seed=seed, timestamp_dir=False, network="vgg16_ssd300",
                                   l2norm=True, **kw)


def trained_model(ops, tmp_path):
    """tests/test_vgg16_model_gpu.py's four steps of the paper's recipe on one fixed batch (MultiBox loss, momentum SGD at 1e-3
    with weight decay, no clipping, L2Norm); returns (model, the batch's images f32 in [0, 1], its ground truth lists)"""
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt
    model = make_model(tmp_path, fp8_inference=True)
    cls_l, box_l = synth_batch_gt(0, MODEL_B)
    cls_l = [np.mod(c, MODEL_CLASSES).astype(np.float32) for c in cls_l]
    raw = torch.rand((MODEL_B, 300, 300, 3), generator=torch.Generator().manual_seed(21))
    x = ops.image_prep(raw.cuda(), normalize=True)
    tgt = model.match_async(ops.pack_gt(box_l, cls_l))
    cfg = SSDObjectDetectionModel.TrainConfig(epoch=1, batch_size=MODEL_B, optimizer=None, warmup=False, loss="multibox", clip=None)
    opt = optimizers.SGD(1e-3, momentum=0.9, weight_decay=5e-4)
    for _ in range(4):
        _, _, info = model._train_step(x, *tgt, opt, cfg=cfg)
        assert float(info["status"]) == 0.0
    return model, raw, cls_l, box_l


def matched_share(model, image_, thresh):
    """(bf16 detections kept, mxfp8 detections kept, share of the bf16 ones an mxfp8 one matches: same class, IoU >= 0.5)"""
    from ssd_object_detection_amd.utils.metrics import iou_matrix
    kept = {}
    for prec in ("bf16", "mxfp8"):
        score, dcls, box, keep = model.detect(image_, score_thresh=thresh, precision=prec)
        keep = keep.cpu().numpy().astype(bool)
        kept[prec] = [(dcls[i].cpu().numpy()[keep[i]], box[i].cpu().numpy()[keep[i]]) for i in range(image_.shape[0])]
    n16, n8 = (sum(len(c) for c, _ in kept[k]) for k in ("bf16", "mxfp8"))
    found = 0
    for (c16, b16), (c8, b8) in zip(kept["bf16"], kept["mxfp8"]):
        if len(c16) and len(c8):
            iou = iou_matrix(b16.astype(np.float64), b8.astype(np.float64))
            found += int(((iou >= 0.5) & (c16[:, None] == c8[None, :])).any(1).sum())
    return n16, n8, found / max(n16, 1)


def test_model_detect_evaluate_and_checkpoints(ops, tmp_path):
    model, raw, cls_l, box_l = trained_model(ops, tmp_path)
    assert model.fp8_inference and not model.get_engine().bf16_only
    image_ = (raw.cuda() - 0.5) * 2
    n16, n8, share = matched_share(model, image_, SCORE_THRESH)
    print("kept detections at score >= %.3f: bf16 %d, mxfp8 %d; bf16 ones matched by an mxfp8 one (same class, IoU >= 0.5): %.3f"
          % (SCORE_THRESH, n16, n8, share))
    assert n16 > 0
    assert share >= SHARE - max(0.05, 5.0 / n16), (share, n16, n8)
    d = model.detections(image_, score_thresh=SCORE_THRESH, keep_top_k=50, precision="mxfp8")
    assert d.score.shape == (MODEL_B, 50) and bool(torch.isfinite(d.score).all())
    samples = [(raw[i].numpy(), cls_l[i], box_l[i]) for i in range(MODEL_B)]
    r16 = model.evaluate(samples, batch_size=MODEL_B, precision="bf16")
    r8 = model.evaluate(samples, batch_size=MODEL_B, precision="mxfp8")
    print("mAP bf16 %.4f, mxfp8 %.4f; AP50 %.4f / %.4f" % (r16["mAP"], r8["mAP"], r16["AP50"], r8["AP50"]))
    assert set(r8) == set(r16) and all(0.0 <= r8[k] <= 1.0 for k in ("mAP", "AP50", "AP75"))
    assert model.get_engine().last_forward == "mxfp8"
    with pytest.raises(ValueError):
        model.detect(image_, precision="fp16")
    # a model built without the switch still refuses, and loads what the one with the switch saved (and the reverse)
    path = str(tmp_path / "with_switch.pt")
    model.save(path)
    plain = make_model(tmp_path, seed=31)
    assert not plain.fp8_inference and plain.get_engine().bf16_only
    with pytest.raises(NotImplementedError, match="VGG-16"):
        plain.detect(image_, precision="mxfp8")
    assert plain.get_engine().last_forward == "bf16"
    plain.load(path)
    assert torch.equal(plain.get_engine().param, model.get_engine().param)
    a = model.detect(image_, score_thresh=SCORE_THRESH)
    b = plain.detect(image_, score_thresh=SCORE_THRESH)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    back = str(tmp_path / "without_switch.pt")
    plain.save(back)
    assert torch.load(back, map_location="cpu", weights_only=True)["network"] == torch.load(path, map_location="cpu", weights_only=True)["network"]
    model.load(back)
    c = model.detect(image_, score_thresh=SCORE_THRESH, precision="mxfp8")
    assert all(bool(torch.isfinite(t.float()).all()) for t in c)
