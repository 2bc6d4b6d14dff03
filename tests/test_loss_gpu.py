"""GPU parity: fused SSD loss forward+backward (ssd_loss_fwd_bwd) vs the float64 oracle restatement of
models/ssd_model.py:341-396.  Tolerance: 1e-4 relative on the fp32 loss scalars (north star);
P and N exact; gradients 2e-5 absolute-relative mix for f32, bf16 rounding for bf16."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import ssd_oracle as O                                   # noqa: E402
from tests.helpers import golden_priors                              # noqa: E402


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def make_targets(ops, B, first=0, n_t=None):
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt
    pset = ops.build_priors()
    cls_l, box_l = synth_batch_gt(first, B, n_t)
    gt_box, gt_cls, gt_off, total, max_nt = ops.pack_gt(box_l, cls_l)
    return ops.match_encode(gt_box, gt_cls, gt_off, total, max_nt, pset, 0.5)


def run_case(ops, conf, loc, cls, gloc, mask, rtol=1e-4, gtol=2e-5):
    out, dconf, dloc = ops.ssd_loss(conf, loc, cls, gloc, mask)
    out = out.cpu().numpy()
    ref = O.ssd_loss(cls.cpu().numpy(), gloc.cpu().numpy(), mask.cpu().numpy(),
                     loc.float().cpu().numpy(), conf.float().cpu().numpy(), want_grad=True)
    assert out[7] == 0.0
    assert int(out[4]) == ref["num_pos"]
    for i, key in enumerate(["loc", "pos", "neg", "total"]):
        assert abs(out[i] - ref[key]) <= rtol * abs(ref[key]), (key, out[i], ref[key])
    # negatives: ties at tau are included (models/ssd_model.py:372); a 1-ulp difference in a key next to
    # tau may move an anchor across the threshold, so allow a handful of flips
    tau = out[6]
    assert abs(tau - ref["tau"]) <= 1e-5 * max(1.0, abs(ref["tau"]))
    assert abs(int(out[5]) - ref["num_neg"]) <= 2
    d = dconf.float().cpu().numpy().astype(np.float64)
    rows_ref = np.abs(ref["dcls"]).sum(-1) > 0
    rows_got = np.abs(d).sum(-1) > 0
    flips = rows_ref != rows_got
    assert flips.sum() <= 2
    same = ~flips
    scale = np.abs(ref["dcls"]).max()
    bound = gtol * scale + (0 if conf.dtype == torch.float32 else 4e-3 * scale)
    dl = dloc.float().cpu().numpy().astype(np.float64)
    lscale = np.abs(ref["dbox"]).max()
    lbound = (1e-6 if conf.dtype == torch.float32 else 4e-3) * lscale
    print("flips", int(flips.sum()), "error / bound: scalars", max(abs(out[i] - ref[k]) / max(rtol * abs(ref[k]), 1e-300) for i, k in
                                                                    enumerate(["loc", "pos", "neg", "total"])),
          "dconf", np.abs(d[same] - ref["dcls"][same]).max() / bound, "dloc", np.abs(dl - ref["dbox"]).max() / lbound)
    assert np.abs(d[same] - ref["dcls"][same]).max() <= bound
    assert np.abs(dl - ref["dbox"]).max() <= lbound
    return out, ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_loss_random_logits(ops, dtype):
    B, A, C = 4, 8732, 81
    cls, gloc, mask = make_targets(ops, B)
    g = torch.Generator(device="cuda").manual_seed(7)
    conf = torch.randn((B, A, C), generator=g, device="cuda", dtype=torch.float32).to(dtype)
    loc = (0.5 * torch.randn((B, A, 4), generator=g, device="cuda", dtype=torch.float32)).to(dtype)
    run_case(ops, conf, loc, cls, gloc, mask)


def test_loss_microbatch_of_default_yml(ops):
    # split_train.batch_size = 4 of the reference's config/default.yml:40-42: B=4 micro-batch, plus B=1
    for B in (1, 3):
        cls, gloc, mask = make_targets(ops, B, first=40 + B)
        g = torch.Generator(device="cuda").manual_seed(B)
        conf = 3.0 * torch.randn((B, 8732, 81), generator=g, device="cuda")
        conf[..., 80] += 2.0                       # background-heavy, like a trained net
        loc = torch.randn((B, 8732, 4), generator=g, device="cuda")
        run_case(ops, conf, loc, cls, gloc, mask)


def test_loss_ties_at_threshold(ops):
    """All-equal logits: every background CE is identical, tau equals it, and `>=` keeps every
    non-positive anchor (more than 3P of them)."""
    B, A, C = 2, 8732, 81
    cls, gloc, mask = make_targets(ops, B, first=9)
    conf = torch.zeros((B, A, C), device="cuda")
    loc = torch.zeros((B, A, 4), device="cuda")
    out, dconf, dloc = ops.ssd_loss(conf, loc, cls, gloc, mask)
    out = out.cpu().numpy()
    P = int(mask.sum())
    assert int(out[4]) == P and int(out[5]) == B * A - P and out[7] == 0
    np.testing.assert_allclose(out[1], np.log(81.0), rtol=1e-6)
    np.testing.assert_allclose(out[2], np.log(81.0), rtol=1e-6)
    ref = O.ssd_loss(cls.cpu().numpy(), gloc.cpu().numpy(), mask.cpu().numpy(), loc.cpu().numpy(), conf.cpu().numpy())
    np.testing.assert_allclose(out[0], ref["loc"], rtol=1e-5)


def test_loss_status_codes(ops):
    A, C = 256, 81
    conf = torch.randn((1, A, C), device="cuda")
    loc = torch.randn((1, A, 4), device="cuda")
    cls = torch.zeros((1, A), dtype=torch.int32, device="cuda")
    gloc = torch.zeros((1, A, 4), device="cuda")
    mask = torch.zeros((1, A), dtype=torch.uint8, device="cuda")
    out, _, _ = ops.ssd_loss(conf, loc, cls, gloc, mask)
    assert out.cpu().numpy()[7] == 1.0                        # P == 0: TF top_k(k=0)[-1] / division by zero
    mask[0, :100] = 1                                         # 3P = 300 > 256 anchors: TF top_k raises
    out, _, _ = ops.ssd_loss(conf, loc, cls, gloc, mask)
    assert out.cpu().numpy()[7] == 1.0
    mask[0, 70:] = 0                                          # P = 70, k = 210 > 186 negatives -> tau = 0
    out, _, _ = ops.ssd_loss(conf, loc, cls, gloc, mask)
    assert out.cpu().numpy()[7] == 2.0                        # reference assert at models/ssd_model.py:375


@pytest.mark.parametrize("where", ["logit_nan", "logit_inf", "offset_nan"])
def test_loss_flags_non_finite_inputs(ops, where):
    """status 3: the convolution epilogues are compiled without NaN semantics (ReLU may turn a NaN into 0), so the loss kernel is
    where a diverged run must show: one NaN / Inf logit anywhere, or a non-finite predicted offset of a positive, sets status 3
    in both forms of the loss (dense gradient and compact rows); clean inputs of the same shape give 0."""
    B, A, C = 2, 8732, 81
    cls, gloc, mask = make_targets(ops, B, first=17)
    g = torch.Generator(device="cuda").manual_seed(11)
    conf = torch.randn((B, A, C), generator=g, device="cuda").bfloat16()
    loc = (0.5 * torch.randn((B, A, 4), generator=g, device="cuda")).bfloat16()
    hw, npc = (1444, 361, 100, 25, 9, 1), (4, 6, 6, 6, 4, 4)
    npad = tuple((n * 85 + 7) // 8 * 8 for n in npc)
    hgb = ops.HeadGradBuffers(B, hw, npc, npad)
    assert float(ops.ssd_loss(conf, loc, cls, gloc, mask)[0][7]) == 0.0
    assert float(ops.ssd_loss_heads(conf, loc, cls, gloc, mask, hgb)[7]) == 0.0
    if where == "logit_nan":
        conf[1, 5000, 17] = float("nan")            # a background anchor somewhere in the middle
    elif where == "logit_inf":
        conf[0, 8731, 80] = float("inf")
    else:
        pos = mask[1].nonzero()[0, 0]
        loc[1, pos, 2] = float("nan")
    assert float(ops.ssd_loss(conf, loc, cls, gloc, mask)[0][7]) == 3.0
    assert float(ops.ssd_loss_heads(conf, loc, cls, gloc, mask, hgb)[7]) == 3.0


def test_loss_full_config_properties(ops):
    """BASELINE config 2 size (B=32, bf16): size-independent properties of the gradient."""
    B, A, C = 32, 8732, 81
    cls, gloc, mask = make_targets(ops, B, first=100)
    g = torch.Generator(device="cuda").manual_seed(3)
    conf = torch.randn((B, A, C), generator=g, device="cuda").to(torch.bfloat16)
    loc = torch.randn((B, A, 4), generator=g, device="cuda").to(torch.bfloat16)
    out, dconf, dloc = ops.ssd_loss(conf, loc, cls, gloc, mask)
    o = out.cpu().numpy()
    P, N = int(o[4]), int(o[5])
    assert P == int(mask.sum()) and N >= 3 * P and o[7] == 0
    d = dconf.float()
    nz = (d.abs().sum(-1) > 0)
    assert int(nz.sum()) == P + N                                # exactly the selected rows carry gradient
    assert float(d.sum(-1).abs().max()) < 2e-2 / P               # softmax - onehot sums to ~0 per row (bf16 rounding)
    assert int((dloc.float().abs().sum(-1) > 0).sum()) <= P
    # determinism: bitwise identical on a second run
    out2, dconf2, _ = ops.ssd_loss(conf, loc, cls, gloc, mask)
    assert torch.equal(out, out2) and torch.equal(dconf, dconf2)


def hand_targets(B, A, C, P, seed, device="cuda"):
    """targets without the 81-class prior set: a random mask with exactly P positives, random foreground classes, random offsets"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros((B * A,), dtype=torch.uint8)
    mask[torch.randperm(B * A, generator=g)[:P]] = 1
    cls = torch.randint(0, C - 1, (B, A), generator=g, dtype=torch.int32)
    gloc = torch.randn((B, A, 4), generator=g)
    return cls.to(device), gloc.to(device), mask.view(B, A).to(device)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [2, 21, 112, 288])
def test_loss_random_logits_any_class_count(ops, C, dtype):
    """k_loss_rows<T, 0> (any class count but 81) and the ragged last block on ordinary logits: __expf / __logf away from the
    exact regime of tests/test_loss_strict_gpu.py.  A = 301, B = 3: seven rows in the last block, a scalar tail for every C."""
    B, A = 3, 301
    cls, gloc, mask = hand_targets(B, A, C, 40, 5 + C)
    g = torch.Generator(device="cuda").manual_seed(C)
    conf = (2.0 * torch.randn((B, A, C), generator=g, device="cuda")).to(dtype)
    loc = (0.5 * torch.randn((B, A, 4), generator=g, device="cuda")).to(dtype)
    run_case(ops, conf, loc, cls, gloc, mask)
