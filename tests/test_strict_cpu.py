"""CPU: the strict harness itself (tests/strict.py).
  * The exact-operand regime of every case tests/test_conv_strict_gpu.py runs, asserted on the fp32 reference: every bf16
    output exactly representable in bf16, every fp32 sum below 2^24; for the small cases also fp32 == float64, bit for bit.
  * The arena, on CPU tensors with fake "kernels" that are wrong in one way each: every one of them must be reported.  No
    kernel may be broken on purpose on the GPU, so this is the evidence that the harness fails on a subtly wrong kernel."""
import pytest

torch = pytest.importorskip("torch")

from tests import strict                                                              # noqa: E402
from tests.conv_cases import CASES, FULL_SIZE_CASES, RESNET_CASES                     # noqa: E402


# ---------------------------------------------------------------- the regime
@pytest.mark.parametrize("case", CASES, ids=[str(c[:8]) for c in CASES])
def test_conv_case_regime(case):
    r = strict.conv_reference(case)
    strict.check_conv_regime(case, r)
    r64 = strict.conv_reference(case, dtype=torch.float64)
    for name in ("y", "y_relu", "dx", "dx_acc", "dw", "dbias"):
        assert torch.equal(r[name].double(), r64[name]), name


@pytest.mark.parametrize("case", FULL_SIZE_CASES, ids=[str(c[:8]) for c in FULL_SIZE_CASES])
def test_full_size_case_regime(case):
    B = strict.smallest_batch(case)
    print("batch used for %s: %d" % (str(case[:8]), B))
    case = (B,) + tuple(case[1:])
    strict.check_conv_regime(case, strict.conv_reference(case))


@pytest.mark.parametrize("case", RESNET_CASES, ids=[str(c[:8]) for c in RESNET_CASES])
def test_resnet_case_regime(case):
    """as test_conv_case_regime; fp32 == float64 where no tensor of the case has 4M elements (the one-image cases on large maps
    are in the regime by the same conditions, which do not depend on the map's size)"""
    r = strict.conv_reference(case)
    strict.check_conv_regime(case, r)
    if max(r["x"].numel(), r["y"].numel()) < 1 << 22:
        r64 = strict.conv_reference(case, dtype=torch.float64)
        for name in ("y", "y_relu", "dx", "dx_acc", "dw", "dbias"):
            assert torch.equal(r[name].double(), r64[name]), name
    if case[5] == 1 and case[6] == 2:
        # 1x1 stride 2: only the pixels (2i, 2j) have a tap, so about three quarters of dx are exact zeros
        B, H, W = case[:3]
        zeros = float((r["dx"] == 0).float().mean())
        assert zeros >= 1 - (-(-H // 2) * -(-W // 2)) / (H * W), zeros
        assert bool((r["dx"][:, 1::2] == 0).all()) and bool((r["dx"][:, :, 1::2] == 0).all())
        assert bool((r["dx_acc"][:, 1::2] != 0).any()), "the masked base must show where no tap reaches"


RESNET_HEADS = [(2, 1, 1, 256, 4), (2, 2, 2, 256, 4), (2, 4, 4, 256, 6), (2, 16, 16, 512, 6), (2, 60, 58, 64, 4)]


@pytest.mark.parametrize("shape", RESNET_HEADS, ids=str)
def test_resnet_head_regime(shape):
    """the head shapes tests/test_conv_strict_gpu.py::test_head_fwd_and_grad_pack_strict adds for the ResNet-50 SSD512"""
    strict.check_regime(strict.head_case(*shape))


@pytest.mark.parametrize("name", sorted(strict.EXTRAS), ids=str)
def test_extra_case_regime(name):
    r = strict.EXTRAS[name]()
    strict.check_regime(r)
    if r.get("f64") is not None:
        r64 = r["f64"]()
        for key in r["exact"]:
            assert torch.equal(r[key].double(), r64[key].double()), key


def test_mx_fp8_round_trip_of_the_integer_operands():
    """{+-1, +-2} (amax 2: scale 2^-7, elements 128 and 256) and thinned {-1, 0, 1} are exact in MX e4m3"""
    g = torch.Generator().manual_seed(1)
    for t in (strict.ints(g, (3, 5, 128), (-2, -1, 1, 2)), strict.ints(g, (64, 3, 3, 128), (-1, 1), 0.2),
              torch.zeros((2, 64), dtype=torch.bfloat16)):
        q, s = strict.ref_quantize_mx(t)
        assert torch.equal(strict.ref_dequantize_mx(q, s), t.float())


# ---------------------------------------------------------------- the arena's own checks
N = 1000


def make_arena():
    a = strict.Arena("cpu", strict.Arena.bytes_for(4 * N, 4 * N, 2 * N, 64))
    x = a.put(torch.arange(N, dtype=torch.float32), "x")
    y = a.out((N,), torch.float32, "y")
    return a, x, y, a.workspace()


def flat_bytes(a, t):
    """the arena's bytes from the tensor's first byte on (what a stray pointer sees)"""
    off = t.data_ptr() - a.buf.data_ptr()
    return a.buf, off


def test_arena_layout():
    a, x, y, ws = make_arena()
    w = ws.get(52, "cpu")
    for t in (x, y, w):
        assert t.data_ptr() % 256 == 0
    assert w.numel() == 52 and w.dtype == torch.uint8 and ws.get(52, "cpu") is w
    s = a._slot_of(y)
    assert s.nbytes == 4 * N and strict.GUARD == 1 << 20
    # the guards touch the tensor: the word just before and the word just past it are poison, viewed in its own type
    buf, off = flat_bytes(a, y)
    assert buf[off - 4:off].view(torch.int32).item() == 0x7FA5A5A5 and buf[off + 4 * N:off + 4 * N + 4].view(torch.int32).item() == 0x7FA5A5A5
    assert bool(torch.isnan(y).all())
    z = a.out((N,), torch.bfloat16, "z")
    assert z.view(torch.int16)[0].item() == 0x7FA5 and bool(torch.isnan(z.float()).all())


def test_arena_passes_a_correct_kernel():
    a, x, y, ws = make_arena()

    def good():
        w = ws.get(4 * N, "cpu").view(torch.float32)
        w.copy_(x)
        y.copy_(w * 2)
    (got,) = a.run(good, [(y, torch.arange(N, dtype=torch.float32) * 2)])
    assert torch.equal(got, torch.arange(N, dtype=torch.float32) * 2)


def check_reported(a, fn, expect, what):
    with pytest.raises(strict.StrictError, match=what):
        a.run(fn, expect)


def test_arena_reports_a_write_past_the_end():
    a, x, y, ws = make_arena()
    buf, off = flat_bytes(a, y)

    def bad():
        y.copy_(x * 2)
        buf[off + 4 * N:off + 4 * N + 4].view(torch.float32).fill_(2.0 * N)      # element N
    check_reported(a, bad, [(y, x.clone() * 2)], "write past the end of y")


def test_arena_reports_a_write_before_the_start():
    a, x, y, ws = make_arena()
    buf, off = flat_bytes(a, y)

    def bad():
        y.copy_(x * 2)
        buf[off - 4:off].view(torch.float32).fill_(-2.0)                           # element -1
    check_reported(a, bad, [(y, x.clone() * 2)], "write before the start of y")


def test_arena_reports_an_element_left_unwritten():
    a, x, y, ws = make_arena()

    def bad():
        y[:N - 1].copy_(x[:N - 1] * 2)
    check_reported(a, bad, [(y, x.clone() * 2)], r"y differs from the reference: 1 of 1000 elements differ, first at \(999,\)")


def test_arena_reports_an_unwritten_element_that_already_held_the_answer():
    """what the caching allocator does to the existing re-run tests: stale memory that is already right"""
    a, x, y, ws = make_arena()
    want = x.clone() * 2
    y.copy_(want)

    def bad():
        y[1:].copy_(x[1:] * 2)
    check_reported(a, bad, [(y, want)], r"y differs from the reference: 1 of 1000 elements differ, first at \(0,\)")


def test_arena_reports_a_guard_value_added_into_the_result():
    a, x, y, ws = make_arena()
    buf, off = flat_bytes(a, x)

    def bad():
        y.copy_(x * 2)
        y[N - 1] += buf[off + 4 * N:off + 4 * N + 4].view(torch.float32)[0]       # reads x[N]
    check_reported(a, bad, [(y, x.clone() * 2)], "y differs from the reference")


def test_arena_reports_a_read_of_unwritten_scratch_that_stays_finite():
    """~P is no NaN (bf16 0x805A is a denormal): such a read shows as a difference between the two poisons at the latest"""
    a, x, y, ws = make_arena()

    def bad():
        w = ws.get(64, "cpu")
        y.copy_(x * 2)
        y[3] = float(w[5].item() > 0x80)                                           # 0xA5 -> 1, 0x5A -> 0
    with pytest.raises(strict.StrictError) as e:
        a.run(bad, [(y, x.clone() * 2)])
    assert "differs between the two poisons" in str(e.value) or "differs from the reference" in str(e.value)


def test_arena_reports_a_modified_input():
    a, x, y, ws = make_arena()

    def bad():
        y.copy_(x * 2)
        x[17] = 0.0
    check_reported(a, bad, [(y, torch.arange(N, dtype=torch.float32) * 2)], r"input x was modified: 1 of 1000 elements differ, first at \(17,\)")


def test_arena_reports_one_byte_past_an_exact_size_workspace():
    a, x, y, ws = make_arena()
    buf = a.buf

    def bad():
        w = ws.get(53, "cpu")
        w.fill_(0)
        off = w.data_ptr() - buf.data_ptr()
        buf[off + 53] = 0                                                            # byte 53 of a 53-byte workspace
        y.copy_(x * 2)
    check_reported(a, bad, [(y, x.clone() * 2)], r"write past the end of workspace\[53\]: 1 guard words changed, nearest within 1 bytes")


def test_arena_reports_a_write_outside_the_documented_extent():
    a, x, y, ws = make_arena()
    written = torch.zeros(N, dtype=torch.bool)
    written[10:] = True

    def good():
        y[10:].copy_(x[10:] * 2)

    def bad():
        y[9:].copy_(x[9:] * 2)
    a.run(good, [(y, x.clone() * 2, written)])
    check_reported(a, bad, [(y, x.clone() * 2, written)], "y was written outside its documented extent")


def test_arena_reports_an_output_the_call_does_not_list():
    a, x, y, ws = make_arena()
    z = a.out((8,), torch.bfloat16, "z")

    def bad():
        y.copy_(x * 2)
        z[0] = 1.0
    check_reported(a, bad, [(y, x.clone() * 2)], "z was written although the call does not list it")


# ---------------------------------------------------------------- seeded faults of the ResNet regimes (torch restatements)
def conv_fault_arena(case):
    r = strict.conv_reference(case)
    strict.check_conv_regime(case, r)
    B, H, W, Cin, Cout = case[:5]
    Ho, Wo = r["geom"][:2]
    a = strict.Arena("cpu", 64 << 20)
    t = dict(y=a.out((B, Ho, Wo, Cout), torch.bfloat16, "y"), dx=a.out((B, H, W, Cin), torch.bfloat16, "dx"),
             acc=a.inout(r["base"], "dx (accumulated onto)"))
    return r, a, t


def test_arena_reports_a_strided_1x1_data_gradient_that_skips_the_classes_without_a_tap():
    """1x1 stride 2: of the four parity classes of dx only (even, even) has a tap; a kernel that returns from a class whose k
    loop is empty leaves three quarters of dx unwritten"""
    case = (3, 17, 17, 64, 128, 1, 2, "same")
    r, a, t = conv_fault_arena(case)
    want = r["dx"].to(torch.bfloat16)

    def good():
        t["dx"].zero_()
        t["dx"][:, ::2, ::2] = want[:, ::2, ::2]

    def bad():
        t["dx"][:, ::2, ::2] = want[:, ::2, ::2]
    a.run(good, [(t["dx"], want)])
    untouched = want.numel() - want[:, ::2, ::2].numel()
    check_reported(a, bad, [(t["dx"], want)], r"dx differs from the reference: %d of %d elements differ, first at \(0, 0, 1, 0\)"
                   % (untouched, want.numel()))


def test_arena_reports_a_strided_1x1_data_gradient_that_zeroes_the_base_it_accumulates_onto():
    """the same under accumulate with a ReLU mask: a class without a tap must hold the masked base, not 0"""
    case = (2, 18, 18, 128, 256, 1, 2, "same")
    r, a, t = conv_fault_arena(case)
    want = r["dx_acc"].to(torch.bfloat16)
    keep = r["mask_src"].float() > 0

    def good():
        dx = torch.zeros_like(r["dx"])
        dx[:, ::2, ::2] = r["dx"][:, ::2, ::2]
        t["acc"].copy_(strict.masked(dx + t["acc"].float(), keep))

    def bad():
        out = strict.masked(r["dx"] + t["acc"].float(), keep)
        t["acc"].zero_()                                       # the classes without a tap: "no gradient" stored as 0
        t["acc"][:, ::2, ::2] = out[:, ::2, ::2].to(torch.bfloat16)
    a.run(good, [(t["acc"], want)])
    check_reported(a, bad, [(t["acc"], want)], r"dx \(accumulated onto\) differs from the reference")


def test_arena_reports_a_7x7_stem_padded_3_3_where_same_gives_2_3():
    """7x7 stride 2 at an even size: SAME pads 5 in all, 2 before and 3 after; 3 before shifts every tap by one pixel"""
    case = (2, 32, 32, 8, 64, 7, 2, "same")
    r, a, t = conv_fault_arena(case)
    Ho, Wo, pt, pl = r["geom"]
    assert (pt, pl) == (2, 2) and strict.geometry(37, 37, 7, 2, "same")[2:] == (3, 3)

    def conv(pad):
        return lambda: t["y"].copy_(strict.ref_conv(r["x"].float(), r["w"].float(), r["bias"], 7, 2, pad, pad, Ho, Wo, False))
    a.run(conv(2), [(t["y"], r["y"].to(torch.bfloat16))])
    check_reported(a, conv(3), [(t["y"], r["y"].to(torch.bfloat16))], "y differs from the reference")


# ---------------------------------------------------------------- the exact loss cases
import numpy as np                                                                  # noqa: E402


@pytest.mark.parametrize("name", sorted(strict.LOSS_CASES), ids=str)
def test_loss_case_regime(name):
    strict.check_loss_regime(strict.loss_cached(name))


@pytest.mark.parametrize("name", sorted(strict.HEADS_LOSS_CASES), ids=str)
def test_heads_loss_case_regime(name):
    r = strict.heads_cached(name)
    strict.check_loss_regime(r)
    assert r["pow2"] and r["N"] == 4 * r["P"], "P, N and grad_scale are powers of two in every case that feeds the head kernels"
    for l in r["levels"]:
        k = l["count"]
        assert bool((l["pixel_of_row"][1:] > l["pixel_of_row"][:-1]).all()) and int((l["row_of_pixel"] >= 0).sum()) == k
        assert not bool((l["rows"][:, l["n"] * (4 + r["C"]):] != 0).any())
    mask = r["gt_mask"].numpy().reshape(-1).astype(bool)
    assert int(((r["pos_ce"] == 0) & mask).sum()) > 0, "a selected positive with an all-zero row"


def test_loss_catalogue_covers_what_it_names():
    """the radix digits that decide, the tie shapes, the block shapes: properties of the inputs"""
    def keys(name):
        r = strict.loss_cached(name)
        return r, r["key"][~r["gt_mask"].numpy().reshape(-1).astype(bool)].view(np.uint32), int(r["out8"][6:7].view(torch.int32))
    for name in ("level3 first (2,300,21) f32", "level3 middle (2,300,21) f32", "level3 last (2,300,21) f32"):
        r, k, tau = keys(name)
        near = k[(k >> 21) == (tau >> 21)]
        assert len(set(near >> 10)) == 1 and len(set(near & 1023)) > 500            # one level-2 bin, the low digit decides
        assert sorted(set(np.diff(np.unique(near)))) == [1]                       # consecutive floats
    assert [strict.loss_cached("level3 %s (2,300,21) f32" % n)["design"]["rank_in_tie"] for n in ("first", "middle", "last")] == [1, 3, 5]
    r, k, tau = keys("level3 all 1024 low digits (4,500,21) f32")
    assert len(set(k[(k >> 10) == (tau >> 10)] & 1023)) == 1024
    r, k, tau = keys("level2 (4,500,5) f32")
    near = k[(k >> 21) == (tau >> 21)]
    assert len(set(near >> 10)) >= 1499 and len(set((near >> 10) & 2047) & set(range(0, 2048, 8))) > 100    # every owner thread
    r, k, tau = keys("level1 (3,301,21) f32")
    assert len(set(k >> 21)) >= 473 and k.max() == 0x7F7FFFFF and (k >> 21).min() <= 0x224
    for tag in ("f32", "bf16"):
        r = strict.loss_cached("tie straddles 3P (2,300,21) %s" % tag)
        assert r["N"] > 3 * r["P"] and (r["key"] == 0).sum() > r["P"]               # background-is-maximum rows below tau
        r = strict.loss_cached("tie ends at 3P (2,300,21) %s" % tag)
        assert r["N"] == 3 * r["P"] and r["design"]["tie"] > 1
        r = strict.loss_cached("every negative (2,128,21) %s" % tag)
        assert r["N"] == 3 * r["P"] == r["B"] * r["A"] - r["P"]
        r = strict.loss_cached("odd tail (3,301,21) %s" % tag)
        assert (r["B"] * r["A"]) % 128 % 2 == 1 and ((r["B"] * r["A"]) % 128 * r["C"]) % 4 != 0
    for name in ("persistent (5,19661,81) bf16", "persistent (5,19661,4) f32"):
        r = strict.loss_cached(name)
        assert r["B"] * r["A"] >= 98305 and r["conf"].numel() * r["conf"].element_size() <= 16 << 20


def fake_loss(r, ge=True, rank_shift=0):
    """The loss restated for the exact regime in plain fp32 numpy (the softmax is the one-hot of the row maximum), with the two
    classic mistakes of a selection as switches.  Returns out8, dconf, dloc, selected."""
    B, A, C, gs = r["B"], r["A"], r["C"], np.float32(r["grad_scale"])
    n = B * A
    z = r["conf"].float().numpy().reshape(n, C)
    mask = r["gt_mask"].numpy().reshape(n).astype(bool)
    cls = r["gt_cls"].numpy().reshape(n)
    m = z.max(-1)
    key = np.where(mask, np.float32(0), m - z[:, C - 1])
    P = int(mask.sum())
    tau = np.sort(key)[::-1][3 * P + rank_shift - 1]
    neg = ~mask & ((key >= tau) if ge else (key > tau))
    N = int(neg.sum())
    label = np.where(mask, cls, C - 1)
    onehot = (np.arange(C)[None, :] == label[:, None]).astype(np.float32)
    sc = np.where(mask, gs / np.float32(P), gs / np.float32(N)) * (mask | neg)
    dconf = ((z == m[:, None]).astype(np.float32) - onehot) * sc[:, None].astype(np.float32) + np.float32(0)
    d = r["loc"].float().numpy().reshape(n, 4) - r["gt_loc"].numpy().reshape(n, 4)
    dloc = np.sign(d) * (mask[:, None] * (gs / np.float32(P))) + np.float32(0)
    ce = (m - z[np.arange(n), cls])[mask].astype(np.float64).sum() / P
    out = np.array([np.abs(d)[mask].astype(np.float64).sum() / P, ce, key[neg].astype(np.float64).sum() / N, 0, P, N, tau, 0], dtype=np.float32)
    out[3] = (out[0] + out[1]) + out[2]
    dt = r["dtype"]
    return (torch.from_numpy(out), torch.from_numpy(dconf.astype(np.float32)).view(B, A, C).to(dt),
            torch.from_numpy(dloc.astype(np.float32)).view(B, A, 4).to(dt), mask | neg)


def loss_arena(r):
    a = strict.Arena("cpu", 64 << 20)
    return a, a.out((8,), torch.float32, "out8"), a.out(tuple(r["dconf"].shape), r["dtype"], "dconf"), a.out(tuple(r["dloc"].shape), r["dtype"], "dloc")


def run_fake(r, **kw):
    a, out8, dconf, dloc = loss_arena(r)

    def fn():
        o, dc, dl, _ = fake_loss(r, **kw)
        out8.copy_(o); dconf.copy_(dc); dloc.copy_(dl)
    return a.run(fn, [(out8, r["out8"]), (dconf, r["dconf"]), (dloc, r["dloc"])])


@pytest.mark.parametrize("name", ["tie straddles 3P (2,300,21) f32", "tie straddles 3P (2,300,21) bf16", "level3 middle (2,300,21) f32",
                                  "level1 (3,301,21) f32", "odd tail (3,301,21) bf16", "C=2 (3,301,2) f32"])
def test_arena_passes_a_correct_fake_loss(name):
    """an fp32 restatement of the kernel's formulas gives the expected outputs bit for bit: the expectation does not lean on
    float64"""
    run_fake(strict.loss_cached(name))


def test_arena_reports_a_loss_that_selects_with_greater_than():
    r = strict.loss_cached("tie straddles 3P (2,300,21) f32")
    with pytest.raises(strict.StrictError) as e:
        run_fake(r, ge=False)
    assert "out8 differs from the reference" in str(e.value) and "dconf differs from the reference" in str(e.value)


@pytest.mark.parametrize("shift", [-1, 1])
def test_arena_reports_a_loss_that_is_off_by_one_rank(shift):
    """consecutive floats around the threshold: one rank is one ulp of tau and one row of dconf"""
    r = strict.loss_cached("level3 last (2,300,21) f32" if shift == 1 else "level3 first (2,300,21) f32")
    with pytest.raises(strict.StrictError) as e:
        run_fake(r, rank_shift=shift)
    assert "out8 differs from the reference" in str(e.value) and "dconf differs from the reference" in str(e.value)


def heads_fake_arena(r):
    a = strict.Arena("cpu", 64 << 20)
    B = r["B"]
    t = dict(rows=[a.out((B * l["hw"], l["npad"]), torch.bfloat16, "rows[%d]" % i) for i, l in enumerate(r["levels"])],
             por=[a.out((B * l["hw"],), torch.int32, "pixel_of_row[%d]" % i) for i, l in enumerate(r["levels"])],
             count=a.out((8,), torch.int32, "count"))
    expect = []
    nl = len(r["levels"])
    counts = torch.zeros((8,), dtype=torch.int32)
    counts[:nl] = torch.tensor([l["count"] for l in r["levels"]], dtype=torch.int32)
    expect.append((t["count"], counts, torch.arange(8) < nl))
    for i, l in enumerate(r["levels"]):
        first = torch.arange(B * l["hw"]) < l["count"]
        por = torch.zeros((B * l["hw"],), dtype=torch.int32)
        por[:l["count"]] = l["pixel_of_row"]
        expect += [(t["por"][i], por, first), (t["rows"][i], l["rows"], first[:, None].expand(-1, l["npad"]).clone())]

    def good():
        t["count"][:nl] = counts[:nl]
        for i, l in enumerate(r["levels"]):
            k = l["count"]
            t["por"][i][:k] = l["pixel_of_row"]
            t["rows"][i][:k] = l["rows"][:k]
    return a, t, expect, good, nl


def test_arena_reports_a_stale_row_behind_count_and_a_write_of_count_levels():
    r = strict.heads_cached("1 level B=1 C=5")
    a, t, expect, good, nl = heads_fake_arena(r)
    a.run(good, expect)
    k = r["levels"][0]["count"]

    def stale_row():
        good()
        t["rows"][0][k] = 0                                                          # a zero-filled row nobody asked for
    check_reported(a, stale_row, expect, r"rows\[0\] was written outside its documented extent")

    def stale_index():
        good()
        t["por"][0][k] = 0
    check_reported(a, stale_index, expect, r"pixel_of_row\[0\] was written outside its documented extent")

    def count_levels():
        good()
        t["count"][nl] = 0
    check_reported(a, count_levels, expect, "count was written outside its documented extent")


# ---------------------------------------------------------------- the sparse head backward cases
@pytest.mark.parametrize("name", sorted(strict.SPARSE_CASES), ids=str)
def test_sparse_case_regime(name):
    case = strict.sparse_cached(name)
    strict.check_sparse_regime(case["levels"])
    for l in case["levels"]:
        k, por, rop = l["count"], l["pixel_of_row"], l["row_of_pixel"]
        assert bool((por[:k][1:] > por[:k][:-1]).all()) and int((rop >= 0).sum()) == k
        assert torch.equal(rop[por[:k].long()], torch.arange(k, dtype=torch.int32))
        assert bool((l["rows"][k:].float() == strict.UNREAD).all())
        vals = set(l["rows"][:k].float().abs().unique().tolist())
        assert vals <= {0.0, 2.0 ** -6, 2.0 ** -8}
        assert not bool((l["rows"][:k, l["cout"]:] != 0).any())
        if case["relu"] != "none":
            assert bool((l["x"] >= 0).all()) and bool((l["x"] == 0).any())
        # the reference of the weight gradient in float64 is the same number
        dy = torch.zeros((case["B"] * l["hw"], l["npad"]))
        dy[por[:k].long()] = l["rows"][:k].float()
        dy = dy.view(case["B"], l["H"], l["W"], l["npad"])[..., :l["cout"]].contiguous()
        _, dw64, db64 = strict.head_bwd_reference(l["x"].double(), l["w"].double(), dy.double())
        assert torch.equal(dw64, l["dw"].double()) and torch.equal(db64.double(), l["dbias"].double())


def test_sparse_catalogue_covers_what_it_names():
    counts = sorted(l["count"] for n in strict.SPARSE_CASES for l in strict.sparse_cached(n)["levels"])
    assert {0, 1, 127, 128, 129, 768, 1444} <= set(counts)
    b1 = strict.sparse_cached("B=1 bits")
    assert all((b1["B"] * l["hw"]) % 4 for l in b1["levels"]) and any(l["H"] != l["W"] for l in b1["levels"])
    full = b1["levels"][1]
    assert full["count"] == full["hw"]                                                  # every corner and edge of a 7 x 5 map
    assert {l["cout"] for n in strict.SPARSE_CASES for l in strict.sparse_cached(n)["levels"]} == {36, 340, 510}
    assert {l["Cin"] for n in strict.SPARSE_CASES for l in strict.sparse_cached(n)["levels"]} == {128, 256}
    for l in strict.sparse_cached("B=1 bits")["levels"][:1] + strict.sparse_cached("B=4 splits")["levels"]:
        k, por = l["count"], l["pixel_of_row"]
        assert {0, l["W"] - 1, (l["H"] - 1) * l["W"], l["hw"] - 1} <= set(por[:k].tolist())


def test_chained_case_regime():
    c = strict.chained_case()
    strict.check_sparse_regime(c["levels"])
    strict.check_loss_regime(c["loss"])
    assert len(c["levels"]) == 7 and c["loss"]["pow2"]
