"""CPU: the strict harness itself (tests/strict.py).
  * The exact-operand regime of every case tests/test_conv_strict_gpu.py runs, asserted on the fp32 reference: every bf16
    output exactly representable in bf16, every fp32 sum below 2^24; for the small cases also fp32 == float64, bit for bit.
  * The arena, on CPU tensors with fake "kernels" that are wrong in one way each: every one of them must be reported.  No
    kernel may be broken on purpose on the GPU, so this is the evidence that the harness fails on a subtly wrong kernel."""
import pytest

torch = pytest.importorskip("torch")

from tests import strict                                                              # noqa: E402
from tests.conv_cases import CASES, FULL_SIZE_CASES                                   # noqa: E402


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
