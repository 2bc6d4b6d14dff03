"""GPU: ssd_ema_step (csrc/optim.hip) through the C ABI, in strict.Arena with guard bands and two poisons.

Exact case: om = 2^-3, p and e multiples of 2^-10 below 64 -- the difference is a multiple of 2^-10 below 128 (17 bits), the
product a multiple of 2^-13 below 16, the sum a multiple of 2^-13 below 64 (19 bits): nothing rounds, contracted or not, so the
comparison is an equality of bits.  om = 1 copies p's bits (-0.0, denormals), om = 0 keeps e's.  Random operands: every element
within tests/ema_oracle.step_bound of the float64 oracle; ten chained updates with the warm-up factors within the chained bound.
The regime is asserted on the operands and the oracle, never on what the kernel returned."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import ema_oracle as E                                     # noqa: E402
from tests import strict                                             # noqa: E402

BLK = 1024


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    lib = _lib.lib()
    assert lib.ssd_opt_block_elems() == BLK
    return lib


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.from_numpy(np.asarray(a, np.float64).astype(np.float32))


def exact32(a):
    a = np.asarray(a, np.float64)
    return np.array_equal(a.astype(np.float32).astype(np.float64), a)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def grid_operands(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randint(-65535, 65536, (n,), generator=g).double() / 1024).numpy()        # multiples of 2^-10, |.| < 64
    e = (torch.randint(-65535, 65536, (n,), generator=g).double() / 1024).numpy()
    return e, p


def mixed_operands(n, seed):
    """fp32 numbers of magnitudes 2^-20 .. 2^10, both signs, e and p of unrelated magnitudes."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        mant = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
        expo = torch.randint(-20, 10, (n,), generator=g).double()
        sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
        out.append((sign * mant * 2.0 ** expo).float().double().numpy())
    return out


def test_exact_updates_bit_for_bit(L):
    om = 2.0 ** -3
    big = 8 * BLK
    a = strict.Arena("cuda", strict.Arena.bytes_for(4 * BLK, 4 * BLK, 4 * 3 * BLK, 4 * 3 * BLK, 4 * big, 4 * big) + (4 << 20))
    for n in (BLK, 3 * BLK):
        e0, p0 = grid_operands(n, seed=n)
        want = E.ema_update(e0, p0, np.float32(om))
        assert exact32(p0 - e0) and exact32(om * (p0 - e0)) and exact32(want)             # the regime, on the oracle
        assert len(np.unique(want)) > n // 2
        p = a.put(f32(p0), "param[%d]" % n)
        e = a.inout(f32(e0), "ema[%d]" % n)
        got, = a.run(lambda: L.ssd_ema_step(ptr(e), ptr(p), n, om, stream()) == 0 or pytest.fail("refused"), [(e, f32(want))])
        assert torch.equal(bits(got), bits(f32(want)))
    # a 3-block slice starting at block 2 of a larger buffer: the blocks around it keep their values
    e0, p0 = grid_operands(big, seed=7)
    sl = slice(2 * BLK, 5 * BLK)
    want = e0.copy()
    want[sl] = E.ema_update(e0[sl], p0[sl], np.float32(om))
    assert exact32(want)
    p = a.put(f32(p0), "param[big]")
    e = a.inout(f32(e0), "ema[big]")
    written = torch.zeros(big, dtype=torch.bool)
    written[sl] = True
    a.run(lambda: L.ssd_ema_step(ptr(e[sl]), ptr(p[sl]), 3 * BLK, om, stream()) == 0 or pytest.fail("refused"),
          [(e, f32(want), written)])


def test_special_factors(L):
    """om = 1: e' is p bit for bit, whatever e held (NaN poison included: e is not read); om = 0: e keeps its bits."""
    n = 2 * BLK
    e0, p0 = grid_operands(n, seed=3)
    pt, et = f32(p0), f32(e0)
    tiny = np.float32(2.0 ** -149)
    pt[:8] = torch.tensor([-0.0, 0.0, float(tiny), -float(tiny), float(np.float32(2.0 ** -130)), 1e-40, -1e-45, 3.0 ** 0.5])
    et[:8] = torch.tensor([1.0, -0.0, 5.0, -0.0, 2.0 ** -140, -3.0, 0.0, float("nan")])
    et[8:12] = torch.tensor([-0.0, 2.0 ** -149, -2.0 ** -130, 0.0])
    assert bits(pt)[0] == -2 ** 31 and (pt[2:7] != 0).all()            # a signed zero, and the denormals survived the host
    a = strict.Arena("cuda", strict.Arena.bytes_for(4 * n, 4 * n, 4 * n) + (4 << 20))
    p = a.put(pt, "param")
    e = a.inout(et, "ema")
    got, = a.run(lambda: L.ssd_ema_step(ptr(e), ptr(p), n, 1.0, stream()) == 0 or pytest.fail("refused"), [(e, pt)])
    assert torch.equal(bits(got), bits(pt))
    fresh = a.out((n,), torch.float32, "ema (uninitialised)")           # initialisation: the poison is never read
    got, = a.run(lambda: L.ssd_ema_step(ptr(fresh), ptr(p), n, 1.0, stream()) == 0 or pytest.fail("refused"), [(fresh, pt)])
    assert torch.equal(bits(got), bits(pt))
    keep = et.clone()
    keep[7] = 4.0                                                      # (torch.equal cannot compare a NaN; bits are compared below)
    a.set(e, keep)
    got, = a.run(lambda: L.ssd_ema_step(ptr(e), ptr(p), n, 0.0, stream()) == 0 or pytest.fail("refused"), [(e, keep)])
    assert torch.equal(bits(got), bits(keep))


@pytest.mark.parametrize("om", [1e-4, 0.1, 0.9])
def test_random_operands_within_the_rounding_bound(L, om):
    n = 5 * BLK
    om32 = np.float32(om)
    e0, p0 = mixed_operands(n, seed=int(om * 1e4))
    lo, hi = np.abs(np.concatenate([e0, p0])).min(), np.abs(np.concatenate([e0, p0])).max()
    assert 2.0 ** -20 <= lo < 2.0 ** -18 and 2.0 ** 8 < hi < 2.0 ** 10
    want, bound = E.ema_update(e0, p0, om32), E.step_bound(e0, p0)
    assert (bound == 2.0 ** -22 * (np.abs(p0) + np.abs(e0))).all()
    a = strict.Arena("cuda", strict.Arena.bytes_for(4 * n, 4 * n) + (4 << 20))
    p = a.put(f32(p0), "param")
    e = a.inout(f32(e0), "ema")
    e.copy_(f32(e0))
    assert L.ssd_ema_step(ptr(e), ptr(p), n, float(om32), stream()) == 0
    got = e.cpu()
    err = np.abs(got.double().numpy() - want)
    print("om %g: max err / bound %.3f" % (om, float((err / bound).max())))
    assert (err <= bound).all(), int((err > bound).sum())
    assert float(np.abs(got.double().numpy() - e0).max()) > 0          # it moved
    # ... and the same bits under both poisons, guards and param intact
    a.run(lambda: L.ssd_ema_step(ptr(e), ptr(p), n, float(om32), stream()) == 0 or pytest.fail("refused"), [(e, got)])


def test_ten_chained_updates_with_warmup_factors(L):
    n, T, decay = 3 * BLK, 10, 0.9998
    e0, _ = mixed_operands(n, seed=21)
    params = [mixed_operands(n, seed=30 + k)[1] for k in range(T)]
    want, bound = E.ema_chain(e0, params, decay, warmup=True)
    a = strict.Arena("cuda", strict.Arena.bytes_for(4 * n, 4 * n) + (4 << 20))
    p = a.put(f32(params[0]), "param")
    e = a.inout(f32(e0), "ema")
    cur = f32(e0)
    for k in range(T):
        a.set(p, f32(params[k]))
        a.set(e, cur)
        om = float(E.one_minus_decay(k, decay))
        assert om == float(np.float32(1.0 - (1.0 + k) / (10.0 + k)))    # all ten are warm-up factors
        # (the reference is this call's own first result: a.run then asserts guards, the input and two-poison determinism)
        e.copy_(cur)
        assert L.ssd_ema_step(ptr(e), ptr(p), n, om, stream()) == 0
        nxt = e.cpu()
        a.run(lambda: L.ssd_ema_step(ptr(e), ptr(p), n, om, stream()) == 0 or pytest.fail("refused"), [(e, nxt)])
        cur = nxt
    err = np.abs(cur.double().numpy() - want)
    print("chained: max err / bound %.3f" % float((err / bound).max()))
    assert (err <= bound).all(), int((err > bound).sum())


def test_grid_coverage_far_blocks(L):
    """n = 4097 * 1024: one block per 1024 elements, no grid cap -- every element of every block against the oracle (exact
    operands, so the comparison is an equality)."""
    n, om = 4097 * BLK, 2.0 ** -3
    g = torch.Generator(device="cuda").manual_seed(5)
    p = torch.randint(-65535, 65536, (n,), generator=g, device="cuda").float() / 1024
    e0 = torch.randint(-65535, 65536, (n,), generator=g, device="cuda").float() / 1024
    want = (e0.double() + om * (p.double() - e0.double()))
    assert torch.equal(want.float().double(), want)                    # the regime: the oracle's result is an fp32 number
    e, p_before = e0.clone(), p.clone()
    assert L.ssd_ema_step(ptr(e), ptr(p), n, om, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(e.double(), want), strict.first_diff(e.double(), want)
    assert torch.equal(p, p_before)
    assert not torch.equal(e[-BLK:], e0[-BLK:]) and not torch.equal(e[:BLK], e0[:BLK])


def test_refusals_launch_nothing(L):
    from ssd_object_detection_amd import _lib
    n = 2 * BLK
    a = strict.Arena("cuda", strict.Arena.bytes_for(4 * n, 4 * n) + (4 << 20))
    p = a.put(torch.ones(n), "param")
    e = a.out((n,), torch.float32, "ema")

    def refused(*args):
        def fn():
            assert L.ssd_ema_step(*args, stream()) == _lib.SSD_ERR_VALUE, args
        return fn

    for args in ((None, ptr(p), n, 0.5), (ptr(e), None, n, 0.5), (ptr(e), ptr(p), 0, 0.5), (ptr(e), ptr(p), -BLK, 0.5),
                 (ptr(e), ptr(p), BLK + 4, 0.5), (ptr(e), ptr(p), BLK - 1, 0.5), (ptr(e), ptr(p), n, float("nan")),
                 (ptr(e), ptr(p), n, -0.5), (ptr(e), ptr(p), n, 1.5), (ptr(e), ptr(e), n, 0.5), (ptr(e), ptr(e[4:]), BLK, 0.5),
                 (ptr(e[BLK:]), ptr(e[4:]), BLK, 0.5)):
        a.run(refused(*args), [])                                      # the output keeps its poison, the input its values
    from ssd_object_detection_amd import ops
    with pytest.raises(ValueError):
        ops.ema_step(e, p, 1.5)
    with pytest.raises(ValueError):
        ops.ema_step(e[:BLK + 4], p[:BLK + 4], 0.5)
    got, = a.run(lambda: ops.ema_step(e, p, 1.0), [(e, torch.ones(n))])
    assert torch.equal(got.cpu(), torch.ones(n))
