"""Inputs for the MultiBox loss tests.  Plain Python / numpy / CPU torch: importable without a GPU.

hand_case: random logits with hand-made masks (P_b chosen per image), compared against tests/multibox_oracle.py by tolerance.
exact_case: the regime of tests/strict.py's loss cases -- one maximum m per row, one chosen logit m - v with v = 0 or v >= 1024,
fill logits <= m - 1024 elsewhere -- in which exp(z - m) is exactly 0 or 1 in fp32 and in float64: every key, every CE and
every sum is exact, the softmax is exactly one-hot, and with P, loc_weight and grad_scale powers of two and offsets multiples
of 1/4 the float64 oracle's out8 / dconf / dloc convert to the output dtype without rounding.  They are expected bit for bit."""
import numpy as np
import torch

from tests import multibox_oracle as M
from tests import strict

SSD300_GEOM = ((38, 38, 4), (19, 19, 6), (10, 10, 6), (5, 5, 6), (3, 3, 4), (1, 1, 4))


def hand_case(B, A, C, P_b, seed, dtype=torch.float32, offsets="random"):
    """conf = 3 randn with the background logit raised by 2, P_b positives at seeded random places of image b.
    offsets "edges": the differences loc - gt_loc of the positives cycle through 0, +-0.5, +-1 (exactly), +-1.25, +-3."""
    g = torch.Generator().manual_seed(seed)
    conf = 3.0 * torch.randn((B, A, C), generator=g)
    conf[..., C - 1] += 2.0
    mask = torch.zeros((B, A), dtype=torch.uint8)
    for b, p in enumerate(P_b):
        mask[b, torch.randperm(A, generator=g)[:p]] = 1
    gt_cls = torch.randint(0, C - 1, (B, A), generator=g, dtype=torch.int32)
    gt_loc = torch.randint(-8, 9, (B, A, 4), generator=g).float() / 4
    if offsets == "edges":
        d = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 1.25, -1.25, 3.0, -3.0])
        loc = gt_loc + d[torch.arange(B * A * 4).view(B, A, 4) % 9]          # multiples of 1/4: exact in bf16 too
    else:
        loc = torch.randn((B, A, 4), generator=g)
    return dict(B=B, A=A, C=C, dtype=dtype, conf=conf.to(dtype), loc=loc.to(dtype), gt_cls=gt_cls, gt_loc=gt_loc, gt_mask=mask)


def oracle_of(r, ratio=3, alpha=1.0, gs=1.0):
    """the float64 oracle on the values the kernel reads (the inputs cast to their dtype, then widened)"""
    return M.multibox_loss(r["gt_cls"].numpy(), r["gt_loc"].numpy(), r["gt_mask"].numpy(), r["loc"].float().numpy(),
                           r["conf"].float().numpy(), ratio, alpha, gs)


def _pow2(v):
    return v > 0 and float(np.log2(v)).is_integer()


def image_keys(A, P_b, ratio, top, tie_value, tie, rank_in_tie, below=(), seed=0, dtype=torch.float32):
    """The A - P_b candidate keys of one image: ratio * P_b - rank_in_tie keys of `top` (all above tie_value) over a tie group of
    `tie` keys at tie_value, whose member rank_in_tie is the threshold; `below`: keys under tie_value (sharing radix digits with
    it); the rest are exact zeros and keys of [1024, 1536).  Unordered."""
    above = ratio * P_b - rank_in_tie
    top = np.sort(np.asarray(top, dtype=np.float32))[:above]
    below = np.asarray(below, dtype=np.float32)
    assert top.size == above and (top > tie_value).all() and tie_value >= 1536 and 1 <= rank_in_tie <= tie and (below < tie_value).all()
    rest = A - P_b - above - tie - below.size
    assert rest >= 0
    return np.concatenate([top, np.full(tie, tie_value, dtype=np.float32), below, strict._fill_keys(rest, seed, dtype)])


def exact_case(B, A, C, mask, key, dtype=torch.float32, ratio=3, alpha=1.0, gs=1.0, seed=0):
    """mask bool[B,A]: the positives; key f32[B,A]: the background CE of every candidate row, 0 or >= 1024 (ignored at
    positives, whose own background logit is a fill value: a large key that must not take part in the mining).
    Returns inputs (CPU torch) and the expected out8 / dconf / dloc / selection, with the regime asserted."""
    n = B * A
    rng = np.random.default_rng(2000 + seed)
    mask = np.asarray(mask, dtype=bool).reshape(n)
    key = np.where(mask, 0, np.asarray(key, dtype=np.float32).reshape(n)).astype(np.float32)
    pos_ce = np.where(mask, rng.choice(np.array([0.0, 1024.0, 1536.0, 2048.0], dtype=np.float32), n), 0).astype(np.float32)
    chosen = np.where(mask, pos_ce, key)
    assert ((chosen == 0) | (chosen >= 1024)).all()
    label = rng.integers(0, C - 1, n)
    assert C > 2
    other = (label + 1 + rng.integers(0, C - 2, n)) % (C - 1)           # a foreground class that is not the label
    fg = rng.integers(0, C - 1, n)
    assert (other != label).all() and (other < C - 1).all()
    top = np.where(mask, np.where(pos_ce == 0, label, other), np.where(key == 0, C - 1, fg))
    low = np.where(mask, label, C - 1)
    conf = rng.choice(np.array(strict.FILL, dtype=np.float32), (n, C))
    rows = np.arange(n)
    has_low = chosen != 0
    conf[rows[has_low], low[has_low]] = -chosen[has_low]                  # m = 0 on these rows: m - v = -v is the key's own bits
    m = np.where(has_low, 0.0, rng.choice(np.array([0.0, 4.0, -4.0]), n)).astype(np.float32)
    conf[rows, top] = m
    d = rng.integers(-12, 13, (n, 4)).astype(np.float32) / 4              # differences on both sides of |d| = 1, and exact zeros
    gt_loc = rng.integers(-8, 9, (n, 4)).astype(np.float32) / 4
    loc = gt_loc + d
    gt_loc[~mask] = 12345.0                                               # never read
    gt_cls = np.where(mask, label, rng.integers(0, C, n)).astype(np.int32)
    r = dict(B=B, A=A, C=C, dtype=dtype, ratio=ratio, alpha=float(alpha), grad_scale=float(gs), key=key.reshape(B, A),
             conf=torch.from_numpy(conf).view(B, A, C).to(dtype), loc=torch.from_numpy(loc).view(B, A, 4).to(dtype),
             gt_cls=torch.from_numpy(gt_cls).view(B, A), gt_loc=torch.from_numpy(gt_loc).view(B, A, 4),
             gt_mask=torch.from_numpy(mask.astype(np.uint8)).view(B, A))
    assert torch.equal(r["conf"].float(), torch.from_numpy(conf).view(B, A, C)), "a logit does not survive the cast"
    assert torch.equal(r["loc"].float(), torch.from_numpy(loc).view(B, A, 4)), "an offset does not survive the cast"
    ref = oracle_of(r, ratio, alpha, gs)
    # the regime, on the inputs and the float64 reference
    mb = mask.reshape(B, A)
    assert np.array_equal(ref["key"][~mb], key.reshape(B, A)[~mb].astype(np.float64)), "the keys are the chosen numbers"
    assert (ref["key"][mb] >= 1024).all(), "a positive's own key is large: it must be excluded, not out-ranked"
    P, N = ref["num_pos"], ref["num_neg"]
    out8 = np.zeros(8, dtype=np.float32)
    out8[4], out8[5] = P, N
    if P == 0:
        out8[7] = 1.0
        dconf, dloc = np.zeros((B, A, C)), np.zeros((B, A, 4))
    else:
        assert _pow2(P) and _pow2(alpha) and _pow2(gs)
        assert strict.sums_exactly(key.reshape(B, A)[ref["neg_mask"]]) and strict.sums_exactly(pos_ce[mask])
        assert strict.sums_exactly(M.smooth_l1(d.astype(np.float64))[mask].reshape(-1))
        out8[0], out8[1], out8[2] = np.float32(ref["loc"]), np.float32(ref["pos"]), np.float32(ref["neg"])
        out8[3] = (out8[0] + out8[1]) + out8[2]
        mined = ~np.isnan(ref["tau"])
        out8[6] = np.float32(ref["tau"][mined].min()) if mined.any() else 0.0
        dconf, dloc = ref["dcls"] + 0.0, ref["dbox"] + 0.0                # (+ 0.0: no negative zeros)
        assert set(np.unique(np.abs(dconf))) <= {0.0, gs / P}
    for name, v in (("dconf", dconf), ("dloc", dloc)):
        t = torch.from_numpy(v)
        assert torch.equal(t.to(dtype).double(), t), name + " converts without rounding"
        r[name] = t.to(dtype)
    r.update(out8=torch.from_numpy(out8), status=int(out8[7]), P=P, N=N, ref=ref, selected=(mb | ref["neg_mask"]).reshape(n),
             N_b=ref["neg_mask"].sum(1), tau=ref["tau"])
    return r


def place(keys, mask_row, at, value, seed):
    """a full row of keys [A]: `keys` (the candidates' keys, any order) scattered over the non-positive anchors in a seeded order,
    then swapped so that the anchors `at` hold the keys equal to `value` (a tie group at chosen places)"""
    rng = np.random.default_rng(seed)
    A = mask_row.size
    row = np.zeros(A, dtype=np.float32)
    cand = np.flatnonzero(~mask_row)
    row[cand] = rng.permutation(np.asarray(keys, dtype=np.float32))
    at = np.asarray(at, dtype=np.int64)
    if at.size:
        assert not mask_row[at].any()
        have = np.flatnonzero((row == np.float32(value)) & ~mask_row)
        assert have.size == at.size, (have.size, at.size)
        move_from = np.setdiff1d(have, at)
        move_to = np.setdiff1d(at, have)
        row[move_from], row[move_to] = row[move_to].copy(), row[move_from].copy()
    return row


def _mask_rows(B, A, P_b, seed, avoid=()):
    rng = np.random.default_rng(seed)
    mask = np.zeros((B, A), dtype=bool)
    free = np.setdiff1d(np.arange(A), np.asarray(avoid, dtype=np.int64))
    for b, p in enumerate(P_b):
        mask[b, rng.choice(free, p, replace=False)] = True
    return mask


def ranks_case(dtype=torch.float32):
    """B = 5, A = 300: tau_b first / middle / last member of its tie group; tau_0 and tau_2 differ in their low 10 bits only,
    tau_1 from them in the middle digit, tau_3 in the high digit; image 4 has no positive.  P = 32."""
    k3, k2 = strict.level3_keys(), strict.level2_keys()
    kh = strict.f32_bits(0x47000400 + np.arange(1024))
    B, A, P_b = 5, 300, (16, 8, 4, 4, 0)
    mask = _mask_rows(B, A, P_b, 31)
    per = [image_keys(A, 16, 3, k3[500:], k3[499], 5, 1, k3[400:499], 1),
           image_keys(A, 8, 3, k2[901:], k2[900], 5, 3, k2[800:900], 2),
           image_keys(A, 4, 3, k3[701:], k3[700], 5, 5, k3[600:700], 3),
           image_keys(A, 4, 3, kh[301:], kh[300], 2, 2, kh[200:300], 4),
           strict._fill_keys(A, 5)]
    key = np.stack([place(per[b], mask[b], (), 0, 40 + b) for b in range(B)])
    r = exact_case(B, A, 21, mask, key, dtype, seed=1)
    assert list(r["N_b"]) == [52, 26, 12, 12, 0]
    bits = [int(np.float32(t).view(np.uint32)) for t in r["tau"][:4]]
    assert bits[0] >> 10 == bits[2] >> 10 and bits[0] != bits[2]
    assert bits[0] >> 21 == bits[1] >> 21 and bits[0] >> 10 != bits[1] >> 10 and bits[3] >> 21 != bits[0] >> 21
    return r


def boundary_case(dtype, C=81, ratio=3, alpha=1.0, gs=1.0):
    """B = 2, A = 200 (128-row blocks straddle the images): each image's tie group sits on consecutive anchors across a block
    boundary (rows 125..130, and rows 253..258 = anchors 53..58 of image 1).  bf16-representable keys.  P = 8."""
    B, A, P_b = 2, 200, (4, 4)
    ks = strict.bf16_keys(64)
    at = (np.arange(125, 131), np.arange(53, 59))
    mask = np.stack([_mask_rows(1, A, (4,), 50 + b, at[b])[0] for b in range(B)])
    key = np.stack([place(image_keys(A, 4, ratio, ks[9:], ks[8], 6, 2 + 3 * b, ks[:8], 6 + b, dtype), mask[b], at[b], ks[8], 60 + b)
                    for b in range(B)])
    return exact_case(B, A, C, mask, key, dtype, ratio, alpha, gs, seed=2)


def saturated_case(dtype):
    """B = 2, A = 300: image 0 has 128 positives, 3 * 128 > 172 candidates: every candidate is mined and tau_0 is the smallest
    candidate key, an exact 0 -- legal here; image 1 has none.  P = 128."""
    B, A = 2, 300
    mask = _mask_rows(B, A, (128, 0), 70)
    key = np.stack([place(strict._fill_keys(172, 8, dtype), mask[0], (), 0, 71), strict._fill_keys(A, 9, dtype)])
    r = exact_case(B, A, 21, mask, key, dtype, gs=4.0, alpha=0.5, seed=3)
    assert list(r["N_b"]) == [172, 0] and r["tau"][0] == 0.0 and (key[0][~mask[0]] == 0).any()
    return r


def empty_case(dtype):
    """no positive anywhere: status 1, zeros"""
    B, A = 2, 150
    return exact_case(B, A, 21, np.zeros((B, A), dtype=bool), strict._fill_keys(B * A, 10, dtype).reshape(B, A), dtype, seed=4)


def heads_case(B, geom, C, P_b, full=(), empty=(), ratio=3, gs=1.0, alpha=1.0, seed=0):
    """bf16, exact: image b has P_b[b] positives and (ratio + 1) * P_b[b] selected anchors at chosen places -- one per pixel of
    every level in `full`, none in the levels of `empty`, the rest seeded -- its mined keys distinct above 1536, every other key
    below.  Adds the compact-row expectation (strict.heads_expected) under "levels"."""
    A = strict.anchors_of(geom)
    rng = np.random.default_rng(500 + seed)
    mask = np.zeros((B, A), dtype=bool)
    key = np.zeros((B, A), dtype=np.float32)
    for b in range(B):
        if P_b[b] == 0:
            key[b] = strict._fill_keys(A, seed + b, torch.bfloat16)
            continue
        nsel = (ratio + 1) * P_b[b]
        allowed = np.ones(A, dtype=bool)
        chosen = np.zeros(A, dtype=bool)
        off = 0
        for l, (h, w, k) in enumerate(geom):
            if l in empty:
                allowed[off:off + h * w * k] = False
            if l in full:
                chosen[off + np.arange(h * w) * k + rng.integers(0, k, h * w)] = True
            elif l not in empty:
                chosen[off + rng.integers(0, h * w * k)] = True
            off += h * w * k
        need = nsel - int(chosen.sum())
        free = np.flatnonzero(allowed & ~chosen)
        assert 0 <= need <= free.size, (need, free.size)
        chosen[rng.choice(free, need, replace=False)] = True
        sel = rng.permutation(np.flatnonzero(chosen))
        mask[b, sel[:P_b[b]]] = True
        key[b, sel[P_b[b]:]] = strict.bf16_keys(nsel - P_b[b])
        rest = np.flatnonzero(~chosen)
        key[b, rest] = strict._fill_keys(rest.size, seed + b, torch.bfloat16)
    r = exact_case(B, A, C, mask, key, torch.bfloat16, ratio, alpha, gs, seed=10 + seed)
    assert list(r["N_b"]) == [ratio * p for p in P_b]
    r["geom"] = geom
    r["npad"] = tuple((k * (4 + C) + 7) // 8 * 8 + (8 if l % 2 else 0) for l, (_, _, k) in enumerate(geom))
    r["levels"] = strict.heads_expected(r, geom, r["npad"])
    for l in full:
        assert r["levels"][l]["count"] == sum(1 for p in P_b if p) * r["levels"][l]["hw"]
    for l in empty:
        assert r["levels"][l]["count"] == 0
    return r


HEADS_CASES = {}
for _B, _P1, _P7, _P8 in ((1, (16,), (8,), (128,)), (3, (16, 0, 16), (8, 0, 8), (128, 0, 128))):
    for _C in (21, 81):
        HEADS_CASES["GEOM1 B=%d C=%d" % (_B, _C)] = lambda B=_B, C=_C, P=_P1: heads_case(B, strict.GEOM1, C, P, full=(0,), seed=B + C)
        HEADS_CASES["GEOM7 B=%d C=%d" % (_B, _C)] = lambda B=_B, C=_C, P=_P7: heads_case(B, strict.GEOM7, C, P, full=(3,), empty=(1,), gs=0.5, seed=B + C)
        HEADS_CASES["GEOM8 B=%d C=%d" % (_B, _C)] = lambda B=_B, C=_C, P=_P8: heads_case(B, strict.GEOM8, C, P, full=(0,), empty=(5,), gs=4.0, alpha=0.5, seed=B + C)
HEADS_CASES["SSD300 B=2 C=81"] = lambda: heads_case(2, SSD300_GEOM, 81, (64, 64), full=(5,), empty=(4,), seed=7)

_CACHE = {}


def cached(name, build):
    """a case built once per process and never modified"""
    if name not in _CACHE:
        _CACHE[name] = build()
    return _CACHE[name]
