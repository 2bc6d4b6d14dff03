"""CPU suite: convolution dispatch coverage.  The library's dispatch queries (ssd_conv2d_*_plan, include/ssd_hip.h) are
host functions -- the dispatch code with launching switched off -- so which kernel serves which layer can be checked
without a GPU:
  * every (forward, data-gradient, weight-gradient) kernel the batch-64 SSD300 train step launches is reached by at
    least one oracle-compared case of tests/test_conv_gpu.py (tests/conv_cases.py), so no kernel of the benchmarked
    step runs unchecked;
  * every (pass, kernel, kernel size, stride) the ResNet-50 SSD512 trunk's convolutions run at input 512 and 256, batch 1
    to 32, is reached by a case of the strict and the oracle-compared tests (RESNET_CASES were written from this walk);
  * every case still names the kernels it was written for (the GPU tests assert the same before computing)."""
import pytest

from tests.conv_cases import CASES, FIRST_LAYER_CASE, FULL_SIZE_CASES, RESNET_CASES, WS_BYTES, _geom, plan_name, plan_names


def _network_plans(B):
    from ssd_object_detection_amd import _lib
    from ssd_object_detection_amd.engine import SSD300_TRUNK, SSD300_NUM_PRIORS
    L = _lib.lib()
    out, s, fms = [], 300, []
    for i, (kind, cin, cout, k, stride, mode, feat) in enumerate(SSD300_TRUNK):
        ho, _, pt, _ = _geom(s, s, k, stride, mode)
        if kind == "conv":
            pooled = i + 1 < len(SSD300_TRUNK) and SSD300_TRUNK[i + 1][0] == "pool"
            out.append(("conv%d fwd" % i, L.ssd_conv2d_fwd_plan(B, s, s, cin, cout, k, stride, pt, pt, ho, ho, 2 if pooled else 0, WS_BYTES)))
            if i > 0:
                out.append(("conv%d dgrad" % i, L.ssd_conv2d_bwd_data_plan(B, s, s, cin, cout, k, stride, pt, pt, ho, ho, 0, WS_BYTES)))
            out.append(("conv%d wgrad" % i, L.ssd_conv2d_bwd_weight_plan(B, s, s, cin, cout, cout, k, stride, pt, pt, ho, ho)))
        s = ho
        if feat:
            fms.append((ho, cout))
    for lvl, ((h, c), n) in enumerate(zip(fms, SSD300_NUM_PRIORS)):
        nout, npad = n * 85, (n * 85 + 7) // 8 * 8
        out.append(("head%d fwd" % lvl, L.ssd_conv2d_head_fwd_plan(B, h, h, c, n, 81, WS_BYTES)))
        out.append(("head%d dgrad" % lvl, L.ssd_conv2d_bwd_data_plan(B, h, h, c, npad, 3, 1, 1, 1, h, h, 0, WS_BYTES)))
        out.append(("head%d wgrad" % lvl, L.ssd_conv2d_bwd_weight_plan(B, h, h, c, nout, npad, 3, 1, 1, 1, h, h)))
    return L, out


def test_cases_name_the_kernels_they_reach():
    for case in CASES + FULL_SIZE_CASES + RESNET_CASES + [FIRST_LAYER_CASE]:
        assert plan_names(case[:8]) == case[8], case[:8]


def _resnet_plans(in_size, B):
    """(node, pass, kernel name, (kernel size, stride)) of every convolution of the ResNet-50 SSD512 trunk as
    ResNet50SSDEngine calls the library: forward and weight gradient of each, the data gradient of each but the stem,
    accumulating where a later node (processed earlier by backward) has already written the same map's gradient."""
    from ssd_object_detection_amd import _lib
    from ssd_object_detection_amd.resnet_engine import resnet50_ssd512_graph
    L, g = _lib.lib(), resnet50_ssd512_graph()
    size, out = {-1: in_size}, []
    for i, nd in enumerate(g):
        src = nd["src"][0] if nd["op"] == "add" else nd["src"]
        h = size[src]
        if nd["op"] not in ("conv", "pool3"):
            size[i] = h
            continue
        ho, _, pt, _ = _geom(h, h, nd["k"], nd["stride"], "same")
        size[i] = ho
        if nd["op"] != "conv":
            continue
        cin, cout, k, s = nd["cin"], nd["cout"], nd["k"], nd["stride"]
        assert cout % 8 == 0
        out.append((i, 0, plan_name(L, L.ssd_conv2d_fwd_plan(B, h, h, cin, cout, k, s, pt, pt, ho, ho, 0, WS_BYTES)), (k, s)))
        if src >= 0:
            acc = any(j > i and (src in n["src"] if n["op"] == "add" else n["src"] == src) for j, n in enumerate(g))
            out.append((i, 1, plan_name(L, L.ssd_conv2d_bwd_data_plan(B, h, h, cin, cout, k, s, pt, pt, ho, ho, int(acc), WS_BYTES)), (k, s)))
        out.append((i, 2, plan_name(L, L.ssd_conv2d_bwd_weight_plan(B, h, h, cin, cout, cout, k, s, pt, pt, ho, ho)), (k, s)))
    return out


@pytest.mark.parametrize("in_size", [512, 256])
def test_every_kernel_of_the_resnet_trunk_has_a_strict_case(in_size):
    """Every (pass, kernel name with its flags) the trunk's convolutions resolve to at batch 1 .. 32 is named, for the same
    pass, with the same flags and at the same kernel size and stride, by a case that tests/test_conv_strict_gpu.py and
    tests/test_conv_gpu.py run.  A dispatch change that sends a ResNet layer to a kernel (or a mode of one) no case reaches
    fails here, on the CPU.  (Kernel size and stride belong to the key: the parity-class data gradient was right at 3x3 and
    1x1 and wrong at 7x7.)"""
    tested = [set(), set(), set()]
    for case in CASES + FULL_SIZE_CASES + RESNET_CASES:
        for p in range(3):
            tested[p].add((case[8][p], case[5], case[6]))
    nconv = 0
    for B in (1, 2, 4, 8, 16, 32):
        plans = _resnet_plans(in_size, B)
        nconv = len({i for i, _, _, _ in plans})
        for i, p, name, ks in plans:
            assert not name.startswith("error"), (i, B, name)
            assert (name,) + ks in tested[p], "node %d at input %d, batch %d: the %s runs %s at k = %d, stride %d, which no case names" % (
                (i, in_size, B, ("forward", "data gradient", "weight gradient")[p], name) + ks)
    assert nconv == 53                                       # the stem, 39 bottleneck convolutions, 3 projections, 10 extras


@pytest.mark.parametrize("B", [64, 32, 4])
def test_every_kernel_of_the_train_step_has_an_oracle_case(B):
    L, plans = _network_plans(B)
    assert all(p > 0 for _, p in plans), [n for n, p in plans if p <= 0]
    fused_pool = 0x800                                        # tests/test_conv_gpu.py::test_conv_fwd_pool_fused covers the flag
    tested = set()
    for case in CASES + FULL_SIZE_CASES:
        tested.update(case[8])
    tested.update((FIRST_LAYER_CASE[8][0], FIRST_LAYER_CASE[8][2]))
    for name, plan in plans:
        kernel = plan_name(L, plan & ~fused_pool)
        base = kernel.split("+")[0]
        flags = set(kernel.split("+")[1:])
        hit = [t for t in tested if t.split("+")[0] == base and flags <= set(t.split("+")[1:])]
        assert hit, "%s at batch %d runs %s, which no oracle-compared case reaches" % (name, B, kernel)
