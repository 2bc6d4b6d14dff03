"""Execution engine of the SSD300 network on the gfx950 library: parameter storage, forward, backward and
the optimizer step.  Python only sequences C-ABI calls (ops.py / _lib.py); every tensor operation runs in
libssd_hip.so.  torch provides device memory, streams and (for data parallelism) torch.distributed.

Network = SSDObjectDetectionModel._build of the reference (models/ssd_model.py:74-171): Keras VGG16 up to
block3_conv3, a SAME max-pool, three 38x38 convolutions, five extra stages, and per-level 3x3 loc/conf heads.
Activations are NHWC bf16, weights [Cout][k][k][Cin] bf16 (fp32 masters), accumulation fp32 on MFMA.
The 3-channel image is carried in 8 zero-padded channels (first-layer weights of channels 3..7 are and stay 0).
The same engine runs the SSD paper's VGG-16 SSD300 (VGG16_SSD300_TRUNK below: no reference counterpart).
"""
import collections
import contextlib
import logging
import math
import os

import numpy as np
import torch

from . import _lib, mx, ops

logger = logging.getLogger(__name__)

# (kind, cin, cout, k, stride, mode, feature_map)   -- mode: TF padding; every conv has ReLU
SSD300_TRUNK = [
    ("conv", 8, 64, 3, 1, "same", False),        # block1_conv1   (Cin 3 padded to 8)
    ("conv", 64, 64, 3, 1, "same", False),       # block1_conv2
    ("pool", 64, 64, 2, 2, "valid", False),      # block1_pool 300 -> 150
    ("conv", 64, 128, 3, 1, "same", False),      # block2_conv1
    ("conv", 128, 128, 3, 1, "same", False),     # block2_conv2
    ("pool", 128, 128, 2, 2, "valid", False),    # block2_pool 150 -> 75
    ("conv", 128, 256, 3, 1, "same", False),     # block3_conv1
    ("conv", 256, 256, 3, 1, "same", False),     # block3_conv2
    ("conv", 256, 256, 3, 1, "same", False),     # block3_conv3                     models/ssd_model.py:77-82
    ("pool", 256, 256, 2, 2, "same", False),     # MaxPool2D SAME 75 -> 38           :84
    ("conv", 256, 512, 3, 1, "same", False),     # :86
    ("conv", 512, 512, 3, 1, "same", False),     # :90
    ("conv", 512, 512, 1, 1, "same", True),      # :94   -> feature map 0 (38x38x512)
    ("conv", 512, 1024, 3, 2, "same", False),    # :102
    ("conv", 1024, 1024, 1, 1, "same", True),    # :107  -> feature map 1 (19x19x1024)
    ("conv", 1024, 256, 1, 1, "same", False),    # :113
    ("conv", 256, 512, 3, 2, "same", True),      # :117  -> feature map 2 (10x10x512)
    ("conv", 512, 128, 1, 1, "same", False),     # :124
    ("conv", 128, 256, 3, 2, "same", True),      # :128  -> feature map 3 (5x5x256)
    ("conv", 256, 128, 1, 1, "same", False),     # :135
    ("conv", 128, 256, 3, 1, "valid", True),     # :139  -> feature map 4 (3x3x256)
    ("conv", 256, 128, 1, 1, "same", False),     # :144
    ("conv", 128, 256, 3, 1, "valid", True),     # :148  -> feature map 5 (1x1x256)
]
SSD300_NUM_PRIORS = (4, 6, 6, 6, 4, 4)           # models/ssd_model.py:153
IMAGE_CHANNELS = 3

# BASELINE.json configs[4] stress geometry (no reference counterpart: the reference hard-codes 300 / 8732): the same
# network recipe at 512 x 512 with one more stride-2 stage, 7 feature levels 64, 32, 16, 8, 4, 2, 1 and 4, 6, 6, 6, 6, 4, 4
# default boxes per cell = 24 564 anchors.  (VGG-style trunk in bf16 -- not the ResNet-50 / fp8 of that config's title.)
SSD512_TRUNK = SSD300_TRUNK[:13] + [
    ("conv", 512, 1024, 3, 2, "same", False),    # 64 -> 32
    ("conv", 1024, 1024, 1, 1, "same", True),    # feature map 1 (32x32x1024)
    ("conv", 1024, 256, 1, 1, "same", False),
    ("conv", 256, 512, 3, 2, "same", True),      # feature map 2 (16x16x512)
    ("conv", 512, 128, 1, 1, "same", False),
    ("conv", 128, 256, 3, 2, "same", True),      # feature map 3 (8x8x256)
    ("conv", 256, 128, 1, 1, "same", False),
    ("conv", 128, 256, 3, 2, "same", True),      # feature map 4 (4x4x256)
    ("conv", 256, 128, 1, 1, "same", False),
    ("conv", 128, 256, 3, 2, "same", True),      # feature map 5 (2x2x256)
    ("conv", 256, 128, 1, 1, "same", False),
    ("conv", 128, 256, 3, 2, "same", True),      # feature map 6 (1x1x256)
]
SSD512_NUM_PRIORS = (4, 6, 6, 6, 6, 4, 4)

# The SSD paper's own 300 x 300 network (Liu et al. 2016, section 3.1 / Caffe SSD's VGG_VOC0712_SSD_300): VGG-16 through
# conv5_3, pool5 as 3x3 / stride 1, fc6 as a 3x3 convolution with dilation 6, fc7 as a 1x1, then the extras above.  Feature
# maps conv4_3 (38x38x512, the one the paper L2-normalises), fc7 (19x19x1024), conv8_2 .. conv11_2: grids 38, 19, 10, 5, 3, 1
# and 4, 6, 6, 6, 4, 4 default boxes per cell = 8732 anchors.  Keras padding throughout (pool3 here is the SAME one of
# SSD300_TRUNK, 75 -> 38, where Caffe rounds up).  An eighth element is the dilation; "pool3s1" is the 3x3 / stride-1 SAME pooling.
VGG16_SSD300_TRUNK = SSD300_TRUNK[:10] + [
    ("conv", 256, 512, 3, 1, "same", False),     # conv4_1
    ("conv", 512, 512, 3, 1, "same", False),     # conv4_2
    ("conv", 512, 512, 3, 1, "same", True),      # conv4_3  -> feature map 0 (38x38x512); also pooled
    ("pool", 512, 512, 2, 2, "valid", False),    # pool4 38 -> 19
    ("conv", 512, 512, 3, 1, "same", False),     # conv5_1
    ("conv", 512, 512, 3, 1, "same", False),     # conv5_2
    ("conv", 512, 512, 3, 1, "same", False),     # conv5_3
    ("pool3s1", 512, 512, 3, 1, "same", False),  # pool5 19 -> 19
    ("conv", 512, 1024, 3, 1, "same", False, 6), # fc6, dilation 6
    ("conv", 1024, 1024, 1, 1, "same", True),    # fc7      -> feature map 1 (19x19x1024)
] + SSD300_TRUNK[15:]                            # conv8_1 .. conv11_2 -> feature maps 2 .. 5
VGG16_SSD300_NUM_PRIORS = (4, 6, 6, 6, 4, 4)


def _separable(c, cout, stride, feature=False):
    """A MobileNet block: depthwise 3x3 (kind "dwconv": kernel [3][3][C], bias [C], ReLU) and the 1x1 convolution behind it."""
    return [("dwconv", c, c, 3, stride, "same", False), ("conv", c, cout, 1, 1, "same", feature)]


# MobileNet-v1 SSD300 (Howard et al. 2017, table 1, at width 1; no reference counterpart): the batch normalisations folded into
# the biases, plain ReLU, Keras SAME padding.  Feature maps: the last 19x19 block (node 22, 512 channels), the last 10x10 block
# (node 26, 1024 channels) and four extras pairs in "same" mode: grids 19, 10, 5, 3, 2, 1 and 4, 6, 6, 6, 4, 4 default boxes per
# cell = 2268 anchors.  The last extras pair is 128 / 256 wide (Caffe MobileNet-SSD: 64 / 128): the chain kernel and the sparse
# heads take multiples of 128.  The heads are the engine's ordinary 3x3 ones (SSDLite's separable heads: not planned).
MOBILENET_V1_SSD300_TRUNK = (
    [("conv", 8, 32, 3, 2, "same", False)]           # 300 -> 150 (Cin 3 padded to 8)
    + _separable(32, 64, 1)                          # 150
    + _separable(64, 128, 2) + _separable(128, 128, 1)       # 75
    + _separable(128, 256, 2) + _separable(256, 256, 1)      # 38
    + _separable(256, 512, 2) + 4 * _separable(512, 512, 1) + _separable(512, 512, 1, True)     # 19; node 22 -> feature map 0
    + _separable(512, 1024, 2) + _separable(1024, 1024, 1, True)                                # 10; node 26 -> feature map 1
    + [("conv", 1024, 256, 1, 1, "same", False), ("conv", 256, 512, 3, 2, "same", True),        # -> feature map 2 (5x5x512)
       ("conv", 512, 128, 1, 1, "same", False), ("conv", 128, 256, 3, 2, "same", True),         # -> feature map 3 (3x3x256)
       ("conv", 256, 128, 1, 1, "same", False), ("conv", 128, 256, 3, 2, "same", True),         # -> feature map 4 (2x2x256)
       ("conv", 256, 128, 1, 1, "same", False), ("conv", 128, 256, 3, 2, "same", True)])        # -> feature map 5 (1x1x256)
MOBILENET_V1_SSD300_NUM_PRIORS = (4, 6, 6, 6, 4, 4)
RELU_KINDS = ("conv", "dwconv")                  # node kinds with a ReLU of their own: it masks the data gradient of the node behind


def mxfp8_eligible(nd):
    """Whether the block-scaled fp8 kernels serve node `nd` (ops.conv2d_fwd_mxfp8; a planned node or a graph node of
    resnet_engine): a convolution whose input channels are whole MX k-steps (Cin % 128 == 0) and whose output channels are
    whole MX blocks (Cout % 32 == 0); a dilated one (a planned node's "dilation"; graph nodes carry no such key) only at
    3x3 / stride 1 (ops.conv2d_atrous_fwd_mxfp8)."""
    if nd.get("dilation", 1) != 1 and (nd["k"], nd["stride"]) != (3, 1):
        return False
    return (nd.get("kind", nd.get("op")) == "conv" and nd["cin"] % 128 == 0 and nd["cout"] % 32 == 0 and nd["k"] in (1, 3)
            and nd["stride"] in (1, 2))


MxTrunkPlan = collections.namedtuple("MxTrunkPlan", "fp8 pooled qpool quant writes")


def mxfp8_trunk_plan(nodes, chain_start):
    """The inference fp8 forward of an SSDEngine trunk (its planned nodes: node i reads node i - 1; no device needed).
    Returns MxTrunkPlan(fp8, pooled, qpool, quant, writes):
      fp8     the convolutions that run on block-scaled fp8 operands: one run of them up to the chain (which stays bf16),
              each fed by the epilogue of the layer in front of it;
      pooled  the pools that run inside the fp8 convolution in front of them (ops.conv2d_fwd_pool_mxfp8: 3x3 / stride 1,
              never a feature map: its head reads the full-resolution map, which that launch does not store);
      qpool   the other pools of the run: each launches as a quantising pooling (ops.maxpool2x2_fwd_mxfp8 /
              ops.maxpool3x3s1_fwd_mxfp8) that reads the bf16 map in front of it and stores the pooled map in fp8 -- every
              3x3 / stride-1 pooling, and a 2x2 one whose convolution is a feature map or otherwise does not pool itself;
      quant   the ONE node whose bf16 output gets a standalone ops.quantize_mx_fp8: the input of the run's first layer;
      writes  {node: frozenset of "bf16" / "fp8"}, the forms of its output the walk stores -- exactly what its consumers read
              (the heads and the quantising poolings read bf16), the quantised node's bf16 map besides, nothing for a
              convolution whose pool runs in its own launch.
    The run is the longest stretch of such layers that ends in front of the chain.  It starts at its first convolution
    whose input map is smaller than the map the layer writes: the standalone quantise then costs less than the layer's
    own store (SSD300: block3_conv1 on the 75x75x128 pooled map, not block2_conv2 on the 150x150x128 one)."""
    n = len(nodes)
    end = n if chain_start is None else chain_start
    pools = ("pool", "pool3s1")

    def pools_itself(i):                 # a 3x3 / stride-1 fp8 convolution with a 2x2 pool behind it inside the run
        nd = nodes[i]
        return (mxfp8_eligible(nd) and nd["k"] == 3 and nd["stride"] == 1 and nd.get("dilation", 1) == 1 and not nd["feature"]
                and i + 1 < end and nodes[i + 1]["kind"] == "pool")

    s = end
    while s > 1 and (mxfp8_eligible(nodes[s - 1]) or (nodes[s - 1]["kind"] in pools and mxfp8_eligible(nodes[s - 2]))):
        s -= 1
    size = [nd["hout"] ** 2 * nd["cout"] for nd in nodes]
    start = None
    for i in range(s, end):
        out = size[i + 1] if pools_itself(i) else size[i]
        if nodes[i]["kind"] == "conv" and size[i - 1] < out:
            start = i
            break
    assert start is not None, "no layer of this trunk can run in fp8 behind a quantise cheaper than its own store"
    fp8 = {i for i in range(start, end) if nodes[i]["kind"] == "conv"}
    pooled = {i + 1 for i in fp8 if pools_itself(i)}
    qpool = {i for i in range(start, end) if nodes[i]["kind"] in pools and i not in pooled}
    quant = {start - 1}
    writes = {i: set() for i in range(n)}
    for i, nd in enumerate(nodes):
        if nd["feature"]:
            writes[i].add("bf16")
        if i > 0 and i not in pooled:
            writes[i - 1].add("fp8" if i in fp8 else "bf16")
    writes[start - 1].add("bf16")
    for i, w in writes.items():
        assert w or (i in fp8 and i + 1 in pooled), "node %d has no consumer" % i
        if "fp8" in w:                   # (a quantising pooling is its own quantiser)
            assert i in fp8 or i in pooled or i in qpool or i in quant, "node %d would need a standalone activation quantise" % i
    assert all(i - 1 in fp8 for i in pooled | qpool) and not any(nodes[i - 1]["feature"] for i in pooled)
    return MxTrunkPlan(fp8, pooled, qpool, quant, {i: frozenset(w) for i, w in writes.items()})


def mxfp8_vgg_plan(nodes, chain_start):
    """mxfp8_trunk_plan as the 4-tuple (fp8, pooled, quant, writes): the plan of a trunk without quantising poolings (the
    default SSD300 and its 512 form), where qpool is empty."""
    p = mxfp8_trunk_plan(nodes, chain_start)
    return p.fp8, p.pooled, p.quant, p.writes


class ParamTensor:
    """One trainable variable of the reference (= one tf.clip_by_norm unit, models/ssd_model.py:249): `numel` elements at
    `offset` of the flat buffers, alone in optimizer blocks block0 .. block0 + nblocks - 1 (the rest of them is zero)."""

    def __init__(self, name, shape, offset, index, block0, nblocks):
        self.name, self.shape, self.offset, self.index = name, tuple(shape), offset, index
        self.numel = int(np.prod(shape))
        self.block0, self.nblocks = block0, nblocks


class FusedView:
    """Two adjacent ParamTensors read as one array: the loc and conf filters of a level are separate Keras layers
    (models/ssd_model.py:155-162: separate variables, separate clip norms) but one GEMM here.  The first part ends on a
    block boundary and the second starts on it, so the pair is contiguous without sharing an optimizer block."""

    def __init__(self, name, shape, parts):
        self.name, self.shape, self.parts = name, tuple(shape), tuple(parts)
        self.offset, self.index = parts[0].offset, parts[0].index
        self.numel = int(np.prod(shape))
        assert parts[1].offset == parts[0].offset + parts[0].numel and self.numel == parts[0].numel + parts[1].numel
        self.indices = [p.index for p in parts]


def _launched(fn, *args, refused=NotImplementedError, **kw):
    """Try a fused launch: whether it ran.  The library refuses a shape it has no kernel for before it launches anything
    (SSD_ERR_UNSUPPORTED -> NotImplementedError, SSD_ERR_VALUE -> ValueError): the caller takes the fallback and writes the
    answer where it keeps what it learned, so that it does not ask again."""
    try:
        fn(*args, **kw)
        return True
    except refused:
        return False


class _Streams:
    """The streams of the schedule beside the caller's, each created at its first use with the MatchWorkspace of the launches
    that go to it, and the two operations the schedule is made of."""

    def __init__(self, device):
        self.device = device
        self.side = self.ws_side = self.tail = self.ws_tail = None

    def side_stream(self):
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.device, priority=int(os.environ.get("SSD_SIDE_PRIO", "0")))
            self.ws_side = ops.MatchWorkspace()
        return self.side

    def tail_stream(self):
        if self.tail is None:
            self.tail = torch.cuda.Stream(device=self.device)
            self.ws_tail = ops.MatchWorkspace()
        return self.tail

    @staticmethod
    def behind(s, m):
        """`with behind(s, m):` runs the block on stream s, behind everything enqueued so far on stream m (one new event)."""
        ev = torch.cuda.Event()
        ev.record(m)
        s.wait_event(ev)
        return torch.cuda.stream(s)

    @staticmethod
    def after(s):
        """An event behind what stream s has enqueued."""
        ev = torch.cuda.Event()
        ev.record(s)
        return ev


class _BackwardPass:
    """One call of SSDEngine.backward: the state its phases share, and the phases (backward() is the order they run in)."""

    def __init__(self, eng, c, heads, dloc, dconf, on_ready, fused_adam, on_dgrad):
        self.eng, self.c, self.heads, self.dloc, self.dconf = eng, c, heads, dloc, dconf
        self.on_ready, self.hp, self.on_dgrad = on_ready, fused_adam, on_dgrad
        self.B = c["loc"].shape[0]
        self.big_levels = [lvl for lvl, (_, h, _) in enumerate(eng.fm) if self.B * h * h >= eng.BIG_LEVEL_PIXELS]
        self.acts, self.gacts = c["acts"], c["gacts"]
        self.written = [False] * len(self.acts)            # activation index -> its gradient holds a value to accumulate into
        self.main = torch.cuda.current_stream()
        self.side = eng._side_stream() if eng.overlap_heads else None
        self.pending = []                                  # (fn, tensors) waiting for the side stream's next wait
        self.opt_range, self.opt_at = None, {}             # the bucket update; node -> (t0, t1) of the bucket behind its data gradient
        self.deferred, self.defer_nodes = [], set()        # (t0, t1, event) of the buckets that run at the end of the main stream
        self.prefetch_done = None
        self.sparse_head_done = {}                         # activation index -> event after a large level's sparse data gradient
        self.head_done = {}                                # activation index -> event after a large level's dense data gradient
        self.l2n_done = []                                 # the event behind l2norm_bwd (kept only for on_ready's report)
        self.packed = [None] * len(eng.fm)                 # dense heads: loc + conf gradients per level
        self.unpooled = set()                              # pooling nodes whose backward pass ran inside the next convolution's data gradient
        self.chained, self.batched_w, self.first_fused = set(), set(), False

    # ---- phases, in order
    def plan_optimizer(self):
        e, hp = self.eng, self.hp
        if hp is None:
            return
        trunk_nodes = [node for _, _, node in e.opt_buckets() if node is not None]
        # the last bucket (lowest node) follows its own weight gradients on the side stream; the `opt_defer` before it go to the
        # END of the main stream, which finishes its chain ~0.3 ms before the side stream does
        if e.opt_defer > 0:
            self.defer_nodes = set(trunk_nodes[max(0, len(trunk_nodes) - 1 - e.opt_defer):len(trunk_nodes) - 1])
        e.step_count += 1
        t = e.step_count
        kind = hp.get("kind", "adam")
        if kind == "adam":
            lr_t = hp["lr"] * math.sqrt(1.0 - hp["beta2"] ** t) / (1.0 - hp["beta1"] ** t)
            self.opt_range = lambda t0, t1: e.adam_range(t0, t1, lr_t, hp["beta1"], hp["beta2"], hp["eps"], hp["clip"])
        elif kind == "sgd_momentum":
            self.opt_range = lambda t0, t1: e.sgd_range(t0, t1, hp["lr"], hp["momentum"], hp["nesterov"], hp["decay"], hp["clip"])
        else:
            raise ValueError("unknown fused optimizer kind %r" % (kind,))
        self.opt_at = {node: (t0, t1) for t0, t1, node in e.opt_buckets()}

    def prefetch_chain(self):
        e = self.eng
        if self.side is not None and e.chain_start is not None and "bwd" in e.chain and e.chain_prefetch:
            tail = e._streams.tail_stream()                # (whether or not `tail_stream` is set: that governs the forward heads)
            with _Streams.behind(tail, self.main):         # the data-gradient chain's packed filters into L2, ~50 us ahead of it
                ops.chain_prefetch([e.chain_pk_bwd[j] for j in range(e.chain_start, len(e.nodes))])
            self.prefetch_done = _Streams.after(tail)

    def heads_sparse(self):
        """All levels from the compact rows: data gradient on the main stream (every feature-map gradient is written before
        the trunk chain accumulates into it), weight gradient next to it on the side stream."""
        e, heads = self.eng, self.heads
        hl, keep = e._head_layers(self.c)                  # (keep: what the descriptors point to, alive until the calls are enqueued)
        self.on_side(lambda ws: ops.heads_bwd_weight_sparse(heads, hl, ws=e._ws_hw),
                     [i for wt, bt in e.head_params for t in (wt, bt) for i in t.indices])
        big_lv = self.big_levels
        small_lv = [lvl for lvl in range(len(e.fm)) if lvl not in big_lv]
        if self.side is not None and e.split_heads_dgrad and big_lv and small_lv:
            # the small maps' gradients head the extras' chain; the 38x38 / 19x19 maps' (most of the launch's time: their
            # dense maps are ~140 MB of stores) are not read until the chain reaches those maps -- third stream, the
            # chain's accumulation waits for its event (sparse_head_done)
            self.heads_dgrad_sparse(hl, small_lv)
            # split_heads_dgrad 2: one call per level, the level the chain reaches first (19x19) first: its event does not wait
            # for the 38x38 level's 94 MB of stores
            calls = [[lvl] for lvl in reversed(big_lv)] if e.split_heads_dgrad == 2 else [big_lv]
            tail = e._streams.tail_stream()
            with _Streams.behind(tail, self.main):
                for levels in calls:
                    self.heads_dgrad_sparse(hl, levels)    # (l2norm_bwd in front of the level's event: the trunk and the heads' optimizer wait for it)
                    done = _Streams.after(tail)
                    for lvl in levels:
                        self.sparse_head_done[e.fm[lvl][0] + 1] = done
        else:
            self.heads_dgrad_sparse(hl)
        for ni, _, _ in e.fm:
            self.written[ni + 1] = True

    def heads_dense(self):
        """From the dense (dloc, dconf): per level a packed gradient, a data gradient and a weight gradient on the dense kernels."""
        e = self.eng
        big = self.big_levels if self.side is not None and e.big_heads_side else []
        for lvl in range(len(e.fm)):                       # the large levels are packed where they are consumed (side stream)
            if lvl not in big or not e.pack_side:
                self.pack(lvl)
        if big:
            with _Streams.behind(self.side, self.main):
                for lvl in reversed(big):                  # 19x19 first: the trunk chain reaches it first
                    if e.pack_side:
                        self.pack(lvl)
                    self.head_dgrad(lvl, e._ws_side)
                    self.head_done[e.fm[lvl][0] + 1] = _Streams.after(self.side)
                for lvl in reversed(big):
                    self.head_wgrad(lvl, e._ws_side)
                    if self.on_ready:
                        self.on_ready([i for t in e.head_params[lvl] for i in t.indices])
        for lvl in range(len(e.fm)):
            if lvl not in big:
                self.on_side(lambda ws, lvl=lvl: self.head_wgrad(lvl, ws), [i for t in e.head_params[lvl] for i in t.indices])
                self.head_dgrad(lvl, e._ws)

    def report_l2norm(self):
        if self.l2n_done:
            # the scale's gradient is reported from the side stream like every weight gradient, behind the event of the stream
            # that ran l2norm_bwd: the reducer records ONE event, on the current stream, when a bucket completes
            self.on_side(lambda ws: torch.cuda.current_stream().wait_event(self.l2n_done[0]), [self.eng.l2norm_scale.index])

    def opt_bucket(self, node):
        """Called once the data gradient of `node` (None: of every head) is enqueued on the main stream."""
        if self.on_dgrad is not None:
            self.on_dgrad(node)
        if node not in self.opt_at:
            return
        t0, t1 = self.opt_at.pop(node)
        if self.side is not None and node in self.defer_nodes:
            self.flush_side()                             # the bucket's weight gradients are all enqueued there by now
            self.deferred.append((t0, t1, _Streams.after(self.side)))
            return
        # the heads' update rewrites head_w_t, which the large levels' sparse data gradients on the third stream still
        # read: behind their events as well as behind the main stream
        readers = list(self.sparse_head_done.values()) if node is None else []

        def run(ws):
            for ev in readers:
                torch.cuda.current_stream().wait_event(ev)
            self.opt_range(t0, t1)
        self.on_side(run, [])

    def chain_dgrads(self):
        """Data gradients of nodes end .. chain_start in one launch (ops.conv_chain): the head of the backward pass's critical
        path -- nothing large can start before this chain reaches the 19x19 map."""
        e, c, written = self.eng, self.c, self.written
        if e.chain_start is None or "bwd" not in e.chain:
            return
        last = len(e.nodes) - 1
        assert written[last + 1]
        layers = []
        for j in range(last, e.chain_start - 1, -1):
            ndj = e.nodes[j]
            use_bits = e.relu_bits is not None and j in e.bits_valid
            layers.append(ops.chain_layer_dgrad(e.w_t[j], e.chain_pk_bwd[j], self.gacts[j], ndj["stride"], ndj["pt"], ndj["pl"],
                                                accumulate=written[j], mask_bits=c["rbits"][j] if use_bits else None,
                                                mask_src=None if use_bits else self.acts[j]))
        for j in range(last, e.chain_start - 1, -1):
            self.wait_for_head(j)
        if _launched(ops.conv_chain, self.gacts[last + 1], layers):
            self.chained = set(range(e.chain_start, last + 1))
            for j in self.chained:
                written[j] = True
        else:
            e.chain = e.chain - {"bwd"}

    def chain_wgrads(self):
        """... and their weight gradients in two launches (slab kernel + slab sums) instead of twelve."""
        e = self.eng
        if not (self.chained and self.side is not None and e.batch_chain_wgrads and e.wgrad_probe is None):
            return
        order = sorted(self.chained, reverse=True)
        layers, tens = [], []
        for j in order:
            ndj = e.nodes[j]
            wt, bt = e.conv_params[j]
            layers.append((self.acts[j], self.gacts[j + 1], ndj["cout"], ndj["k"], ndj["stride"], ndj["pt"], ndj["pl"],
                           e.view(wt, e.grad), e.view(bt, e.grad)))
            tens += [wt.index, bt.index]
        if _launched(self.on_side, lambda ws: ops.conv2d_bwd_weight_batched(layers, ws=ws), tens):
            self.batched_w = set(order)
        else:
            e.batch_chain_wgrads = False

    def node(self, i):
        """Trunk node i: its weight gradient to the side stream, its data gradient (a pooling's backward pass) on the
        main stream, then the optimizer bucket that waited for that data gradient."""
        e, nd, written = self.eng, self.eng.nodes[i], self.written
        assert written[i + 1]
        if nd["kind"] == "pool3s1":
            assert not written[i], "the 3x3 / stride-1 un-pooling overwrites: its input cannot also feed a head"
            ops.maxpool3x3s1_bwd(self.c["pool_code"][i], self.gacts[i + 1], self.acts[i].shape, out=self.gacts[i])
            written[i] = True
            return
        if nd["kind"] == "pool":
            if written[i]:
                # the pooled activation feeds a head as well (conv4_3 of the VGG-16 SSD300): the head's gradient is in
                # gacts[i], possibly written on another stream; the un-pooling adds to it (dgrad() declined to un-pool
                # in the convolution's store stage, which overwrites)
                assert i not in self.unpooled
                self.wait_for_head(i)
                ops.maxpool2x2_bwd_argmax(self.c["pool_code"][i], self.gacts[i + 1], self.acts[i].shape, out=self.gacts[i],
                                          accumulate=True)
            elif i not in self.unpooled:                   # (else the convolution behind the pooling already wrote gacts[i])
                ops.maxpool2x2_bwd_argmax(self.c["pool_code"][i], self.gacts[i + 1], self.acts[i].shape, out=self.gacts[i])
            written[i] = True
            return
        wt, bt = e.conv_params[i]
        if nd["kind"] == "dwconv":
            self.on_side(lambda ws: self.dw_wgrad(i, ws), [wt.index, bt.index], grouped=True)
            self.dw_dgrad(i)
            self.opt_bucket(i)
            return
        if i == 0 and self.first_fused:                    # its weight gradient came out of the second layer's data-gradient kernel
            self.on_side(lambda ws: None, [wt.index, bt.index], grouped=True)
        elif i not in self.batched_w:                      # (else its weight gradient left with the batched launch)
            self.on_side(lambda ws: self.wgrad(i, ws), [wt.index, bt.index], grouped=True)
        if i > 0 and i not in self.chained:                # (no gradient w.r.t. the image / its data gradient came out of the chain launch)
            self.dgrad(i)
        self.opt_bucket(i)

    def finish(self):
        assert not self.opt_at
        self.flush_side()
        if self.prefetch_done is not None:
            self.main.wait_event(self.prefetch_done)       # (joins the third stream even where nothing else ran on it)
        for ev in self.sparse_head_done.values():          # (a large level whose map no trunk node accumulated into)
            self.main.wait_event(ev)
        for t0, t1, ev in self.deferred:
            self.main.wait_event(ev)
            self.opt_range(t0, t1)
        if self.side is not None:
            self.main.wait_stream(self.side)

    # ---- the side stream's queue: weight-gradient launches, the report behind each (on_ready) and the optimizer
    def on_side(self, fn, tensors, grouped=False):
        """Run fn(ws) on the side stream, after everything enqueued so far on the main stream, and report `tensors` from there
        (in place where there is no side stream).  grouped: it may wait for the next flush_side()."""
        if self.side is None:
            self._run(fn, tensors, self.eng._ws)
        elif grouped and self.eng.wgrad_group > 1:
            # the side stream is hundreds of microseconds behind the main stream for most of the backward pass, yet every
            # cross-stream wait costs it ~6 us of idle time (30 of them per step).  `wgrad_group` launches share ONE wait -- on the
            # event of the LAST of them, which a stream that is behind anyway has long passed
            self.pending.append((fn, tensors))
            if len(self.pending) >= self.eng.wgrad_group:
                self.flush_side()
        else:
            self.flush_side()
            with _Streams.behind(self.side, self.main):
                self._run(fn, tensors, self.eng._ws_side)

    def flush_side(self):
        """Precedes every direct run on the side stream and every event recorded there."""
        if self.pending:
            with _Streams.behind(self.side, self.main):
                for fn, tensors in self.pending:
                    self._run(fn, tensors, self.eng._ws_side)
            self.pending.clear()

    def _run(self, fn, tensors, ws):
        fn(ws)
        if self.on_ready:
            self.on_ready(tensors)                         # inside the stream context of the launch: the reducer records its event there

    # ---- launches the phases share
    def wait_for_head(self, a):
        """A large head wrote the gradient of activation a on another stream: the main stream accumulates after it."""
        for done in (self.head_done, self.sparse_head_done):
            if a in done:
                self.main.wait_event(done.pop(a))

    def l2norm_bwd(self):
        """Right behind head 0's data gradient, on its stream: that gradient (w.r.t. the normalised map) becomes gacts of
        feature map 0 -- written, the trunk accumulates into it afterwards as before -- and the scale's gradient."""
        e, c = self.eng, self.c
        a0, sc = e.fm[0][0] + 1, e.l2norm_scale
        ops.l2norm_bwd(c["l2n_gy"], self.acts[a0], e.view(sc, e.param), rnorm=c["l2n_r"], out=self.gacts[a0],
                       dscale=e.view(sc, e.grad), ws=e._ws_l2n, eps=e.l2norm.eps)
        if self.on_ready:
            self.l2n_done.append(_Streams.after(torch.cuda.current_stream()))

    def heads_dgrad_sparse(self, hl, levels=None):
        e = self.eng
        ops.heads_bwd_data_sparse(self.heads, hl, ws=e._ws_hz, levels=levels)
        if e.l2norm is not None and (levels is None or 0 in levels):
            self.l2norm_bwd()

    def pack(self, lvl):                                   # loc + conf gradients of one level in the head's channel order
        e, h = self.eng, self.eng.fm[lvl][1]
        self.packed[lvl] = ops.head_grad_pack(self.dloc, self.dconf, h * h, e.num_priors[lvl], e.classes, e.head_npad[lvl],
                                              e.level_off[lvl], out=self.c["packed"][lvl]).view(self.B, h, h, e.head_npad[lvl])

    def head_dgrad(self, lvl, ws):
        e = self.eng
        ni = e.fm[lvl][0]
        normed = lvl == 0 and e.l2norm is not None
        self.masked_dgrad("head%d" % lvl, self.packed[lvl], e.head_w_t[lvl], ni + 1, 1, 1, 1, False, ws,
                          out=self.c["l2n_gy"] if normed else None)
        if normed:
            self.l2norm_bwd()
        self.written[ni + 1] = True

    def head_wgrad(self, lvl, ws):
        e = self.eng
        wt, bt = e.head_params[lvl]
        src = self.c["l2n_y"] if lvl == 0 and e.l2norm is not None else self.acts[e.fm[lvl][0] + 1]
        ops.conv2d_bwd_weight(src, self.packed[lvl], wt.shape[0], 3, 1, 1, 1, dw=e.view(wt, e.grad), dbias=e.view(bt, e.grad), ws=ws)

    def masked_dgrad(self, key, dy, w_t, a, stride, pt, pl, accumulate, ws, out=None):
        """Data gradient w.r.t. activation a (index), masked by its ReLU sign: from the sign bits where this step's forward
        pass wrote them and the kernel reads them (learned per call site), else from the bf16 activation.  out: where it
        goes instead of gacts[a]."""
        e, x = self.eng, self.acts[a]
        out = self.gacts[a] if out is None else out
        if e.relu_bits is not None and a in e.bits_valid and e.relu_bits.get(key, True):
            e.relu_bits[key] = _launched(ops.conv2d_bwd_data_bits, dy, w_t, self.c["rbits"][a], x.shape, stride, pt, pl,
                                         accumulate=accumulate, out=out, ws=ws)
            if e.relu_bits[key]:
                return
        ops.conv2d_bwd_data(dy, w_t, x, x.shape, stride, pt, pl, accumulate=accumulate, out=out, ws=ws)

    def wgrad(self, i, ws):
        e, nd = self.eng, self.eng.nodes[i]
        wt, bt = e.conv_params[i]
        probe = e.wgrad_probe                              # measurement only (bench.py): HIP events around the launches of chosen layers
        timed = probe is not None and i in probe["nodes"]
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if nd["dilation"] != 1:                            # (a workspace of its own size, from the same stream's buffer)
            ops.conv2d_atrous_bwd_weight(self.acts[i], self.gacts[i + 1], nd["cout"], nd["dilation"], dw=e.view(wt, e.grad),
                                         dbias=e.view(bt, e.grad), ws=ws)
        else:
            ops.conv2d_bwd_weight(self.acts[i], self.gacts[i + 1], nd["cout"], nd["k"], nd["stride"], nd["pt"], nd["pl"],
                                  dw=e.view(wt, e.grad), dbias=e.view(bt, e.grad), ws=ws)
        if timed:
            e1.record()
            probe["events"].append((i, e0, e1))

    def dw_wgrad(self, i, ws):
        e, nd = self.eng, self.eng.nodes[i]
        wt, bt = e.conv_params[i]
        ops.dwconv3x3_bwd_weight(self.acts[i], self.gacts[i + 1], nd["stride"], nd["pt"], nd["pl"], dw=e.view(wt, e.grad),
                                 dbias=e.view(bt, e.grad), ws=ws)

    def dw_dgrad(self, i):
        """Data gradient of depthwise node i on the main stream, masked by the ReLU of the node in front of it: from that
        node's sign bytes where this step's forward pass wrote them (and the engine takes them: dw_dgrad_bits), else from the
        bf16 map.  It reads the bf16 parameters themselves (no transposed copy): the bucket's optimizer, which rewrites them, is
        enqueued behind this launch like behind every other data gradient (opt_bucket)."""
        e, nd = self.eng, self.eng.nodes[i]
        assert e.nodes[i - 1]["kind"] in RELU_KINDS, "a depthwise node behind a pooling: no unmasked launch planned"
        self.wait_for_head(i)
        w = e.view(e.conv_params[i][0], e.param_bf16)
        x = self.acts[i]
        if e.relu_bits is not None and e.dw_dgrad_bits and i in e.bits_valid:
            ops.dwconv3x3_bwd_data_bits(self.gacts[i + 1], w, self.c["rbits"][i], x.shape, nd["stride"], nd["pt"], nd["pl"],
                                        accumulate=self.written[i], out=self.gacts[i])
        else:
            ops.dwconv3x3_bwd_data(self.gacts[i + 1], w, x, x.shape, nd["stride"], nd["pt"], nd["pl"], accumulate=self.written[i],
                                   out=self.gacts[i])
        self.written[i] = True

    def dgrad(self, i):
        """Data gradient of convolution i (> 0, not in the chain) on the main stream."""
        e, c, nd, written = self.eng, self.c, self.eng.nodes[i], self.written
        g_out = self.gacts[i + 1]
        if i == 1 and e.fuse_first and e.first_pair and not written[1] and e.relu_bits is not None and 1 in e.bits_valid:
            # ... and the first layer's weight gradient in one kernel (gacts[1] is consumed there, not written)
            wt0, bt0 = e.conv_params[0]
            self.first_fused = e.fuse_first = _launched(ops.conv2d_bwd_data_wgrad_first, g_out, e.w_t[1], c["rbits"][1], self.acts[0],
                                                        dw=e.view(wt0, e.grad), dbias=e.view(bt0, e.grad), ws=e._ws)
            if self.first_fused:
                written[1] = True
                return
        self.wait_for_head(i)
        # a 3x3 / stride-1 convolution right behind a pooling: its data gradient is carried through the pooling in the
        # convolution's own store stage (no pooled gradient in HBM, no pooling-backward launch) where an LDS-patch kernel
        # serves the layer; learned at the first call, like pool_only
        fused = False
        if (e.fuse_unpool is not None and e.fuse_unpool.get(i, True) and e.nodes[i - 1]["kind"] == "pool" and not written[i]
                and not written[i - 1] and nd["k"] == 3 and nd["stride"] == 1 and nd["pt"] == 1 and nd["pl"] == 1):
            fused = e.fuse_unpool[i] = _launched(ops.conv2d_bwd_data_unpool, g_out, e.w_t[i], None, c["pool_code"][i - 1],
                                                 tuple(self.gacts[i - 1].shape), out=self.gacts[i - 1], ws=e._ws)
            if fused:
                self.unpooled.add(i - 1)
        if nd["dilation"] != 1:
            # fc6 behind pool5: the pooling's codes carry the ReLU of the layer in front of it, nothing to mask here
            assert e.nodes[i - 1]["kind"] not in RELU_KINDS, "a dilated convolution behind a convolution: no masked launch planned"
            ops.conv2d_atrous_bwd_data(g_out, e.w_t[i], None, self.acts[i].shape, nd["dilation"], accumulate=written[i],
                                       out=self.gacts[i])
        elif not fused and e.nodes[i - 1]["kind"] in RELU_KINDS:    # (its ReLU masks the gradient)
            self.masked_dgrad("conv%d" % i, g_out, e.w_t[i], i, nd["stride"], nd["pt"], nd["pl"], written[i], e._ws)
        elif not fused:
            ops.conv2d_bwd_data(g_out, e.w_t[i], None, self.acts[i].shape, nd["stride"], nd["pt"], nd["pl"],
                                accumulate=written[i], out=self.gacts[i], ws=e._ws)
        written[i] = True


class SSDEngine:
    # backward() takes the per-bucket optimizer schedule (fused_adam / on_dgrad); an engine without it is stepped by
    # backward -> clip_scales -> one optimizer launch over the flat buffer
    bucket_optimizer = True
    # backward() spreads its work over side streams (weight gradients, heads, optimizer buckets) around the data-gradient
    # chain on the caller's stream: what a high-priority stream for that chain is good for
    side_streams = True
    # the exponential moving average of the weights (enable_ema): a second flat fp32 buffer, the updates it has taken, and the
    # factor 1 - decay of the optimizer step in flight (None: the optimizer launches are followed by nothing)
    ema = None
    ema_updates = 0
    ema_om = None
    _averaged = False                          # inside `with averaged():` param and ema have changed places

    def __init__(self, classes=81, in_size=300, trunk=SSD300_TRUNK, num_priors=SSD300_NUM_PRIORS, device="cuda",
                 seed=0, sparse_heads=None, l2norm=None, fp8_inference=False):
        """l2norm: the SSD paper's L2 normalisation of feature map 0 in front of its head (ops.L2NormSpec.of: None / False = off,
        True, an initial scale, a dict or a spec).  Off, the engine plans the same tensors and launches what it did without
        the option; on, one more variable "l2norm0/scale" follows every other one.
        fp8_inference: plan forward(x, "mxfp8") for a trunk with a 3x3 / stride-1 pooling or a dilated convolution as well (the
        VGG-16 SSD300: mxfp8_trunk_plan's quantising poolings and the fp8 atrous convolution).  Off, such a trunk is
        bf16_only and refuses that forward, as it always did; a trunk without those nodes has its fp8 plan either way."""
        # the heads' backward pass from the loss's compact gradient rows (csrc/sparse.hip); SSD_SPARSE_HEADS=0: the dense
        # kernels on the scattered gradient (tests compare the two)
        self._plan(classes, in_size, trunk, num_priors, device, l2norm,
                   (os.environ.get("SSD_SPARSE_HEADS", "1") == "1") if sparse_heads is None else bool(sparse_heads),
                   fp8_inference=fp8_inference)
        # the trailing convolutions on LDS-sized maps (the extras behind the 19x19 map) as ONE launch, forward and data gradient
        # (ops.conv_chain); a set: {"fwd", "bwd"}, emptied by a refusal of the kernel
        self.chain = {"1": {"fwd", "bwd"}, "fwd": {"fwd"}, "bwd": {"bwd"}}.get(os.environ.get("SSD_CHAIN", "1"), set())
        self._alloc_params()
        self.init_params(seed)
        self._act_cache = {}
        self._ws = ops.MatchWorkspace()
        self._ws_hz = ops.MatchWorkspace()     # Z of the sparse head data gradient
        self._ws_hw = ops.MatchWorkspace()     # slabs of the sparse head weight gradient
        self._ws_l2n = ops.MatchWorkspace()    # partial sums of the l2norm scale's gradient
        self._streams = _Streams(self.device)
        self.overlap_heads = os.environ.get("SSD_OVERLAP_HEADS", "1") != "0" and self.device.type == "cuda"
        self.step_count = 0
        self.slots = "adam"                    # what adam_m holds: Adam's first moment, or "sgd_momentum": the velocity
        self.skip_fullres = os.environ.get("SSD_SKIP_FULLRES", "1") == "1"   # pooled convs store the pooled map only
        # schedule switches of the host program (read once, here): third stream for the small heads of the forward pass; dense
        # head path only: the two large heads' backward on the side stream, their gradient packing there too
        self.tail_stream = os.environ.get("SSD_TAIL_STREAM", "1") == "1"
        self.big_heads_side = os.environ.get("SSD_BIG_HEADS_SIDE", "1") == "1"
        self.pack_side = os.environ.get("SSD_PACK_SIDE", "1") == "1"
        self.batch_chain_wgrads = os.environ.get("SSD_BATCH_CHAIN_WGRADS", "1") == "1"
        self.wgrad_group = int(os.environ.get("SSD_WGRAD_GROUP", "3"))      # weight-gradient launches per cross-stream wait
        self.split_heads_dgrad = int(os.environ.get("SSD_SPLIT_HEADS_DGRAD", "2"))   # 0 one call, 1 small | large levels, 2 ... and one call per large level
        # the heads of the maps the forward chain produces (all available at once, behind one launch): every other one on the
        # main stream instead of queueing all of them on the third
        self.chain_heads_split = os.environ.get("SSD_CHAIN_HEADS_SPLIT", "1") == "1"
        self.chain_prefetch = os.environ.get("SSD_CHAIN_PREFETCH", "1") == "1"
        # fused-optimizer buckets that run at the END of the main stream instead of in the side stream's queue: the side stream (weight
        # gradients) is the longer chain, the main stream finishes ~0.5 ms earlier (round 4, same-box A/B: 1 -> 4 buckets -0.06 ms)
        self.opt_defer = int(os.environ.get("SSD_OPT_DEFER", "4"))
        self.pool_only = {}                    # node -> whether a pool-only kernel serves it (learned at the first call)
        self.fuse_unpool = {} if os.environ.get("SSD_FUSE_UNPOOL", "1") == "1" else None    # node -> data gradient un-pools itself
        # activation index -> its sign bits are written by the forward kernel (learned at the first call); data-gradient
        # key (str) -> that kernel reads them
        self.relu_bits = {} if os.environ.get("SSD_RELU_BITS", "1") == "1" else None
        self.bits_valid = set()
        # a depthwise node's data gradient takes its mask from the sign bytes (ops.dwconv3x3_bwd_data_bits) rather than from
        # the bf16 map: over the trunk's twelve masked depthwise data gradients at batch 64 it measured 336 us against 583 us
        # (DESIGN.md section 9); both paths give the same bits
        self.dw_dgrad_bits = os.environ.get("SSD_DW_DGRAD_BITS", "1") == "1"
        # second layer's data gradient and first layer's weight gradient in one kernel (the gradient w.r.t. the first layer's
        # output has no other consumer and is never stored); False after a refusal
        self.fuse_first = os.environ.get("SSD_FUSE_FIRST", "1") == "1"
        self.first_fused = False               # the last backward() ran that kernel: gacts[1] was consumed on chip, not written
        self.wgrad_probe = None                # dict(nodes={...}, events=[]): time those layers' weight-gradient launches in the step
        # what the last forward left behind: "bf16" (everything backward() reads), "mxfp8" (an inference fp8 forward: backward()
        # refuses) or, on an engine that trains in fp8, "mxfp8_train"
        self.last_forward = "bf16"

    # ---------------------------------------------------------------- static planning
    @classmethod
    def planned(cls, classes=81, in_size=300, trunk=SSD300_TRUNK, num_priors=SSD300_NUM_PRIORS, l2norm=None, fp8_inference=False):
        """The static plan alone (nodes, fm, grids, A, tensors, chain_start): no device is touched, nothing can be launched."""
        e = cls.__new__(cls)
        e._plan(classes, in_size, trunk, num_priors, "cpu", l2norm, True, fp8_inference=fp8_inference)
        return e

    def _plan(self, classes, in_size, trunk, num_priors, device, l2norm, sparse_heads, fp8_inference=False):
        """The static part of an engine, shared by __init__ and planned()."""
        self.L = _lib.lib()
        self.fp8_inference = bool(fp8_inference)
        self.l2norm = ops.L2NormSpec.of(l2norm)
        self.classes, self.in_size, self.device = classes, in_size, torch.device(device)
        self.trunk, self.num_priors, self.sparse_heads = list(trunk), tuple(num_priors), sparse_heads
        self.block = self.L.ssd_opt_block_elems()
        # inference in block-scaled fp8 (forward(x, "mxfp8")): the plan (mxfp8_trunk_plan, at its first use), the stretch (lo, hi)
        # of param_bf16 that holds the fp8 layers' filters and its quantised form
        self._mx_plan, self._mx_range = None, None
        self.mx_filters = mx.FlatStore()
        self._plan_shapes()
        self._plan_params()

    def _plan_shapes(self):
        s = self.in_size
        self.nodes = []                       # dicts: kind, cin, cout, k, stride, pt, pl, hin, hout, feature
        self.fm = []                          # (node index, h, c)
        for kind, cin, cout, k, stride, mode, feat, *more in self.trunk:
            dilation = more[0] if more else 1                # (an optional eighth element: only the VGG-16 trunk's fc6 has one)
            if kind == "dwconv" and (cin != cout or cin % 8 or (k, mode) != (3, "same") or stride not in (1, 2) or more or not self.nodes):
                raise ValueError("trunk node %d: a depthwise node is (\"dwconv\", C, C, 3, 1 | 2, \"same\", feature) with C a multiple "
                                 "of 8, behind another node; got %r" % (len(self.nodes), (kind, cin, cout, k, stride, mode, feat) + tuple(more)))
            if kind not in ("conv", "dwconv", "pool", "pool3s1") or (dilation != 1 and (kind, k, stride, mode) != ("conv", 3, 1, "same")):
                raise ValueError("trunk node %d: no launch for %r" % (len(self.nodes), (kind, cin, cout, k, stride, mode, feat) + tuple(more)))
            if mode == "same":
                ho, pt = ops.same_pad(s, dilation * (k - 1) + 1, stride)
            else:
                ho, pt = ops.valid_out(s, k, stride), 0
            self.nodes.append(dict(kind=kind, cin=cin, cout=cout, k=k, stride=stride, pt=pt, pl=pt, hin=s, hout=ho,
                                   feature=feat, same=(mode == "same"), dilation=dilation))
            s = ho
            if feat:
                self.fm.append((len(self.nodes) - 1, ho, cout))
        assert len(self.fm) == len(self.num_priors)
        # the chain: the longest run of trailing convolutions whose input and output maps have <= 112 pixels and whose channel
        # counts are multiples of 128 (ssd_conv_chain's limits), each behind another convolution (its ReLU is the mask)
        j = len(self.nodes)
        while (j > 1 and len(self.nodes) - j < _lib.SSD_CHAIN_MAX_LAYERS and self.nodes[j - 1]["kind"] == "conv"
               and self.nodes[j - 2]["kind"] == "conv" and self.nodes[j - 1]["hin"] ** 2 <= 112 and self.nodes[j - 1]["hout"] ** 2 <= 112
               and self.nodes[j - 1]["cin"] % 128 == 0 and self.nodes[j - 1]["cout"] % 128 == 0
               and self.nodes[j - 1]["dilation"] == 1):
            j -= 1
        # ... and, in a trunk with depthwise nodes, whose images fit the kernel's LDS in both directions (ops.chain_lds_bytes:
        # ssd_conv_chain's own arithmetic): a run that does not fit loses its first layers until it does, so what is planned
        # here is what launches (MobileNet: 10x10x1024 in front of the extras is 206 KB; the chain starts one layer later).
        # The older trunks keep the rule above and learn a refusal at the first launch (self.chain empties): only a reduced
        # geometry of theirs is refused (the VGG-16 trunk at 164), and their plans and launches stay what they were
        self.has_dw = any(nd["kind"] == "dwconv" for nd in self.nodes)
        while self.has_dw and len(self.nodes) - j >= 2 and not self._chain_fits(j):
            j += 1
        self.chain_start = j if len(self.nodes) - j >= 2 else None
        if any(c % 128 for _, _, c in self.fm) or len(self.fm) > _lib.SSD_MAX_LEVELS:
            self.sparse_heads = False
        self.level_off = [0]
        for (_, h, _), n in zip(self.fm, self.num_priors):
            self.level_off.append(self.level_off[-1] + h * h * n)
        self.A = self.level_off[-1]            # 8732 for SSD300 (models/ssd_model.py:221)
        self.grids = tuple((h, h) for _, h, _ in self.fm)
        # the first two layers are the pair ops.conv2d_bwd_data_wgrad_first serves: 3x3 / stride 1, 8 -> 64 -> 64 channels
        pair = [(nd["kind"], nd["cin"], nd["cout"], nd["k"], nd["stride"]) for nd in self.nodes[:2]]
        self.first_pair = (pair == [("conv", 8, 64, 3, 1), ("conv", 64, 64, 3, 1)]
                           and self.nodes[1]["pt"] == self.nodes[1]["pl"] == 1)
        # node kinds the block-scaled fp8 forward plans only where the engine was built with fp8_inference (the VGG-16 SSD300's
        # pool5 and fc6)
        # ...; a depthwise node has no fp8 form at all
        if self.has_dw and getattr(self, "fp8_inference", False):
            raise ValueError("fp8_inference=True: a trunk with depthwise (\"dwconv\") nodes runs in bf16 only")
        self.bf16_only = self.has_dw or (any(nd["kind"] == "pool3s1" or nd["dilation"] != 1 for nd in self.nodes)
                                         and not getattr(self, "fp8_inference", False))

    def _chain_fits(self, j):
        """Whether nodes j .. end as ONE ssd_conv_chain launch stay within its LDS, forward (images: the input of node j, then
        every output but the last) and data gradient (the last node's output gradient first, the walk reversed)."""
        nds = self.nodes[j:]
        fwd = [(nd["hin"] ** 2, nd["cin"], nd["hout"] ** 2, nd["cout"]) for nd in nds]
        bwd = [(nd["hout"] ** 2, nd["cout"], nd["hin"] ** 2, nd["cin"]) for nd in reversed(nds)]
        return max(ops.chain_lds_bytes(fwd), ops.chain_lds_bytes(bwd)) <= ops.CHAIN_LDS_MAX

    def _plan_params(self):
        self.tensors = []
        off = 0

        def add(name, shape, end_aligned=False):
            nonlocal off
            numel = int(np.prod(shape))
            nb = (numel + self.block - 1) // self.block
            # end-aligned: the tensor ENDS on a block boundary (the next one starts there: one contiguous GEMM operand over two
            # optimizer variables); its start must stay 16-byte aligned in the bf16 copy too (DMA, float4)
            start = off + (nb * self.block - numel if end_aligned else 0)
            if start % 8:
                raise ValueError("%s: %d elements do not end-align on a 16-byte boundary (per-cell anchor counts must make "
                                 "n*4 a multiple of 8, i.e. even: the reference's are 4 and 6)" % (name, numel))
            t = ParamTensor(name, shape, start, len(self.tensors), off // self.block, nb)
            self.tensors.append(t)
            off += nb * self.block
            return t

        self.conv_params = {}
        for i, nd in enumerate(self.nodes):
            if nd["kind"] == "dwconv":                      # [3][3][C]: what the kernels read, forward and data gradient
                self.conv_params[i] = (add("dwconv%d/kernel" % i, (3, 3, nd["cout"])), add("dwconv%d/bias" % i, (nd["cout"],)))
            if nd["kind"] != "conv":
                continue
            self.conv_params[i] = (add("conv%d/kernel" % i, (nd["cout"], nd["k"], nd["k"], nd["cin"])),
                                   add("conv%d/bias" % i, (nd["cout"],)))
        self.head_params = []
        for lvl, ((_, h, c), n) in enumerate(zip(self.fm, self.num_priors)):
            # loc filters (n*4) then conf filters (n*classes): one fused GEMM over two variables each (kernel, bias)
            nl, nc = n * 4, n * self.classes
            lk, ck = add("head%d/loc_kernel" % lvl, (nl, 3, 3, c), True), add("head%d/conf_kernel" % lvl, (nc, 3, 3, c))
            lb, cb = add("head%d/loc_bias" % lvl, (nl,), True), add("head%d/conf_bias" % lvl, (nc,))
            self.head_params.append((FusedView("head%d/kernel" % lvl, (nl + nc, 3, 3, c), (lk, ck)),
                                     FusedView("head%d/bias" % lvl, (nl + nc,), (lb, cb))))
        # the scale of the L2 normalisation in front of head 0: behind every other tensor, so those keep index, offset and
        # block; opt_buckets() then has it in the heads' bucket (which ends at len(self.tensors))
        self.l2norm_scale = None
        if self.l2norm is not None:
            c0 = self.fm[0][2]
            if c0 % 128 or not 128 <= c0 <= 1024:
                raise ValueError("l2norm: feature map 0 has %d channels; the kernels serve multiples of 128 in 128 .. 1024" % c0)
            self.l2norm_scale = add("l2norm0/scale", (c0,))
        self._plan_extra_params(add)
        self.n_flat = off
        self.n_params = sum(t.numel for t in self.tensors)

    def _plan_extra_params(self, add):
        """Variables of a subclass, behind every tensor planned above (which keep their index, offset and block)."""

    def _alloc_params(self):
        dev, n = self.device, self.n_flat
        self.param = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grad_acc = None
        self.adam_m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.adam_v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.param_bf16 = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        nb = n // self.block
        tbo = np.zeros(len(self.tensors) + 1, np.int32)
        bt = np.zeros(nb, np.int32)
        for i, t in enumerate(self.tensors):
            b0, b1 = t.block0, t.block0 + t.nblocks
            tbo[i], tbo[i + 1] = b0, b1
            bt[b0:b1] = i
        self.tensor_block_off = torch.from_numpy(tbo).to(dev)
        self.block_tensor = torch.from_numpy(bt).to(dev)
        self.sq_partial = torch.empty(nb, dtype=torch.float64, device=dev)
        self.clip_scale = torch.empty(len(self.tensors), dtype=torch.float32, device=dev)
        self.grad_norms = torch.empty(len(self.tensors), dtype=torch.float32, device=dev)
        # transposed weights for the data gradient (own buffers)
        self.w_t = {}
        for i, nd in enumerate(self.nodes):
            if nd["kind"] == "conv" and i > 0:
                self.w_t[i] = torch.empty((nd["cin"], nd["k"], nd["k"], nd["cout"]), dtype=torch.bfloat16, device=dev)
        # fragment-packed copies of the chain layers' filters (ops.conv_chain's operands), forward and data gradient
        self.chain_pk_fwd, self.chain_pk_bwd = {}, {}
        if getattr(self, "chain_start", None) is not None and self.chain:
            for i in range(self.chain_start, len(self.nodes)):
                nd = self.nodes[i]
                self.chain_pk_fwd[i] = torch.empty((nd["cout"], nd["k"], nd["k"], nd["cin"]), dtype=torch.bfloat16, device=dev)
                self.chain_pk_bwd[i] = torch.empty_like(self.w_t[i])
        self.head_npad = [(n * (4 + self.classes) + 7) // 8 * 8 for n in self.num_priors]
        # transposed head filters: [Cin][3][3][npad] flipped for the dense data gradient, or tap-major [3][3][Cin][npad] for
        # the sparse one
        self.head_w_t = [torch.empty((3, 3, c, npad) if self.sparse_heads else (c, 3, 3, npad), dtype=torch.bfloat16, device=dev)
                         for (_, _, c), npad in zip(self.fm, self.head_npad)]

    # ---------------------------------------------------------------- parameter views
    def view(self, t, buf):
        return buf[t.offset:t.offset + t.numel].view(t.shape)

    def init_params(self, seed=0):
        """Keras defaults: glorot_uniform kernels, zero biases (the reference's VGG part loads ImageNet weights
        from the network, which is unavailable offline -- SURVEY.md F9); the l2norm scale, where planned, at its spec's init."""
        rng = np.random.default_rng(seed)
        host = np.zeros(self.n_flat, np.float32)
        for t in self.tensors:
            if not t.name.endswith("kernel"):
                continue
            if t.name.startswith("dwconv"):
                # He-uniform over the true fan-in 9 (variance 2 / 9): thirteen depthwise layers without a normalisation keep
                # their maps alive; Keras's glorot over 9C + 9 shrinks every map by ~1 / C and the network dies out
                lim = math.sqrt(6.0 / 9.0)
                host[t.offset:t.offset + t.numel] = rng.uniform(-lim, lim, t.shape).astype(np.float32).reshape(-1)
                continue
            cout, k, _, cin = t.shape
            if t.name.startswith("head"):                       # loc and conf: two separate Keras layers (:155-162)
                lim = math.sqrt(6.0 / (k * k * cin + k * k * cout))
                w = rng.uniform(-lim, lim, (cout, k, k, cin))
            else:
                real_cin = IMAGE_CHANNELS if t.name == "conv0/kernel" else cin
                lim = math.sqrt(6.0 / (k * k * real_cin + k * k * cout))
                w = rng.uniform(-lim, lim, (cout, k, k, cin))
                if real_cin != cin:
                    w[..., real_cin:] = 0.0
            host[t.offset:t.offset + t.numel] = w.astype(np.float32).reshape(-1)
        if self.l2norm_scale is not None:
            t = self.l2norm_scale
            host[t.offset:t.offset + t.numel] = self.l2norm.init
        self.param.copy_(torch.from_numpy(host))
        self.adam_m.zero_()
        self.adam_v.zero_()
        self.step_count = 0
        self.refresh_weights(cast=True)

    def set_background_prior(self, pi=0.01):
        """Start every head's class biases at a foreground prior (Lin et al. 2017, section 4.1, for C softmax logits): for every
        default box the bias of conf channel C-1 becomes log((C-1)(1-pi)/pi) and the other conf biases 0, so that a head whose
        filters contribute nothing puts 1 - pi on the background and pi / (C-1) on every class.  Loc biases and all filters
        keep their bits.  Every copy the forward passes read is refreshed: the bf16 parameters, what is derived from them,
        and the fp8 operand store where one exists.  pi in (0, 1), else ValueError.
        Never called implicitly: a focal loss wants it before the first step of a run from scratch."""
        if isinstance(pi, bool) or not isinstance(pi, (int, float, np.integer, np.floating)) or not 0.0 < pi < 1.0:
            raise ValueError("pi must be a number in (0, 1), not %r" % (pi,))
        C = self.classes
        row = torch.zeros(C, dtype=torch.float32, device=self.device)
        row[C - 1] = math.log((C - 1) * (1.0 - pi) / pi)
        for _, bt in self.head_params:
            cb = bt.parts[1]                                   # "head%d/conf_bias": [per_cell * C], a box's C channels together
            self.view(cb, self.param).view(-1, C).copy_(row)
        self.refresh_weights(cast=True)
        if self.mx_filters.allocated:                          # an fp8 forward has run: its operand store follows param_bf16
            self._quantize_filters()

    def refresh_weights(self, cast=False, tensors=None):
        """bf16 copy (if not already written by the optimizer kernel) + transposed copies for the data gradient.
        tensors=(t0, t1): only the copies of parameter tensors t0..t1-1 (the per-bucket optimizer step)."""
        if cast:
            ops.cast_bf16(self.param, self.param_bf16)
        if getattr(self, "_tr_desc", None) is None:         # {src, dst, Cout, k, Cin, Cout_pad} per transposed copy
            rows, tiles = [], 0
            pairs = [(self.conv_params[i][0], wt) for i, wt in self.w_t.items()]
            n_trunk = len(pairs)
            pairs += [(self.head_params[lvl][0], wt) for lvl, wt in enumerate(self.head_w_t)]
            for r, (pt, wt) in enumerate(pairs):
                cout, k, _, cin = pt.shape
                cpad = wt.shape[-1]
                kfield = k | (0x100 if (self.sparse_heads and r >= n_trunk) else 0)     # bit 8: tap-major, not flipped
                rows.append([self.view(pt, self.param_bf16).data_ptr(), wt.data_ptr(), cout, kfield, cin, cpad])
                tiles = max(tiles, ((cpad + 31) // 32) * ((cin + 31) // 32) * k * k)
            self._tr_desc = torch.tensor(rows, dtype=torch.int64, device=self.device)
            self._tr_tiles = tiles
            self._tr_tensor = [pt.index for pt, _ in pairs]      # ascending: trunk kernels, then head kernels
        r0, r1 = 0, self._tr_desc.shape[0]
        if tensors is not None:
            inside = [r for r, t in enumerate(self._tr_tensor) if tensors[0] <= t < tensors[1]]
            if not inside:
                return
            r0, r1 = inside[0], inside[-1] + 1
            assert inside == list(range(r0, r1))
        _lib.check(self.L.ssd_weight_transpose_batched(ops._ptr(self._tr_desc[r0:]), r1 - r0, self._tr_tiles,
                                                       ops._stream()))
        if self.chain_pk_fwd:                                # ... and the chain's fragment-packed copies of the same tensors
            items = []
            for i in self.chain_pk_fwd:
                wt = self.conv_params[i][0]
                if tensors is None or tensors[0] <= wt.index < tensors[1]:
                    items += [(self.view(wt, self.param_bf16), self.chain_pk_fwd[i]), (self.w_t[i], self.chain_pk_bwd[i])]
            if items:
                ops.chain_pack_weights(items)

    # ---------------------------------------------------------------- activations
    def _acts(self, B):
        c = self._act_cache.get(B)
        if c is None:
            dev = self.device
            acts = [None]                         # acts[0] = network input, set per call
            gacts = [None]
            for nd in self.nodes:
                shape = (B, nd["hout"], nd["hout"], nd["cout"])
                acts.append(torch.empty(shape, dtype=torch.bfloat16, device=dev))
                gacts.append(torch.empty(shape, dtype=torch.bfloat16, device=dev))
            loc = torch.empty((B, self.A, 4), dtype=torch.bfloat16, device=dev)
            conf = torch.empty((B, self.A, self.classes), dtype=torch.bfloat16, device=dev)
            packed = [torch.empty((B, h * h, npad), dtype=torch.bfloat16, device=dev)
                      for (_, h, _), npad in zip(self.fm, self.head_npad)]
            pool_code = {i: torch.empty((B, nd["hout"], nd["hout"], nd["cout"] // 8), dtype=torch.int32, device=dev)
                         for i, nd in enumerate(self.nodes) if nd["kind"] in ("pool", "pool3s1")}
            # ReLU sign bits of every convolution output (one byte per pixel and 8 channels): what the data gradients read
            # instead of the bf16 activation
            rbits = {i + 1: torch.empty((B, nd["hout"], nd["hout"], nd["cout"] // 8), dtype=torch.uint8, device=dev)
                     for i, nd in enumerate(self.nodes) if nd["kind"] in RELU_KINDS and nd["cout"] % 8 == 0}
            hgb = None
            if self.sparse_heads:
                hgb = ops.HeadGradBuffers(B, [h * h for _, h, _ in self.fm], self.num_priors, self.head_npad, device=dev)
            c = dict(acts=acts, gacts=gacts, loc=loc, conf=conf, packed=packed, pool_code=pool_code, rbits=rbits, hgb=hgb)
            if self.l2norm is not None:
                # the normalised feature map 0 (what head 0 reads; the trunk keeps the map itself), 1 / norm per pixel as the
                # forward pass computed it, and the gradient w.r.t. the normalised map (head 0's data gradient)
                a0 = acts[self.fm[0][0] + 1]
                c["l2n_y"], c["l2n_gy"] = torch.empty_like(a0), torch.empty_like(a0)
                c["l2n_r"] = torch.empty((a0.numel() // a0.shape[-1],), dtype=torch.float32, device=dev)
            self._act_cache = {B: c}              # keep one batch size resident
        return c

    # ---------------------------------------------------------------- forward / backward
    # Two HIP streams.  The two large heads (38x38 and 19x19 maps) are independent of the small tail of the network
    # (conv 12-19 and heads 2-5: ~45 short, latency-bound launches that leave most CUs idle), so they run on a side
    # stream next to it, forward and backward; results do not depend on this (disjoint outputs, the one shared
    # accumulation target is ordered by an event).
    SIDE_HEADS = (0, 1)
    BIG_LEVEL_PIXELS = 16384                   # backward: a level with at least B * h * h of them is a "large" one (SSD300: 38x38 from B = 12, 19x19 from 46)

    _side = property(lambda self: self._streams.side)
    _ws_side = property(lambda self: self._streams.ws_side)
    _ws_tail = property(lambda self: self._streams.ws_tail)

    def _side_stream(self):
        return self._streams.side_stream()

    def forward(self, x, precision="bf16"):
        """x: bf16 [B, S, S, 8] (ops.image_prep).  Returns (loc bf16 [B,A,4], conf bf16 [B,A,classes]).
        precision="mxfp8": inference only -- the trunk layers of mxfp8_trunk_plan on block-scaled fp8 operands, the rest, the
        chain and the heads in bf16, on the same streams as the bf16 forward; backward() then raises until a bf16 forward."""
        if precision == "mxfp8":
            if self.bf16_only:
                raise NotImplementedError("forward(x, 'mxfp8'): this trunk (3x3 / stride-1 pooling and dilated fc6 of the VGG-16 SSD300 "
                                          "without fp8_inference, or depthwise nodes) has no block-scaled fp8 plan; it runs in bf16")
            return self._forward_vgg_mxfp8(x)
        if precision != "bf16":
            raise ValueError("precision must be 'bf16' or 'mxfp8', not %r" % (precision,))
        self.last_forward = "bf16"
        return self._walk(x, self._bf16_node)

    def _head_fwd(self, lvl, c, ws):
        """The head of level lvl (behind the L2 normalisation of its map where the engine has one), into c["loc"] / c["conf"]."""
        wt, bt = self.head_params[lvl]
        src = c["acts"][self.fm[lvl][0] + 1]
        if lvl == 0 and self.l2norm is not None:
            src = ops.l2norm_fwd(src, self.view(self.l2norm_scale, self.param), out=c["l2n_y"], rnorm=c["l2n_r"],
                                 eps=self.l2norm.eps)
        ops.conv2d_head_fwd(src, self.view(wt, self.param_bf16), self.view(bt, self.param), c["loc"], c["conf"],
                            self.num_priors[lvl], self.classes, self.level_off[lvl], ws=ws)

    def _walk(self, x, launch_node):
        """The forward pass: trunk nodes through launch_node(i, c) (the chain excepted), heads, chain and their streams."""
        B = x.shape[0]
        c = self._acts(B)
        acts = c["acts"]
        acts[0] = x
        main = torch.cuda.current_stream()
        side = self._side_stream() if self.overlap_heads else None
        tail = self._streams.tail_stream() if side is not None and self.tail_stream else None
        fm_level = {ni: lvl for lvl, (ni, _, _) in enumerate(self.fm)}

        def after_node(i):
            """Launch the head of the feature map node i produced, where it runs next to the trunk."""
            lvl = fm_level.get(i)
            if side is not None and lvl in self.SIDE_HEADS:
                s, ws = side, self._ws_side
            elif tail is not None and lvl is not None:
                # the small levels' heads (10x10 and below: a few workgroups each) on a third stream, as soon as their map
                # exists: next to the extras' chain on the main stream and the 19x19 head on the side stream they cost
                # nothing, behind them they were 190 us of a nearly idle GPU
                s, ws = tail, self._ws_tail
            else:
                return
            with _Streams.behind(s, main):
                self._head_fwd(lvl, c, ws)

        self.bits_valid = set()
        for i, nd in enumerate(self.nodes):
            if (self.chain_start is not None and i == self.chain_start - 1 and "fwd" in self.chain and tail is not None
                    and self.chain_prefetch):
                with _Streams.behind(tail, main):                  # the chain's packed filters into L2 while the layer in front of it runs
                    ops.chain_prefetch([self.chain_pk_fwd[j] for j in range(self.chain_start, len(self.nodes))])
            if i == self.chain_start and "fwd" in self.chain:
                # nodes i .. end in one launch, one workgroup per image (ops.conv_chain)
                want_bits = self.relu_bits is not None
                layers = []
                for j in range(i, len(self.nodes)):
                    ndj = self.nodes[j]
                    wt, bt = self.conv_params[j]
                    rb = c["rbits"].get(j + 1) if want_bits else None
                    layers.append(ops.chain_layer_fwd(self.view(wt, self.param_bf16), self.chain_pk_fwd[j], self.view(bt, self.param), acts[j + 1],
                                                      ndj["stride"], ndj["pt"], ndj["pl"], relu=True, relu_bits=rb))
                if _launched(ops.conv_chain, acts[i], layers):
                    nth = 0
                    for j in range(i, len(self.nodes)):
                        if layers[j - i]["relu_bits"] is not None:
                            self.bits_valid.add(j + 1)
                        lvl = fm_level.get(j)
                        if lvl is not None and tail is not None and self.chain_heads_split and lvl not in self.SIDE_HEADS:
                            nth += 1
                            if nth % 2 == 0:
                                self._head_fwd(lvl, c, self._ws)           # (the main stream has nothing else left to do)
                                continue
                        after_node(j)
                    break
                self.chain = set()
            launch_node(i, c)
            after_node(i)
        for lvl in range(len(self.fm)):
            if side is None or (lvl not in self.SIDE_HEADS and tail is None):
                self._head_fwd(lvl, c, self._ws)
        if side is not None:
            main.wait_stream(side)
            if tail is not None:
                main.wait_stream(tail)
        return c["loc"], c["conf"]

    @staticmethod
    def _pool_same(nd):
        """Whether pooling node nd keeps the last row / column of an odd map (TF 'SAME': hout = ceil(hin / 2)); a VALID pooling
        of an odd map drops it (hout = floor(hin / 2)), and on an even map the two are the same windows."""
        return nd["hout"] * 2 > nd["hin"]

    def _bf16_node(self, i, c):
        """Launch trunk node i of the bf16 forward (a pool behind a convolution runs inside that convolution's call)."""
        nd, acts = self.nodes[i], c["acts"]
        if nd["kind"] == "conv":
            wt, bt = self.conv_params[i]
            args = (acts[i], self.view(wt, self.param_bf16), self.view(bt, self.param), nd["stride"], nd["pt"], nd["pl"],
                    nd["hout"], nd["hout"])
            nxt = self.nodes[i + 1] if i + 1 < len(self.nodes) else None
            if nd["dilation"] != 1:                            # fc6: no sign bytes, its consumer's data gradient reads the map
                ops.conv2d_atrous_fwd(args[0], args[1], args[2], nd["dilation"], True, out=acts[i + 1])
            elif nxt is not None and nxt["kind"] == "pool":    # conv + the pooling behind it in one call
                # nothing but the pooling reads this conv's full-resolution output (the backward pass works from the
                # pooled map and the winner codes): ask for the pooled map only, where a fused kernel serves the layer.
                # A feature map is read by its head as well: its full-resolution map is always stored
                pool_only = False if nd["feature"] else self.pool_only.get(i, self.skip_fullres)
                args += (True, self._pool_same(nxt))
                kw = dict(out=acts[i + 1], pool_out=acts[i + 2], code=c["pool_code"][i + 1], ws=self._ws)
                if pool_only:                     # (refused with SSD_ERR_VALUE: no pooling kernel for this shape)
                    pool_only = _launched(ops.conv2d_fwd_pool, *args, pool_only=True, refused=ValueError, **kw)
                self.pool_only[i] = pool_only
                if not pool_only:                 # (with the map stored the library pools in a second launch where no kernel fuses it)
                    ops.conv2d_fwd_pool(*args, **kw)
            else:
                done = False
                if self.relu_bits is not None and self.relu_bits.get(i + 1, True) and (i + 1) in c["rbits"]:
                    done = self.relu_bits[i + 1] = _launched(ops.conv2d_fwd_relubits, *args, c["rbits"][i + 1], out=acts[i + 1],
                                                             ws=self._ws)
                    if done:
                        self.bits_valid.add(i + 1)
                if not done:
                    ops.conv2d_fwd(*args, True, out=acts[i + 1], ws=self._ws)
        elif nd["kind"] == "dwconv":
            wt, bt = self.conv_params[i]
            args = (acts[i], self.view(wt, self.param_bf16), self.view(bt, self.param), nd["stride"], nd["pt"], nd["pl"],
                    nd["hout"], nd["hout"])
            if self.relu_bits is not None:                     # (the sign-byte form serves every shape the plain one serves)
                ops.dwconv3x3_fwd_relubits(*args, c["rbits"][i + 1], out=acts[i + 1])
                self.bits_valid.add(i + 1)
            else:
                ops.dwconv3x3_fwd(*args, True, out=acts[i + 1])
        elif nd["kind"] == "pool3s1":
            ops.maxpool3x3s1_fwd(acts[i], out=acts[i + 1], code=c["pool_code"][i])
        elif i == 0 or self.nodes[i - 1]["kind"] != "conv":
            ops.maxpool2x2_fwd_argmax(acts[i], out=acts[i + 1], code=c["pool_code"][i],
                                      same=self._pool_same(nd))

    # ---------------------------------------------------------------- inference in block-scaled fp8 (MX e4m3)
    def mxfp8_plan(self):
        """mxfp8_trunk_plan of this engine's trunk (MxTrunkPlan), with the filters' stretch of param_bf16 laid out."""
        if self._mx_plan is None:
            plan = mxfp8_trunk_plan(self.nodes, self.chain_start)
            fp8 = plan.fp8
            # the fp8 layers' filters: their stretch of param_bf16 (conv filters start on optimizer-block boundaries, so every
            # layer's (q, scale) is a slice of mx_filters)
            lo = min(self.conv_params[i][0].offset for i in fp8)
            hi = max(bt.block0 + bt.nblocks for _, bt in (self.conv_params[i] for i in fp8)) * self.block
            assert all((self.conv_params[i][0].offset - lo) % 32 == 0 for i in fp8) and lo % 32 == 0 and (hi - lo) % 32 == 0
            self._mx_plan = plan
            self._mx_range = (lo, hi)
        return self._mx_plan

    def vgg_mxfp8_plan(self):
        """mxfp8_plan() as the 4-tuple (fp8, pooled, quant, writes)."""
        p = self.mxfp8_plan()
        return p.fp8, p.pooled, p.quant, p.writes

    def _mx_act_writes(self):
        """{node: forms of its output the fp8 forward stores}."""
        return self.mxfp8_plan().writes

    def _mx_pairs(self, B, key, nodes):
        """{node: mx.pair of its [B,H,W,C] map} for `nodes`, kept under `key` beside the bf16 activations of batch size B
        (allocated at the first use for that batch size: a bf16-only run allocates none)."""
        c = self._acts(B)
        if key not in c:
            c[key] = {i: mx.pair((B, self.nodes[i]["hout"], self.nodes[i]["hout"], self.nodes[i]["cout"]), self.device)
                      for i in nodes}
        return c[key]

    def mxfp8_acts(self, B):
        """{node: (q u8 [B,H,W,C], scale u8 [B,H,W,C/32])} for every node whose fp8 form the fp8 forward stores."""
        return self._mx_pairs(B, "mxfp8", [i for i, w in self._mx_act_writes().items() if "fp8" in w])

    def mxfp8_weights(self, i):
        """(q [Cout,k,k,Cin], scale [Cout,k,k,Cin/32]) of fp8 node i as the last fp8 forward quantised them."""
        wt = self.conv_params[i][0]
        return self.mx_filters.view(wt.offset - self._mx_range[0], wt.shape)

    def _quantize_filters(self):
        lo, hi = self._mx_range
        self.mx_filters.quantize(self.param_bf16[lo:hi])

    def _forward_vgg_mxfp8(self, x):
        maps8 = self.mxfp8_acts(x.shape[0])
        self._quantize_filters()
        self.last_forward = "mxfp8"            # the bf16 maps, ReLU bits and pool codes backward() reads are not all written
        return self._walk(x, lambda i, c: self._mxfp8_node(i, c, maps8))

    def _mxfp8_node(self, i, c, maps8):
        """Launch trunk node i of the fp8 forward: an fp8 convolution (with the pool behind it where the plan fuses one), a
        quantising pooling, or node i as the bf16 forward launches it (+ the plan's one standalone quantise of its output)."""
        fp8, pooled, qpool, quant, writes = self._mx_plan
        if i in pooled:
            return                                 # the fp8 convolution in front of it wrote its output
        if i in qpool:                             # reads the bf16 map in front of it, stores the pooled map in fp8
            nd, w = self.nodes[i], writes[i]
            kw = dict(want_bf16="bf16" in w, out=c["acts"][i + 1], q=maps8[i][0], scale=maps8[i][1])
            if nd["kind"] == "pool3s1":
                ops.maxpool3x3s1_fwd_mxfp8(c["acts"][i], **kw)
            else:
                ops.maxpool2x2_fwd_mxfp8(c["acts"][i], same=self._pool_same(nd), **kw)
            return
        if i not in fp8:
            self._bf16_node(i, c)
            if i in quant:
                ops.quantize_mx_fp8(c["acts"][i + 1], q=maps8[i][0], scale=maps8[i][1])
            return
        nd, acts = self.nodes[i], c["acts"]
        xq, xs = maps8[i - 1]
        wq, ws = self.mxfp8_weights(i)
        bias = self.view(self.conv_params[i][1], self.param)
        args = (xq, xs, wq, ws, bias, nd["stride"], nd["pt"], nd["pl"], nd["hout"], nd["hout"], True)
        o = i + 1 if i + 1 in pooled else i         # the node whose map this launch writes
        w = writes[o]
        q, sc = maps8.get(o, (None, None))
        kw = dict(want_bf16="bf16" in w, want_fp8="fp8" in w, out=acts[o + 1], out_q=q, out_scale=sc)
        if o != i:
            pnd = self.nodes[o]
            ops.conv2d_fwd_pool_mxfp8(*args, self._pool_same(pnd), **kw)
        elif nd["dilation"] != 1:
            ops.conv2d_atrous_fwd_mxfp8(xq, xs, wq, ws, bias, nd["dilation"], True, **kw)
        else:
            ops.conv2d_fwd_mxfp8(*args, **kw)

    def head_grad_buffers(self, B):
        """The ops.HeadGradBuffers the loss writes for a batch of B (None when the dense head path is selected)."""
        return self._acts(B)["hgb"]

    def heads_from_dense(self, dloc, dconf):
        """Compact rows from a dense (dloc, dconf) pair -- for callers that hold an arbitrary gradient (tests, the oracle
        comparison); the training step gets the rows from the loss directly.  Synchronises the host."""
        B = dloc.shape[0]
        hgb = self.head_grad_buffers(B)
        counts = []
        for lvl, (_, h, _) in enumerate(self.fm):
            npad = self.head_npad[lvl]
            packed = ops.head_grad_pack(dloc, dconf, h * h, self.num_priors[lvl], self.classes, npad,
                                        self.level_off[lvl]).view(B * h * h, npad)
            idx = (packed != 0).any(dim=1).nonzero().squeeze(1)
            k = int(idx.numel())
            hgb.rows[lvl][:k] = packed[idx]
            hgb.pixel_of_row[lvl][:k] = idx.int()
            hgb.row_of_pixel[lvl].fill_(-1)
            hgb.row_of_pixel[lvl][idx] = torch.arange(k, dtype=torch.int32, device=idx.device)
            counts.append(k)
        hgb.count[:len(counts)] = torch.tensor(counts, dtype=torch.int32, device=hgb.count.device)
        return hgb

    def _head_layers(self, c):
        acts, gacts = c["acts"], c["gacts"]
        idx = [ni + 1 for ni, _, _ in self.fm]
        use_bits = [self.relu_bits is not None and a in self.bits_valid for a in idx]
        xs, dxs = [acts[a] for a in idx], [gacts[a] for a in idx]
        if self.l2norm is not None:
            # head 0 reads the normalised map and its data gradient goes to that map's own buffer (l2norm_bwd turns it into
            # gacts); the ReLU mask stays the un-normalised map's: the normalised one is zero exactly where that one is
            xs[0], dxs[0] = c["l2n_y"], c["l2n_gy"]
        return ops.head_layers(
            xs, self.head_w_t, dxs,
            [self.view(wt, self.grad) for wt, _ in self.head_params], [self.view(bt, self.grad) for _, bt in self.head_params],
            [n * (4 + self.classes) for n in self.num_priors],
            relu_bits=[c["rbits"][a] if ub else None for a, ub in zip(idx, use_bits)],
            relu_src=[None if ub else acts[a] for a, ub in zip(idx, use_bits)])

    def bucket_gates(self, buckets):
        """For tensor ranges [(t0, t1)] (the gradient exchange's buckets): the trunk node whose data gradient is the last
        reader of the range's transposed weights (the lowest convolution in it), None for a range of head tensors only."""
        gates = []
        for t0, t1 in buckets:
            nodes = [i for i, (wt, bt) in self.conv_params.items() if t0 <= wt.index < t1 or t0 <= bt.index < t1]
            gates.append(min(nodes) if nodes else None)
        return gates

    def backward(self, dloc, dconf, on_ready=None, fused_adam=None, heads=None, on_dgrad=None):
        """Gradients of all parameters into self.grad (flat fp32) from d(loss)/d(loc), d(loss)/d(conf).
        on_ready([tensor indices]) is called right after the launches that complete those tensors' gradients (on the
        stream that runs them: an event recorded there covers them).
        fused_adam = dict(lr, beta1, beta2, eps, clip): clip_by_norm + Adam + weight copies run per bucket of tensors
        (opt_buckets) on the side stream as soon as the bucket's gradients exist and the last data gradient that reads
        its transposed weights has been enqueued -- the optimizer disappears under the rest of the backward pass.
        With kind="sgd_momentum" the dict is dict(kind, lr, momentum, nesterov, decay, clip) and the bucket's update is
        sgd_range() in the same places; without the key (or kind="adam") it is Adam's, as above.

        The data-gradient chain (the critical path) runs on the current stream, every weight gradient on the side
        stream as soon as its input gradient exists: the split reductions and round tails of one overlap the MFMA
        work of the other.  Each launch still sums in a fixed order, so results do not depend on the overlap."""
        self._live_only("backward()")
        if self.last_forward == "mxfp8":
            raise RuntimeError("backward() after an mxfp8 forward: it writes neither the bf16 maps nor the ReLU bits and pool "
                               "codes backward() reads; run forward(x) in bf16 first")
        if heads is None and self.sparse_heads:
            heads = self.heads_from_dense(dloc, dconf)
        B = heads.B if heads is not None else dloc.shape[0]
        p = _BackwardPass(self, self._acts(B), heads, dloc, dconf, on_ready, fused_adam, on_dgrad)
        p.plan_optimizer()                         # host only: which bucket's update follows which node's data gradient
        p.prefetch_chain()                         # third stream: the data-gradient chain's filters into L2
        # heads.  The two large levels (38x38, 19x19: ~1.1 ms of work) leave the main stream, data gradient first, so that the
        # main stream can walk the small levels and the extras' data-gradient chain (a dozen launches that each fill a
        # fraction of the chip) underneath them.  The accumulation order into a feature-map gradient is still "head
        # first, trunk second": the trunk launch waits for the head's event.
        if heads is not None:
            p.heads_sparse()                       # data gradients: main stream, large levels third stream; weight gradients: side
        else:
            p.heads_dense()                        # large levels whole on the side stream; the others' weight gradients too
        p.report_l2norm()
        p.opt_bucket(None)                         # the heads' optimizer bucket: side stream
        p.chain_dgrads()                           # main stream, one launch
        p.chain_wgrads()                           # side stream, one batched launch
        for i in range(len(self.nodes) - 1, -1, -1):   # trunk, last layer first
            p.node(i)                              # data gradient: main stream; weight gradient and optimizer bucket: side
        p.finish()                                 # joins the streams; the deferred optimizer buckets at the end of the main stream
        self.first_fused = p.first_fused

    # ---------------------------------------------------------------- optimizer
    def clip_scales(self, clip=0.01):
        """Per-tensor scale = clip / max(||g||, clip)  (tf.clip_by_norm, models/ssd_model.py:249)."""
        _lib.check(self.L.ssd_grad_clip_scales(ops._ptr(self.grad), self.n_flat, ops._ptr(self.tensor_block_off),
                                               len(self.tensors), float(clip), ops._ptr(self.sq_partial),
                                               ops._ptr(self.clip_scale), ops._ptr(self.grad_norms), ops._stream()))

    def apply_clip_in_place(self):
        _lib.check(self.L.ssd_grad_apply_scale(ops._ptr(self.grad), self.n_flat, ops._ptr(self.block_tensor),
                                               ops._ptr(self.clip_scale), ops._stream()))

    def _range_table(self, t0, t1):
        """(first block, tensor->block offsets, block->tensor map), both relative to the range, for tensors t0..t1-1."""
        key = (t0, t1)
        if not hasattr(self, "_range_tables"):
            self._range_tables = {}
        tab = self._range_tables.get(key)
        if tab is None:
            b0 = self.tensors[t0].block0
            tbo = (self.tensor_block_off[t0:t1 + 1] - b0).contiguous()
            bt = (self.block_tensor[b0:int(self.tensor_block_off[t1].item())] - t0).contiguous()
            tab = (b0, tbo, bt)
            self._range_tables[key] = tab
        return tab

    def opt_buckets(self, min_elems=2_000_000):
        """Contiguous tensor ranges for the per-bucket optimizer step, in the order the backward pass completes them:
        [(t0, t1, node)] -- node = lowest trunk node of the range (its data gradient is the last reader of the
        range's transposed weights), None for the heads (all of them, first)."""
        if getattr(self, "_opt_buckets", None) is None:
            first_head = self.head_params[0][0].index
            out = [(first_head, len(self.tensors), None)]
            hi, acc = first_head, 0
            conv_nodes = sorted(self.conv_params)
            for i in reversed(conv_nodes):
                wt, bt = self.conv_params[i]
                acc += wt.numel + bt.numel
                if acc >= min_elems or i == conv_nodes[0]:
                    out.append((wt.index, hi, i))
                    hi, acc = wt.index, 0
            self._opt_buckets = out
        return self._opt_buckets

    def _clip_scales_range(self, t0, t1, clip):
        """Tensors t0..t1-1 as (slice of the flat buffers, its elements, block -> tensor map relative to t0); unless clip is
        None, their clip_by_norm scales are computed first, on the current stream."""
        b0, tbo, bt = self._range_table(t0, t1)
        start, n = b0 * self.block, bt.numel() * self.block
        sl = slice(start, start + n)
        if clip is not None:
            _lib.check(self.L.ssd_grad_clip_scales(ops._ptr(self.grad[sl]), n, ops._ptr(tbo), t1 - t0, float(clip),
                                                   ops._ptr(self.sq_partial[b0:]), ops._ptr(self.clip_scale[t0:]),
                                                   ops._ptr(self.grad_norms[t0:]), ops._stream()))
        return sl, n, bt

    def adam_range(self, t0, t1, lr_t, beta1, beta2, eps, clip, grad_scale=1.0):
        """clip_by_norm + Adam + bf16 / transposed copies for parameter tensors t0..t1-1 on the current stream.
        Per tensor the arithmetic is that of clip_scales() + adam() over the whole flat buffer, bit for bit.
        clip=None: the gradient is already clipped (and summed over ranks): only grad_scale (1 / world) applies."""
        self._live_only("adam_range()")
        sl, n, bt = self._clip_scales_range(t0, t1, clip)
        _lib.check(self.L.ssd_adam_step(ops._ptr(self.param[sl]), ops._ptr(self.grad[sl]), ops._ptr(self.adam_m[sl]),
                                        ops._ptr(self.adam_v[sl]), ops._ptr(self.param_bf16[sl]), n, ops._ptr(bt),
                                        ops._ptr(self.clip_scale[t0:]) if clip is not None else None, float(grad_scale),
                                        float(lr_t), float(beta1), float(beta2), float(eps), ops._stream()))
        self._ema_follow(sl)
        self.slots = "adam"
        self.refresh_weights(tensors=(t0, t1))

    def decay_table(self, weight_decay, decay_bias=False):
        """Device fp32 [len(tensors)]: the L2 coefficient of every tensor for ssd_sgd_momentum_step -- weight_decay on the
        filters (names ending in "kernel"), on the biases only with decay_bias (Caffe SSD: decay_mult 0), else 0.  The l2norm
        scale ("l2norm0/scale") and the batch normalisation's gamma / beta ("bn*/gamma", "bn*/beta") count as biases: an L2 term
        only with decay_bias.
        Cached per (weight_decay, decay_bias)."""
        key = (float(weight_decay), bool(decay_bias))
        if not hasattr(self, "_decay_tables"):
            self._decay_tables = {}
        tab = self._decay_tables.get(key)
        if tab is None:
            host = [key[0] if (t.name.endswith("kernel") or key[1]) else 0.0 for t in self.tensors]
            tab = torch.tensor(host, dtype=torch.float32).to(self.device)
            self._decay_tables[key] = tab
        return tab

    def sgd_range(self, t0, t1, lr, momentum, nesterov, decay, clip, grad_scale=1.0):
        """clip_by_norm + momentum SGD + bf16 / transposed copies for parameter tensors t0..t1-1 on the current stream; the
        velocity lives in adam_m.  decay: decay_table() or None.  Per tensor the arithmetic is that of clip_scales() +
        sgd_momentum() over the whole flat buffer, bit for bit.
        clip=None: the gradient is already clipped (and summed over ranks): only grad_scale (1 / world) applies."""
        self._live_only("sgd_range()")
        sl, n, bt = self._clip_scales_range(t0, t1, clip)
        _lib.check(self.L.ssd_sgd_momentum_step(ops._ptr(self.param[sl]), ops._ptr(self.grad[sl]), ops._ptr(self.adam_m[sl]),
                                                ops._ptr(self.param_bf16[sl]), n, ops._ptr(bt),
                                                ops._ptr(self.clip_scale[t0:]) if clip is not None else None,
                                                ops._ptr(decay[t0:]) if decay is not None else None, float(grad_scale),
                                                float(lr), float(momentum), 1 if nesterov else 0, ops._stream()))
        self._ema_follow(sl)
        self.slots = "sgd_momentum"
        self.refresh_weights(tensors=(t0, t1))

    def clip_range_in_place(self, t0, t1, clip=0.01):
        """clip_by_norm of tensors t0..t1-1 (a contiguous range of the flat gradient) in place, on the current stream."""
        sl, n, bt = self._clip_scales_range(t0, t1, clip)
        _lib.check(self.L.ssd_grad_apply_scale(ops._ptr(self.grad[sl]), n, ops._ptr(bt), ops._ptr(self.clip_scale[t0:]),
                                               ops._stream()))

    def accumulate_clipped(self, first):
        if self.grad_acc is None:
            self.grad_acc = torch.empty_like(self.grad)
        _lib.check(self.L.ssd_grad_accumulate(ops._ptr(self.grad_acc), ops._ptr(self.grad), self.n_flat,
                                              ops._ptr(self.block_tensor), ops._ptr(self.clip_scale), 1 if first else 0,
                                              ops._stream()))

    def adam(self, lr, grad, grad_scale=1.0, use_clip_scale=False, beta1=0.9, beta2=0.999, eps=1e-7):
        self._live_only("adam()")
        self.step_count += 1
        t = self.step_count
        lr_t = lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        _lib.check(self.L.ssd_adam_step(ops._ptr(self.param), ops._ptr(grad), ops._ptr(self.adam_m), ops._ptr(self.adam_v),
                                        ops._ptr(self.param_bf16), self.n_flat, ops._ptr(self.block_tensor),
                                        ops._ptr(self.clip_scale) if use_clip_scale else None, float(grad_scale),
                                        float(lr_t), float(beta1), float(beta2), float(eps), ops._stream()))
        self._ema_follow()
        self.slots = "adam"
        self.refresh_weights()

    def sgd_momentum(self, lr, grad, grad_scale=1.0, use_clip_scale=False, momentum=0.9, nesterov=False, decay=None):
        """Momentum SGD over the whole flat buffer (ssd_sgd_momentum_step); the velocity lives in adam_m, adam_v is untouched.
        decay: decay_table() or None."""
        self._live_only("sgd_momentum()")
        self.step_count += 1
        _lib.check(self.L.ssd_sgd_momentum_step(ops._ptr(self.param), ops._ptr(grad), ops._ptr(self.adam_m),
                                                ops._ptr(self.param_bf16), self.n_flat, ops._ptr(self.block_tensor),
                                                ops._ptr(self.clip_scale) if use_clip_scale else None,
                                                ops._ptr(decay) if decay is not None else None, float(grad_scale), float(lr),
                                                float(momentum), 1 if nesterov else 0, ops._stream()))
        self._ema_follow()
        self.slots = "sgd_momentum"
        self.refresh_weights()

    def sgd(self, lr, grad, grad_scale=1.0, use_clip_scale=False):
        self._live_only("sgd()")
        self.step_count += 1
        _lib.check(self.L.ssd_sgd_step(ops._ptr(self.param), ops._ptr(grad), ops._ptr(self.param_bf16), self.n_flat,
                                       ops._ptr(self.block_tensor), ops._ptr(self.clip_scale) if use_clip_scale else None,
                                       float(grad_scale), float(lr), ops._stream()))
        self._ema_follow()
        self.refresh_weights()

    # ---------------------------------------------------------------- averaged weights
    def enable_ema(self):
        """Keep an exponential moving average of the flat parameter buffer (no reference counterpart): `ema`, fp32 [n_flat],
        starts as a bit-for-bit copy of param (ssd_ema_step with factor 1) and ema_updates at 0; called again it restarts the
        average from the current weights.  From then on every optimizer launch (adam_range / sgd_range per bucket, adam /
        sgd_momentum / sgd over the whole buffer) is followed, on its stream, by one ssd_ema_step over the slice it wrote with
        the factor ema_om = 1 - decay -- while ema_om is None, and on an engine without the average, by nothing.  The caller
        owns the schedule: it sets ema_om before an optimizer step and counts ema_updates after it (the model does, from
        ops.EmaSpec).  The average never feeds back into param or the optimizer slots."""
        self._live_only("enable_ema()")
        if self.ema is None:
            self.ema = torch.empty_like(self.param)
        ops.ema_step(self.ema, self.param, 1.0)
        self.ema_updates, self.ema_om = 0, None

    def _ema_follow(self, sl=None):
        """Behind an optimizer launch over param[sl] (None: the whole buffer), on the same stream: the average of that slice."""
        if self.ema is None or self.ema_om is None:
            return
        e, p = (self.ema, self.param) if sl is None else (self.ema[sl], self.param[sl])
        _lib.check(self.L.ssd_ema_step(ops._ptr(e), ops._ptr(p), p.numel(), float(self.ema_om), ops._stream()))

    def _live_only(self, what):
        if self._averaged:
            raise RuntimeError("%s inside `with averaged():` -- the forward paths read the averaged weights there; training and "
                               "checkpoints work on the live ones" % what)

    @contextlib.contextmanager
    def averaged(self):
        """`with eng.averaged():` -- every forward path reads the averaged weights: param and ema change places, the bf16 copy,
        the transposed and fragment-packed copies are rebuilt from the average (refresh_weights(cast=True)) and so is the fp8
        operand store where one is allocated; on exit the two change back and the copies are rebuilt from the live weights,
        bit for bit what they were (each copy is a function of param alone).  On the current stream.  Inside, backward(), the
        optimizer methods, enable_ema() and state_dict() / load_state_dict() raise RuntimeError, and so does a nested block.
        ValueError on an engine without the average.
        Only the flat buffer is averaged.  A batchnorm engine's gamma and beta live in it and are averaged with it; its
        running mean and variance are not -- the averaged network normalises with the live running statistics."""
        if self.ema is None:
            raise ValueError("averaged() on an engine without an average: call enable_ema() first")
        self._live_only("averaged()")
        self._swap_average(True)
        try:
            yield self
        finally:
            self._swap_average(False)

    def _swap_average(self, on):
        self.param, self.ema = self.ema, self.param
        self._averaged = on
        self.refresh_weights(cast=True)
        if self.mx_filters.allocated:                          # an fp8 forward has run: its operand store follows param_bf16
            self._quantize_filters()

    # ---------------------------------------------------------------- state
    LAYOUT_VERSION = 2                         # 2: a level's loc / conf filters are separate variables (64 tensors for SSD300)

    def state_dict(self):
        """The flat buffers, the step count and the layout they belong to; `ema` and `ema_updates` besides on an engine that
        keeps the average (enable_ema), and only there: a plain engine's keys are what they were."""
        self._live_only("state_dict()")
        sd = dict(param=self.param.cpu(), adam_m=self.adam_m.cpu(), adam_v=self.adam_v.cpu(), step=self.step_count,
                  names=[t.name for t in self.tensors], shapes=[t.shape for t in self.tensors],
                  offsets=[t.offset for t in self.tensors], layout_version=self.LAYOUT_VERSION, slots=self.slots)
        if self.ema is not None:
            sd.update(ema=self.ema.cpu(), ema_updates=self.ema_updates)
        return sd

    def load_state_dict(self, sd):
        """The flat buffers are only meaningful together with the layout they were saved under: names, shapes and offsets of
        every variable must match this engine's (another class count, block size or an older fused-head layout would
        otherwise load misaligned weights silently where the sizes happen to coincide)."""
        self._live_only("load_state_dict()")
        mine = ([t.name for t in self.tensors], [tuple(t.shape) for t in self.tensors], [t.offset for t in self.tensors])
        theirs = (list(sd.get("names", [])), [tuple(x) for x in sd.get("shapes", [])], list(sd.get("offsets", [])))
        if sd.get("layout_version", 1) != self.LAYOUT_VERSION or mine != theirs or sd["param"].numel() != self.n_flat:
            bad = [n for n in mine[0] if n not in theirs[0]][:3] + [n for n in theirs[0] if n not in mine[0]][:3]
            raise ValueError("checkpoint parameter layout (version %s, %d variables, %d elements) does not match this engine's "
                             "(version %d, %d variables, %d elements)%s" % (
                                 sd.get("layout_version", 1), len(theirs[0]), sd["param"].numel(), self.LAYOUT_VERSION,
                                 len(mine[0]), self.n_flat, "; e.g. " + ", ".join(bad) if bad else ""))
        slots = sd.get("slots", "adam")                # what adam_m holds; checkpoints from before the key: Adam's moments
        if slots not in ("adam", "sgd_momentum"):
            raise ValueError("checkpoint optimizer slots %r: expected 'adam' or 'sgd_momentum'" % (slots,))
        self.param.copy_(sd["param"])
        self.adam_m.copy_(sd["adam_m"])
        self.adam_v.copy_(sd["adam_v"])
        self.step_count = int(sd["step"])
        self.slots = slots
        self.refresh_weights(cast=True)
        # the average: taken where this engine keeps one and the checkpoint has it; restarted from the loaded weights where the
        # checkpoint has none; ignored by an engine that keeps none
        if self.ema is not None and "ema" in sd:
            self.ema.copy_(sd["ema"])
            self.ema_updates = int(sd.get("ema_updates", 0))
        elif self.ema is not None:
            logger.info("checkpoint holds no averaged weights: the average restarts from the loaded parameters")
            self.enable_ema()
