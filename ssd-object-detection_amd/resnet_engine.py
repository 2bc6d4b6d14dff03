"""SSD512 with a ResNet-50 trunk on the gfx950 library -- BASELINE configs[4]'s network ("SSD512 ResNet-50 backbone ... 8732 ->
24564 anchors").  The reference has no counterpart: it hard-codes the 300 x 300 VGG network (models/ssd_model.py:46, 75-97), so
parity here is against this build's own plain-PyTorch restatement (oracle/net_oracle.py:forward_graph), not against the
reference.

Network: ResNet-50 v1.5 through conv4_x with frozen batch normalisation FOLDED into the convolutions (scale into the filters,
shift into the bias: every convolution is conv + bias, trainable) -- 7x7/2 stem, 3x3/2 max pooling, bottlenecks 1x1 -> 3x3
(stride on the 3x3) -> 1x1 with a projection shortcut where the shape changes, Add + ReLU -- feature maps conv3_x (64 x 64 x
512) and conv4_x (32 x 32 x 1024) at a 512 x 512 input, then the SSD recipe's extra stages (1x1 -> 3x3/2) down to 1 x 1: seven
levels 64, 32, 16, 8, 4, 2, 1 with 4, 6, 6, 6, 6, 4, 4 default boxes per cell = 24 564 anchors, heads as in the reference
(:153-162).  TF "SAME" padding everywhere (Keras semantics, as the rest of the engine).

Opt-in (batchnorm=...): LIVE batch normalisation behind each of the 43 trunk convolutions (csrc/batchnorm.hip), to train the
trunk from scratch; fold_batchnorm_params / engine.folded() turn the trained network into the folded one above.

The network is a DAG (residual adds), so forward / backward are a plain topological walk on ONE stream over the same C-ABI
entry points SSDEngine uses (1x1 layers on k_pw_gemm, 3x3 layers on the LDS-patch kernels, strided layers on the implicit-GEMM
kernels, heads' backward from the loss's compact rows) plus csrc/eltwise.hip (Add + ReLU, its gradient, 3x3/2 pooling).
Parameter storage, clip + Adam, checkpoints: inherited."""
import torch

from . import _lib, mx, ops
from .engine import SSDEngine, SSD512_NUM_PRIORS, mxfp8_eligible


def resnet50_ssd512_graph(batchnorm=False):
    """Topologically ordered nodes: dict(op, src, cin, cout, k, stride, relu, feature).  src = producing node index
    (-1: the network input), for "add": (block output, shortcut).  batchnorm=True: each of the 43 trunk convolutions (stem,
    39 bottleneck convolutions, 3 projections) is followed by a node op="bn" with src = that convolution, which carries the
    convolution's ReLU flag (the convolution's own becomes False); consumers and adds read the bn node.  The ten extras stay
    conv + bias + ReLU."""
    g = []

    def plain(src, cin, cout, k, stride, relu=True, feature=False):
        g.append(dict(op="conv", src=src, cin=cin, cout=cout, k=k, stride=stride, relu=relu, feature=feature))
        return len(g) - 1

    def normed(src, cin, cout, k, stride, relu=True):
        c = plain(src, cin, cout, k, stride, relu=False)
        g.append(dict(op="bn", src=c, cin=cout, cout=cout, k=1, stride=1, relu=relu, feature=False))
        return len(g) - 1

    conv = normed if batchnorm else plain
    x = conv(-1, 8, 64, 7, 2)                                  # stem (image carried in 8 zero-padded channels)
    g.append(dict(op="pool3", src=x, cin=64, cout=64, k=3, stride=2, relu=False, feature=False))
    x, cin = len(g) - 1, 64
    for width, blocks, stride, feat in ((64, 3, 1, False), (128, 4, 2, True), (256, 6, 2, True)):     # conv2_x .. conv4_x
        for b in range(blocks):
            s = stride if b == 0 else 1
            a = conv(x, cin, width, 1, 1)
            a = conv(a, width, width, 3, s)                     # v1.5: the stride sits on the 3x3
            a = conv(a, width, 4 * width, 1, 1, relu=False)
            sc = conv(x, cin, 4 * width, 1, s, relu=False) if (b == 0) else x      # projection shortcut where the shape changes
            g.append(dict(op="add", src=(a, sc), cin=4 * width, cout=4 * width, k=0, stride=1, relu=True,
                          feature=feat and b == blocks - 1))
            x, cin = len(g) - 1, 4 * width
    for mid, out in ((256, 512), (128, 256), (128, 256), (128, 256), (128, 256)):   # extras: 32 -> 16 -> 8 -> 4 -> 2 -> 1
        x = plain(x, cin, mid, 1, 1)
        x = plain(x, mid, out, 3, 2, feature=True)
        cin = out
    return g


def _kind(nd):
    return nd.get("kind", nd.get("op"))           # planned node (engine.nodes) or graph node (resnet50_ssd512_graph)


def mxfp8_plan(nodes, train=False):
    """The fp8 forward of a graph (resnet50_ssd512_graph() or the engine's planned nodes; no device needed).  Returns
    (fp8, writes): the set of nodes that run in fp8, and for every node the outputs it writes, a frozenset of "bf16" / "fp8".
    A producer writes exactly what its consumers read: "fp8" for an fp8 convolution, "bf16" for a bf16 convolution, the
    pooling, an add and the heads (feature maps); adds always write bf16 (ops.add_relu_fwd_mxfp8 adds the fp8 form).  Every
    fp8 map is written by the epilogue of its producer (an fp8 convolution or an add): the plan needs no standalone
    quantisation of an activation.  train=True: the training-mode forward, whose producers also write the bf16 map of every
    node backward() reads -- each convolution's input (its weight gradient; it is also every ReLU mask a data gradient
    applies) besides the adds (identity-shortcut masks) and the feature maps (heads), which write it anyway."""
    fp8 = {i for i, nd in enumerate(nodes) if mxfp8_eligible(nd) and nd["src"] >= 0}     # (>= 0: not the stem)
    writes = {i: set() for i in range(len(nodes))}
    for i, nd in enumerate(nodes):
        if nd["feature"] or _kind(nd) == "add":
            writes[i].add("bf16")
        for s in (nd["src"] if _kind(nd) == "add" else (nd["src"],)):
            if s >= 0:
                writes[s].add("fp8" if i in fp8 else "bf16")
                if train and _kind(nd) == "conv":
                    writes[s].add("bf16")
    for i, w in writes.items():
        assert w, "node %d has no consumer" % i
        if "fp8" in w:
            assert i in fp8 or _kind(nodes[i]) == "add", "node %d would need a standalone activation quantise" % i
    assert all(nodes[i]["src"] >= 0 for i in fp8), "the network input would need a standalone quantise"
    return fp8, {i: frozenset(w) for i, w in writes.items()}


def mxfp8_dgrad_eligible(nd):
    """Whether the data gradient of node `nd` runs in block-scaled fp8 (ops.conv2d_bwd_data_mxfp8): a convolution other than
    the stem, stride 1, k in (1, 3), whose output channels (the K of this GEMM) are whole MX k-steps (Cout % 128 == 0) and
    whose input channels are whole MX blocks (Cin % 32 == 0)."""
    src = nd["src"]
    return (_kind(nd) == "conv" and isinstance(src, int) and src >= 0 and nd["stride"] == 1 and nd["k"] in (1, 3)
            and nd["cout"] % 128 == 0 and nd["cin"] % 32 == 0)


def mxfp8_bwd_plan(nodes):
    """The fp8 data gradients after a training-mode fp8 forward (no device needed).  Returns (dgrad, root, maps):
      dgrad  the set of convolutions whose data gradient runs in fp8 (mxfp8_dgrad_eligible);
      root   {node: the node whose gradient buffer it shares}: the two linear inputs of an add (the block's 1x1 expand and a
             projection shortcut) alias the add's gradient, every other node owns its own;
      maps   {root r: (kind, writer)} for every gradient map an fp8 data gradient reads as dy: the LAST launch of the reverse
             walk that writes it, which also writes its fp8 form.  kind "fp8" = fp8 data gradient `writer`, whose epilogue
             quantises; "dgrad" (a bf16 stride-2 data gradient), "pool", "relu_mask" (identity shortcut of add `writer`) or
             "heads" (writer -1) = a bf16 kernel, behind which ONE standalone ops.quantize_mx_fp8 of the map runs.
    Writers of a map, in walk order: the heads' data gradient (feature maps), then its consumers from the last to the first."""
    n = len(nodes)
    dgrad = {i for i, nd in enumerate(nodes) if mxfp8_dgrad_eligible(nd)}
    root = list(range(n))
    for k in range(n - 1, -1, -1):
        if _kind(nodes[k]) == "add":
            a, sc = nodes[k]["src"]
            root[a] = root[k]
            if _kind(nodes[sc]) == "conv" and not nodes[sc]["relu"]:
                root[sc] = root[k]
    writers = {r: ([("heads", -1)] if nodes[r]["feature"] else []) for r in range(n)}
    for c in range(n - 1, -1, -1):
        nd = nodes[c]
        if _kind(nd) == "add":
            a, sc = nd["src"]
            assert root[a] != a, "the block output of add %d is not linear" % c
            if root[sc] == sc:
                writers[sc].append(("relu_mask", c))
        elif nd["src"] >= 0:
            assert root[nd["src"]] == nd["src"], "node %d reads an aliased map" % c
            kind = "pool" if _kind(nd) == "pool3" else ("fp8" if c in dgrad else "dgrad")
            writers[nd["src"]].append((kind, c))
    maps = {}
    for i in sorted(dgrad):
        r = root[i]
        assert writers[r], "gradient map %d has no writer" % r
        maps[r] = writers[r][-1]
        assert maps[r][1] == -1 or maps[r][1] > i, "the fp8 form of map %d would come after its reader %d" % (r, i)
    return dgrad, root, maps


def fold_batchnorm_params(graph_bn, params, running, eps):
    """The parameters of the default (folded) network that computes what the batch-normalised one computes in inference mode.
    Pure: no device, no engine; works on any {name: tensor} dict (CPU, any float dtype).  graph_bn:
    resnet50_ssd512_graph(batchnorm=True); params: conv{i}/kernel [Cout,k,k,Cin], conv{i}/bias, bn{i}/gamma, bn{i}/beta by
    node index of graph_bn, head*/...; running: (running_mean, running_var), each ONE flat tensor over the bn nodes in node
    order (the engine's bn_running_mean / bn_running_var).  With a = gamma / sqrt(running_var + eps) per output channel:
        w' = w a[cout]        b' = (b - running_mean) a + beta
    The k-th convolution of graph_bn becomes conv{k'}, k' = the node index of the k-th convolution of the default graph; a
    convolution without a bn node behind it (the extras) and the heads are copied."""
    rm, rv = running
    bn_of, off = {}, 0
    for i, nd in enumerate(graph_bn):
        if nd["op"] == "bn":
            bn_of[nd["src"]] = (i, off)
            off += nd["cout"]
    assert rm.numel() == off and rv.numel() == off, (rm.numel(), rv.numel(), off)
    convs_bn = [i for i, nd in enumerate(graph_bn) if nd["op"] == "conv"]
    convs = [i for i, nd in enumerate(resnet50_ssd512_graph()) if nd["op"] == "conv"]
    assert len(convs_bn) == len(convs)
    out = {n: t for n, t in params.items() if n.startswith("head")}
    for i, k in zip(convs_bn, convs):
        w, b = params["conv%d/kernel" % i], params["conv%d/bias" % i]
        if i in bn_of:
            j, o = bn_of[i]
            c = graph_bn[i]["cout"]
            a = params["bn%d/gamma" % j] / torch.sqrt(rv[o:o + c].to(w.dtype) + eps)
            w = w * a.view(-1, 1, 1, 1)
            b = (b - rm[o:o + c].to(b.dtype)) * a + params["bn%d/beta" % j]
        out["conv%d/kernel" % k], out["conv%d/bias" % k] = w, b
    return out


class ResNet50SSDEngine(SSDEngine):
    bucket_optimizer = False                   # one-stream DAG walk: backward() refuses fused_adam / on_dgrad
    side_streams = False                       # ... and nothing runs beside it that a high-priority main stream could overtake

    def __init__(self, classes=81, in_size=512, device="cuda", seed=0, batchnorm=None):
        """batchnorm: live batch normalisation behind each trunk convolution (ops.BatchNormSpec.of: None / False = off, the
        folded network of the module docstring; True, a dict(momentum, eps) or a spec).  Off, the engine plans the same
        graph and tensors and launches what it did without the option.  On: the graph of resnet50_ssd512_graph(True); 86
        more variables "bn{i}/gamma" (1) and "bn{i}/beta" (0), i the bn node's index, behind every other one, trained, clipped
        and saved like the rest; the running mean / variance are plain fp32 buffers (bn_running_mean / bn_running_var, one flat
        tensor each in bn-node order, no optimizer variables).  forward(x, train=True) normalises with the batch's statistics
        and updates the running ones, forward(x) uses the running ones; the block-scaled fp8 paths rest on producer epilogues
        and refuse a batchnorm engine: fold first (folded()).  The bias of a normalised convolution stays in the table (it is
        zero and its gradient slot is never written: batch normalisation cancels it).  The statistics are those of THIS
        process's batch: under data parallelism every rank normalises with its own (no synchronised batch norm); the running
        buffers are per rank too."""
        self.batchnorm = ops.BatchNormSpec.of(batchnorm)
        self.graph = resnet50_ssd512_graph(batchnorm=self.batchnorm is not None)
        super().__init__(classes=classes, in_size=in_size, trunk=[], num_priors=SSD512_NUM_PRIORS, device=device, seed=seed,
                         sparse_heads=True)
        self.relu_bits = None                  # ReLU masks from the bf16 activations (the sign-byte forms are a VGG-chain fusion)
        self.overlap_heads = False
        self._bn_train = False                 # the last forward of a batchnorm engine used (and saved) batch statistics
        self._ws_bn = ops.MatchWorkspace()     # slab partials of the batch normalisation kernels

    # ---------------------------------------------------------------- static planning
    @classmethod
    def planned(cls, classes=81, in_size=512, batchnorm=None):
        """The static plan alone -- graph, nodes, grids, A, tensors (names, indices, blocks) -- without a device: nothing is
        allocated or launched.  For what needs the layout only: decay_table(), ready_order(), bucket plans."""
        eng = cls.__new__(cls)
        eng.batchnorm = ops.BatchNormSpec.of(batchnorm)
        eng.graph = resnet50_ssd512_graph(batchnorm=eng.batchnorm is not None)
        eng._plan(classes, in_size, [], SSD512_NUM_PRIORS, "cpu", None, True)
        return eng

    def ready_order(self):
        """The tensor indices backward() hands to on_ready, call by call: the trunk from the last node to the first (a bn
        node's gamma / beta, a convolution's kernel / bias), then every head at once.  The flat buffer is therefore NOT
        completed from its end -- the heads sit behind the trunk and are reported last, a batchnorm engine's gamma / beta sit
        behind the heads and are reported throughout -- which parallel.GradReducer tolerates: it launches a bucket only once
        every tensor of it was reported, buckets in order, so here the exchange starts when the pass ends."""
        calls = []
        for i in range(len(self.nodes) - 1, -1, -1):
            if i in self.bn_params:
                calls.append([t.index for t in self.bn_params[i]])
            elif i in self.conv_params:
                calls.append([t.index for t in self.conv_params[i]])
        calls.append([i for wt, bt in self.head_params for t in (wt, bt) for i in t.indices])
        return calls

    def _plan_extra_params(self, add):
        self.bn_params, self.bn_off, off = {}, {}, 0          # bn node -> (gamma, beta); -> offset in the flat statistics
        for i, nd in enumerate(self.nodes):
            if nd["kind"] == "bn":
                self.bn_params[i] = (add("bn%d/gamma" % i, (nd["cout"],)), add("bn%d/beta" % i, (nd["cout"],)))
                self.bn_off[i] = off
                off += nd["cout"]
        self.bn_channels = off
        self.bn_convs = {self.nodes[i]["src"] for i in self.bn_params}      # the normalised convolutions

    def _plan_params(self):
        super()._plan_params()
        # the fp8 plans (a batchnorm engine has none: forward(x, "mxfp8") refuses)
        n, bn = len(self.nodes), self.batchnorm is not None
        self.mx_fp8, self.mx_writes = (set(), {}) if bn else mxfp8_plan(self.nodes)
        self.mx_train_writes = {} if bn else mxfp8_plan(self.nodes, train=True)[1]
        self.mx_dgrad, self.mx_groot, self.mx_gmaps = (set(), list(range(n)), {}) if bn else mxfp8_bwd_plan(self.nodes)
        # mx_filters quantises the trunk's part of param_bf16 (conv filters start on optimizer-block boundaries, multiples of
        # 32 elements, so each layer's (q, scale) is a slice of it)
        self._mx_range = (0, max(bt.block0 + bt.nblocks for _, bt in self.conv_params.values()) * self.block)
        # the transposed filters as slices of ONE buffer, the fp8 data gradients' first: mx_filters_t quantises its front
        # (every slice starts on a 32-element block: Cout % 32 == 0 for all of them)
        self.wt_off, self.n_wt8, off = {}, 0, 0               # node -> offset in the flat buffer; the fp8 front; n_wt in all
        for i in sorted((i for i in self.conv_params if i > 0), key=lambda i: (i not in self.mx_dgrad, i)):
            self.wt_off[i] = off
            off += self.conv_params[i][0].numel
            assert off % 32 == 0
            if i in self.mx_dgrad:
                self.n_wt8 = off
        self.n_wt = off
        self.mx_filters_t = mx.FlatStore()

    def _alloc_params(self):
        super()._alloc_params()
        if self.batchnorm is not None:
            dev, n = self.device, self.bn_channels
            self.bn_running_mean = torch.zeros(n, dtype=torch.float32, device=dev)
            self.bn_running_var = torch.ones(n, dtype=torch.float32, device=dev)
            self._bn_mean = torch.empty(n, dtype=torch.float32, device=dev)        # the batch's, saved by forward(train=True)
            self._bn_rstd = torch.empty(n, dtype=torch.float32, device=dev)
            # where conv2d_bwd_weight puts the bias gradient of a normalised convolution: never read (the true gradient is 0)
            self._bn_dbias = torch.empty(max(nd["cout"] for nd in self.nodes), dtype=torch.float32, device=dev)
        flat = torch.empty(self.n_wt, dtype=torch.bfloat16, device=self.device)
        for i, off in self.wt_off.items():
            self.w_t[i] = flat[off:off + self.w_t[i].numel()].view(self.w_t[i].shape)
        self._wt_flat = flat

    def init_params(self, seed=0):
        """As SSDEngine.init_params; a batchnorm engine's gammas start at 1 (betas at 0), its running statistics at (0, 1)."""
        super().init_params(seed)
        if self.batchnorm is not None:
            for gamma, _ in self.bn_params.values():
                self.view(gamma, self.param).fill_(1.0)
            self.bn_running_mean.zero_()
            self.bn_running_var.fill_(1.0)
            self.refresh_weights(cast=True)

    def _bn_stat(self, i, buf):
        o = self.bn_off[i]
        return buf[o:o + self.nodes[i]["cout"]]

    def _plan_shapes(self):
        self.nodes, self.fm = [], []
        sizes = {-1: self.in_size}
        for i, nd in enumerate(self.graph):
            src = nd["src"][0] if nd["op"] == "add" else nd["src"]
            hin = sizes[src]
            if nd["op"] == "add":
                ho, pt = hin, 0
            else:
                ho, pt = ops.same_pad(hin, nd["k"], nd["stride"])
            sizes[i] = ho
            kind = "conv" if nd["op"] == "conv" else nd["op"]
            self.nodes.append(dict(kind=kind, cin=nd["cin"], cout=nd["cout"], k=nd["k"], stride=nd["stride"], pt=pt, pl=pt, hin=hin,
                                   hout=ho, feature=nd["feature"], same=True, src=nd["src"], relu=nd["relu"]))
            if nd["feature"]:
                self.fm.append((i, ho, nd["cout"]))
        assert len(self.fm) == len(self.num_priors), (len(self.fm), len(self.num_priors))
        self.level_off = [0]
        for (_, h, _), n in zip(self.fm, self.num_priors):
            self.level_off.append(self.level_off[-1] + h * h * n)
        self.A = self.level_off[-1]
        self.grids = tuple((h, h) for _, h, _ in self.fm)

    def _acts(self, B):
        c = self._act_cache.get(B)
        if c is None:
            c = super()._acts(B)
            dev = self.device
            c["pool3_code"] = {i: torch.empty((B, nd["hout"], nd["hout"], nd["cout"] // 8), dtype=torch.int32, device=dev)
                               for i, nd in enumerate(self.nodes) if nd["kind"] == "pool3"}
        return c

    def _mx_act_writes(self):
        return self.mx_writes

    def mxfp8_grads(self, B):
        """{root map: (q u8 [B,H,W,C], scale u8 [B,H,W,C/32])}: the fp8 forms of the gradient maps the fp8 data gradients read
        (mxfp8_bwd_plan), allocated at the first fp8 backward of batch size B."""
        return self._mx_pairs(B, "mxfp8_grad", self.mx_gmaps)

    def mxfp8_wt(self, i):
        """(q [Cin,k,k,Cout], scale [Cin,k,k,Cout/32]) of the transposed filters of fp8 data gradient i as the last fp8
        backward quantised them."""
        cout, k, _, cin = self.conv_params[i][0].shape
        return self.mx_filters_t.view(self.wt_off[i], (cin, k, k, cout))

    def _quantize_wt(self):
        self.mx_filters_t.quantize(self._wt_flat[:self.n_wt8])

    def _in(self, acts, src):
        return acts[src + 1]                   # acts[0] = network input, acts[i + 1] = output of node i

    # ---------------------------------------------------------------- forward / backward
    def forward(self, x, precision="bf16", train=False):
        """(loc, conf) of image batch x.  precision="mxfp8": the trunk's fp8 layers (mxfp8_plan) on block-scaled fp8
        operands, each fed directly by the layer before it; the rest and the heads in bf16.  Inference only unless
        train=True, which also writes every bf16 map backward() reads (same fp8 launches, same (loc, conf)); backward()
        then runs the stride-1 data gradients in fp8 (mxfp8_bwd_plan).
        A batchnorm engine (bf16 only): train=True normalises with the batch's statistics, saves them for backward() and
        updates the running ones; train=False normalises with the running ones."""
        if precision == "mxfp8":
            if self.batchnorm is not None:
                raise ValueError("forward(x, 'mxfp8') on a batchnorm engine: the fp8 plan rests on producer epilogues; fold "
                                 "the trained network first (folded()) and run that engine in fp8")
        elif precision != "bf16":
            raise ValueError("precision must be 'bf16' or 'mxfp8', not %r" % (precision,))
        fp8 = precision == "mxfp8"
        B = x.shape[0]
        c = self._acts(B)
        acts = c["acts"]
        acts[0] = x
        self.bits_valid = set()
        self.last_forward = ("mxfp8_train" if train else "mxfp8") if fp8 else "bf16"
        self._bn_train = self.batchnorm is not None and bool(train)
        maps8 = writes = None                  # bf16: no node writes an fp8 form and no convolution reads one
        if fp8:
            maps8, writes = self.mxfp8_acts(B), self.mx_train_writes if train else self.mx_writes
            self._quantize_filters()
        for i, nd in enumerate(self.nodes):
            w = writes[i] if fp8 else ()
            if nd["kind"] == "conv":
                wt, bt = self.conv_params[i]
                if fp8 and i in self.mx_fp8:
                    xq, xs = maps8[nd["src"]]
                    wq, ws = self.mxfp8_weights(i)
                    q, sc = maps8.get(i, (None, None))
                    ops.conv2d_fwd_mxfp8(xq, xs, wq, ws, self.view(bt, self.param), nd["stride"], nd["pt"], nd["pl"], nd["hout"],
                                         nd["hout"], nd["relu"], want_bf16="bf16" in w, want_fp8="fp8" in w, out=acts[i + 1],
                                         out_q=q, out_scale=sc)
                else:
                    ops.conv2d_fwd(self._in(acts, nd["src"]), self.view(wt, self.param_bf16), self.view(bt, self.param),
                                   nd["stride"], nd["pt"], nd["pl"], nd["hout"], nd["hout"], nd["relu"], out=acts[i + 1], ws=self._ws)
            elif nd["kind"] == "bn":
                gamma, beta = (self.view(t, self.param) for t in self.bn_params[i])
                rm, rv = self._bn_stat(i, self.bn_running_mean), self._bn_stat(i, self.bn_running_var)
                if self._bn_train:
                    ops.batchnorm_fwd_train(self._in(acts, nd["src"]), gamma, beta, out=acts[i + 1],
                                            mean=self._bn_stat(i, self._bn_mean), rstd=self._bn_stat(i, self._bn_rstd),
                                            running_mean=rm, running_var=rv, momentum=self.batchnorm.momentum,
                                            eps=self.batchnorm.eps, relu=nd["relu"], ws=self._ws_bn)
                else:
                    ops.batchnorm_fwd_infer(self._in(acts, nd["src"]), gamma, beta, rm, rv, out=acts[i + 1],
                                            eps=self.batchnorm.eps, relu=nd["relu"])
            elif nd["kind"] == "pool3":
                ops.maxpool3x3s2_fwd(self._in(acts, nd["src"]), out=acts[i + 1], code=c["pool3_code"][i])
            else:
                a, sc = nd["src"]
                if "fp8" in w:
                    ops.add_relu_fwd_mxfp8(acts[a + 1], acts[sc + 1], out=acts[i + 1], q=maps8[i][0], scale=maps8[i][1])
                else:
                    ops.add_relu_fwd(acts[a + 1], acts[sc + 1], out=acts[i + 1])
        for lvl in range(len(self.fm)):
            self._head_fwd(lvl, c, self._ws)
        return c["loc"], c["conf"]

    def backward(self, dloc, dconf, on_ready=None, fused_adam=None, heads=None, on_dgrad=None, dgrad_precision=None):
        """Gradients of all parameters into self.grad from d(loss)/d(loc), d(loss)/d(conf) (or the loss's compact rows).
        After forward(x, "mxfp8", train=True) the data gradients of mxfp8_bwd_plan run in block-scaled fp8 (their
        transposed filters quantised here, once per call); dgrad_precision="bf16" keeps every data gradient in bf16.  Weight
        gradients, heads, stride-2 data gradients and pooling always run in bf16 on the bf16 maps."""
        assert fused_adam is None and on_dgrad is None, "the per-bucket optimizer schedule belongs to the VGG chain engine"
        self._live_only("backward()")
        if self.last_forward == "mxfp8":
            raise RuntimeError("backward() after an inference mxfp8 forward: the bf16 activations it needs were not all "
                               "written; run forward(x) in bf16 or forward(x, 'mxfp8', train=True) first")
        if self.batchnorm is not None and not self._bn_train:
            raise RuntimeError("backward() after an inference-mode forward of a batchnorm engine: no batch statistics were "
                               "saved; run forward(x, train=True) first")
        if dgrad_precision not in (None, "bf16", "mxfp8"):
            raise ValueError("dgrad_precision must be 'bf16' or 'mxfp8', not %r" % (dgrad_precision,))
        if dgrad_precision == "mxfp8" and self.last_forward != "mxfp8_train":
            raise ValueError("fp8 data gradients need a forward(x, 'mxfp8', train=True) first")
        fp8 = self.last_forward == "mxfp8_train" and dgrad_precision != "bf16"
        if heads is None:
            heads = self.heads_from_dense(dloc, dconf)
        c = self._acts(heads.B)
        acts, gacts = c["acts"], list(c["gacts"])
        if fp8:
            self._quantize_wt()
            g8 = self.mxfp8_grads(heads.B)

        def wrote(r, kind, writer):            # a bf16 kernel was the last writer of a map an fp8 data gradient reads
            if fp8 and self.mx_gmaps.get(r) == (kind, writer):
                ops.quantize_mx_fp8(c["gacts"][r + 1], q=g8[r][0], scale=g8[r][1])

        n = len(self.nodes)
        written = [False] * (n + 1)
        # heads: every feature-map gradient is written (masked by the map's own ReLU), then the trunk accumulates onto it
        hl, keep = self._head_layers(c)
        ops.heads_bwd_weight_sparse(heads, hl, ws=self._ws_hw)
        ops.heads_bwd_data_sparse(heads, hl, ws=self._ws_hz)
        del keep
        for ni, _, _ in self.fm:
            written[ni + 1] = True
            wrote(ni, "heads", -1)

        def relu_of(idx):                      # does activation acts[idx] carry its own ReLU?
            return idx > 0 and self.nodes[idx - 1]["relu"]

        for i in range(n - 1, -1, -1):
            nd = self.nodes[i]
            g = gacts[i + 1]
            assert written[i + 1], (i, nd)
            if nd["kind"] == "add":
                a, sc = nd["src"]
                # g = d loss / d relu(a + sc), already masked by this node's ReLU (its consumers' data gradients did that).
                # The block output (a linear 1x1 convolution) takes it as it is: alias, no copy.
                assert not written[a + 1] and not self.nodes[a]["relu"]
                gacts[a + 1] = g
                written[a + 1] = True
                if self.nodes[sc]["kind"] in ("conv", "bn") and not self.nodes[sc]["relu"]:      # projection shortcut: linear too
                    assert not written[sc + 1]
                    gacts[sc + 1] = g
                else:                           # identity shortcut: masked by the source's own ReLU, summed with its other uses
                    ops.relu_mask_bwd(g, acts[sc + 1], out=gacts[sc + 1], accumulate=written[sc + 1])
                    wrote(sc, "relu_mask", i)
                written[sc + 1] = True
                continue
            src = nd["src"]
            if nd["kind"] == "pool3":
                assert not written[src + 1]
                ops.maxpool3x3s2_bwd(c["pool3_code"][i], g, acts[src + 1].shape, out=gacts[src + 1])
                wrote(src, "pool", i)
                written[src + 1] = True
                continue
            if nd["kind"] == "bn":
                # g is masked by this node's own ReLU already (its consumers' data gradients did that); xh is rebuilt from the
                # convolution's output and the statistics the forward pass saved
                assert not written[src + 1]
                gamma, beta = self.bn_params[i]
                ops.batchnorm_bwd(g, acts[src + 1], self.view(gamma, self.param), self._bn_stat(i, self._bn_mean),
                                  self._bn_stat(i, self._bn_rstd), out=gacts[src + 1], dgamma=self.view(gamma, self.grad),
                                  dbeta=self.view(beta, self.grad), ws=self._ws_bn)
                if on_ready:
                    on_ready([gamma.index, beta.index])
                written[src + 1] = True
                continue
            wt, bt = self.conv_params[i]
            # a normalised convolution's bias gradient is zero (the mean subtraction cancels the bias): the kernel's sum goes
            # to scratch and the variable's slot in grad is never written
            normed = self.batchnorm is not None and i in self.bn_convs
            ops.conv2d_bwd_weight(acts[src + 1], g, nd["cout"], nd["k"], nd["stride"], nd["pt"], nd["pl"], dw=self.view(wt, self.grad),
                                  dbias=self._bn_dbias[:nd["cout"]] if normed else self.view(bt, self.grad), ws=self._ws)
            if on_ready:
                on_ready([wt.index, bt.index])
            if src < 0:
                continue                        # no gradient w.r.t. the image
            relu_src = acts[src + 1] if relu_of(src + 1) else None
            if fp8 and i in self.mx_dgrad:
                dyq, dys = g8[self.mx_groot[i]]
                wtq, wts = self.mxfp8_wt(i)
                q, sc = g8[src] if self.mx_gmaps.get(src) == ("fp8", i) else (None, None)
                ops.conv2d_bwd_data_mxfp8(dyq, dys, wtq, wts, relu_src, acts[src + 1].shape, nd["stride"], nd["pt"], nd["pl"],
                                          accumulate=written[src + 1], want_fp8=q is not None, out=gacts[src + 1], out_q=q,
                                          out_scale=sc)
            else:
                ops.conv2d_bwd_data(g, self.w_t[i], relu_src, acts[src + 1].shape, nd["stride"], nd["pt"], nd["pl"],
                                    accumulate=written[src + 1], out=gacts[src + 1], ws=self._ws)
                wrote(src, "dgrad", i)
            written[src + 1] = True
        if on_ready:
            on_ready([i for wt, bt in self.head_params for t in (wt, bt) for i in t.indices])

    # ---------------------------------------------------------------- micro-batches
    def accumulate_clipped(self, first):
        """grad_acc (+)= the clipped gradient of this micro-batch, with the roundings of the data-parallel exchange: the
        gradient is clipped IN PLACE (fp32(g * scale), what a rank sends: clip_range_in_place) and then added (ssd_grad_accumulate
        without a scale table), as tf.clip_by_norm followed by the sum does it (reference models/ssd_model.py:249-255).
        SSDEngine's form rounds once, fma(g, scale, acc), so its sum and a two-rank exchange differ in the last bit of some
        elements.  SSD300 absorbs that; this network does not (measured: 64 280 parameters apart by <= 1.5e-8 after one Adam
        step put the next step's gradients 1.25 % apart in relative l2 -- 50 bf16 layers and hard-negative mining in between).
        With this form two ranks and one process running the same two micro-batches hold the same bits.  One more pass over
        the flat gradient per micro-batch."""
        if self.grad_acc is None:
            self.grad_acc = torch.empty_like(self.grad)
        self.apply_clip_in_place()
        _lib.check(self.L.ssd_grad_accumulate(ops._ptr(self.grad_acc), ops._ptr(self.grad), self.n_flat, None, None,
                                              1 if first else 0, ops._stream()))

    # ---------------------------------------------------------------- batchnorm: state and folding
    def state_dict(self):
        sd = super().state_dict()
        if self.batchnorm is not None:
            sd.update(bn_running_mean=self.bn_running_mean.cpu(), bn_running_var=self.bn_running_var.cpu(),
                      bn=dict(momentum=self.batchnorm.momentum, eps=self.batchnorm.eps))
        return sd

    def load_state_dict(self, sd):
        """As SSDEngine.load_state_dict (a default engine's and a batchnorm engine's layouts refuse each other through the
        variable names); a batchnorm engine also restores its running statistics."""
        super().load_state_dict(sd)
        if self.batchnorm is not None:
            self.bn_running_mean.copy_(sd["bn_running_mean"])
            self.bn_running_var.copy_(sd["bn_running_var"])

    def folded(self):
        """A default ResNet50SSDEngine (no batch normalisation) loaded with fold_batchnorm_params of this engine's parameters
        and running statistics: what this engine computes in inference mode, on every path of the default engine, the
        block-scaled fp8 ones included.  Fresh optimizer slots."""
        if self.batchnorm is None:
            raise ValueError("folded() needs a batchnorm engine")
        names = {t.name: t for t in self.tensors}
        params = {n: self.view(t, self.param) for n, t in names.items()}
        out = fold_batchnorm_params(self.graph, params, (self.bn_running_mean, self.bn_running_var), self.batchnorm.eps)
        eng = ResNet50SSDEngine(classes=self.classes, in_size=self.in_size, device=self.device)
        for t in eng.tensors:
            eng.view(t, eng.param).copy_(out[t.name])
        eng.refresh_weights(cast=True)
        return eng
