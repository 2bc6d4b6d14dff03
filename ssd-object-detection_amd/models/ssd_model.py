"""SSDObjectDetectionModel with the reference's surface (models/ssd_model.py of the reference: constructor
:50-52, TrainConfig :20-40, train :326, get_train_set :209, _train_step :229, _ssd_loss :341, get_prior_box
:416, save/load :405-411, get_log_dir :419), executed on MI355X by the HIP engine.

What differs from the reference, by design:
  * get_train_set batches samples first and runs target assignment for the whole batch on the device.
  * _ssd_loss / _train_step return device tensors; nothing synchronises the host unless the caller reads a
    scalar (the reference forces >= 4 device->host copies per micro-batch, :389-394).
  * `distributed=True` shards the batch by image over torch.distributed ranks: every rank is one micro-batch
    (loss, mining and per-tensor clipping are per rank, as the reference does per micro-batch :240-256), the
    clipped gradients are summed with one RCCL all-reduce and divided by the rank count.
  * inference adds a real NMS pass (`detect`), which the reference lacks.
"""
import contextlib
import logging
import math
import os
import time

import numpy as np
import torch

from .. import ops
from ..engine import (MOBILENET_V1_SSD300_NUM_PRIORS, MOBILENET_V1_SSD300_TRUNK, SSDEngine, VGG16_SSD300_NUM_PRIORS,
                      VGG16_SSD300_TRUNK)
from ..parallel import GradReducer, shard_range
from .. import optimizers as _opt
from ..utils.scalar_log import ScalarLog

logger = logging.getLogger(__name__)
_RESTORED = object()                            # _slot_owner marker: the optimizer slots were loaded from a checkpoint


class _RawList(list):
    """The first samples of a reader-contract split (data_loaders RawSplit), still marked for device preprocessing."""
    raw = True


class SSDObjectDetectionModel:
    class TrainConfig:
        def __init__(self, epoch, batch_size, optimizer, warmup=True, warmup_optimizer=None, warmup_step=1000,
                     visualization_log_interval=10, split_batch=False, split_batch_size=4, start_epoch=0, augment=None,
                     val=None, loss=None, clip=0.01, ema=None):
            if warmup_optimizer is None:
                warmup_optimizer = _opt.Adam(_opt.PolynomialDecay(1e-6, 1000, 0.001))
            self.epoch = epoch
            self.batch_size = batch_size
            self.optimizer = optimizer
            self.warmup = warmup
            self.warmup_optimizer = warmup_optimizer
            self.warmup_step = warmup_step
            self.visualization_log_interval = visualization_log_interval
            self.split_batch = split_batch
            self.split_batch_size = split_batch_size
            self.start_epoch = start_epoch                 # > 0: resumed run (no warm-up, epochs start_epoch..epoch-1)
            self.augment = augment                         # ops.AugmentSpec: SSD data augmentation on the device; None = off
            # the training loss: None / "reference" = the reference's _ssd_loss; "multibox" = the SSD paper's loss (per-image
            # mining, smooth L1, every term over P); "softmax_focal" = the softmax focal loss over every anchor; or an
            # ops.LossSpec of either with its parameters.  ValueError for anything else
            self.loss = ops.LossSpec.of(loss)
            # per-tensor clip norm of the gradients (tf.clip_by_norm(g, clip), reference :249); None or 0: no clipping (the
            # clip kernels run with clip = 0: every scale is 1, the norms are still written)
            if clip is not None and (isinstance(clip, bool) or not isinstance(clip, (int, float)) or not clip >= 0):
                raise ValueError("clip must be a number >= 0 or None, not %r" % (clip,))
            self.clip = float(clip) if clip else 0.0
            # validation during the run (None = off): dict(every=1, batch_size=32, score_thresh=0.05, iou_thresh=0.45,
            # max_dets=100, num_data=0, precision="bf16"); missing keys take these defaults.  After every `every`-th epoch
            # the validation split (its first num_data samples if > 0) is evaluated with metric="device".  An optional key
            # scoring="best" | "all" (evaluate()'s; absent = "best") is kept only when given, and so is protocol="map" | "coco"
            # (evaluate()'s; absent = "map": val/mAP, val/AP50, val/AP75; "coco": COCO's twelve values) | "voc07" | "voc12"
            # (PASCAL VOC's mAP: val/mAP only)
            if val is not None and val.get("scoring", "best") not in ("best", "all"):
                raise ValueError("val['scoring'] must be 'best' or 'all', not %r" % (val["scoring"],))
            if val is not None and val.get("protocol", "map") not in ("map", "coco", "voc07", "voc12"):
                raise ValueError("val['protocol'] must be 'map', 'coco', 'voc07' or 'voc12', not %r" % (val["protocol"],))
            # ... and weights="ema" | "live" | "both" (absent: the averaged weights where the run keeps an average, else the live
            # ones; "both": val/... from the averaged weights and val_live/... from the live ones), kept only when given
            if val is not None and val.get("weights", "ema") not in ("ema", "live", "both"):
                raise ValueError("val['weights'] must be 'ema', 'live' or 'both', not %r" % (val["weights"],))
            self.val = None if val is None else dict(dict(every=1, batch_size=32, score_thresh=0.05, iou_thresh=0.45,
                                                          max_dets=100, num_data=0, precision="bf16"), **val)
            # an exponential moving average of the weights (ops.EmaSpec.of: None = off, a decay, a dict(decay, warmup) or a
            # spec): updated behind every optimizer step, the warm-up optimizer's included; validation, evaluate / detect /
            # detections(weights="ema") and save(weights="ema") read it
            self.ema = ops.EmaSpec.of(ema)

    class Config:
        def __init__(self, classes, log_dir):
            self.log_dir = log_dir
            self.input_shape = (300, 300, 3)
            self.classes = classes + 1               # background is the LAST class index
            self.thresh = 0.5

    def __init__(self, classes, log_dir, device="cuda", seed=0, distributed=False, timestamp_dir=True, l2norm=None,
                 network=None, fp8_inference=False):
        """l2norm: the SSD paper's L2 normalisation of the 38x38 feature map in front of its head, with a learned per-channel
        scale (ops.L2NormSpec.of: None / False = off as in the reference, True = the paper's initial scale 20, a number, a dict
        or a spec).  The scale is one more variable of the engine: trained, clipped, saved and loaded like the others.

        network (ops.NetworkSpec.of: None / "ssd300" = the reference's network, as without the argument; "vgg16_ssd300" = the
        SSD paper's VGG-16 SSD300 (engine.VGG16_SSD300_TRUNK: conv4_3 / fc7 feature maps, pool5 3x3 / 1, dilated fc6) on the
        same engine class and the same step, l2norm as for ssd300 (the paper trains it with l2norm=True);
        "mobilenet_v1_ssd300" = MobileNet-v1 SSD300 (engine.MOBILENET_V1_SSD300_TRUNK: depthwise 3x3 + 1x1 blocks, 2268 default
        boxes on grids 19 .. 1 with ops.MOBILENET_SSD300_S_REF), same engine class and step, bf16 only: ValueError together with
        l2norm or fp8_inference; "resnet50_ssd512", a
        dict or a spec): the ResNet-50 SSD512 network (resnet_engine.ResNet50SSDEngine) at a 512 or 256 input, optionally with
        live batch normalisation or an MX-fp8 training forward.  Its step is backward -> clip -> one optimizer launch over the
        flat buffer (the engine has no per-bucket schedule); everything else -- targets, both losses, the three optimizers,
        split_batch, data parallelism, validation, checkpoints, the scalar log -- is the same code.  With split_batch a
        batchnorm network normalises each micro-batch with that micro-batch's statistics and updates its running statistics
        once per micro-batch; under data parallelism every rank normalises with its own batch (no synchronised batch norm).
        ValueError for l2norm together with the ResNet.

        fp8_inference: the engine's switch of the same name -- detect / detections / evaluate(precision="mxfp8") for the
        "vgg16_ssd300" network, which refuses that precision without it ("ssd300" has its fp8 forward either way).  It changes
        nothing else: training, the variables and checkpoints are the same with and without it, so it is not part of the
        network's identity.  ValueError for the ResNet, whose fp8 is NetworkSpec.precision."""
        self.network = ops.NetworkSpec.of(network, l2norm=l2norm)
        if not isinstance(fp8_inference, bool):
            raise ValueError("fp8_inference must be True or False, not %r" % (fp8_inference,))
        if fp8_inference and self.network.kind == "mobilenet_v1_ssd300":
            raise ValueError("fp8_inference together with network kind 'mobilenet_v1_ssd300': its depthwise layers run in bf16 only")
        if fp8_inference and self.network.kind not in ("ssd300", "vgg16_ssd300"):
            raise ValueError("fp8_inference is the switch of the ssd300 / vgg16_ssd300 engines; the %s network's fp8 forward is "
                             "set by its network spec (precision)" % self.network.kind)
        self.fp8_inference = fp8_inference
        self.distributed = bool(distributed)
        if timestamp_dir:
            stamp = [time.strftime("%Y-%m-%d-%H%M%S", time.localtime())]
            if self.distributed and torch.distributed.is_initialized():
                torch.distributed.broadcast_object_list(stamp, src=0)     # one run directory for all ranks (rank 0's clock)
            log_dir = os.path.join(log_dir, stamp[0])
        self.cfg = SSDObjectDetectionModel.Config(classes, log_dir)
        self.device = torch.device(device)
        net = self.network
        if net.kind in ops.NetworkSpec.ENGINE_KINDS:
            # one engine class, three trunks: the same step (fused per-bucket optimizer, high-priority main stream); the two
            # VGG trunks share the default boxes (grids 38, 19, 10, 5, 3, 1), MobileNet has its own (19, 10, 5, 3, 2, 1)
            graph, boxes = {}, {}
            if net.kind == "vgg16_ssd300":
                graph = dict(trunk=VGG16_SSD300_TRUNK, num_priors=VGG16_SSD300_NUM_PRIORS)
            elif net.kind == "mobilenet_v1_ssd300":
                graph = dict(trunk=MOBILENET_V1_SSD300_TRUNK, num_priors=MOBILENET_V1_SSD300_NUM_PRIORS)
                boxes = dict(s_ref=ops.MOBILENET_SSD300_S_REF)
            self._engine = SSDEngine(classes=self.cfg.classes, in_size=self.cfg.input_shape[0], device=device, seed=seed,
                                     l2norm=l2norm, fp8_inference=fp8_inference, **graph)
            self._pset = ops.build_priors(grids=self._engine.grids, device=device, **boxes)
            self._forward_train = self._engine.forward
            self._backward_args = {}
        else:
            from ..resnet_engine import ResNet50SSDEngine
            self.cfg.input_shape = (net.in_size, net.in_size, 3)
            self._engine = eng = ResNet50SSDEngine(classes=self.cfg.classes, in_size=net.in_size, device=device, seed=seed,
                                                   batchnorm=net.batchnorm)
            self._pset = ops.build_priors(grids=eng.grids, s_ref=ops.ssd512_s_ref(net.in_size), ratios=ops.SSD512_RATIOS,
                                          in_size=net.in_size, device=device)
            # train=True: a batchnorm engine uses (and saves) batch statistics, an fp8 forward writes the maps backward() reads
            self._forward_train = lambda x: eng.forward(x, net.precision, train=True)
            self._backward_args = dict(dgrad_precision=net.dgrad_precision)
        assert self._pset.A == self._engine.A
        # bumped by every training forward (running statistics), every optimizer launch and load(): what a cached inference
        # engine (the folded fp8 one of a batchnorm network) was made from
        self._version = 0
        self._folded = None                          # (version, engine.folded())
        self.ema_spec = None                         # ops.EmaSpec of the engine's averaged weights (enable_ema); None: no average
        self._loaded_ema = None                      # (ema, ema_updates) of a checkpoint loaded before the average was enabled
        self.folds_built = 0
        self._prior_box = None
        self._comm_stream = None
        self._slot_owner = None                      # optimizer object whose Adam moments the engine holds
        self._reducer = None
        self.last_info = None
        self._targets_event = None
        self._match_ws = ops.MatchWorkspace()
        self.fused_optimizer = os.environ.get("SSD_FUSED_OPTIMIZER", "1") == "1"   # Adam per bucket inside backward
        # the step's main chain (forward, loss, data gradients) runs on a HIGH-priority stream: its kernels are the critical
        # path, the weight gradients / optimizer on the engine's side stream fill in around them (measured: -0.04 ms per step;
        # the other way round, side stream high, +0.13 ms)
        # An engine that walks its network on ONE stream (side_streams False: the ResNet) has nothing to fill in: there the
        # priority stream only costs its two hand-overs per step (measured at batch 16, input 512: +0.14 ms, +0.33 ms with
        # batchnorm), so its step stays on the caller's stream
        self.high_priority_main = os.environ.get("SSD_MAIN_PRIO", "-1") == "-1" and self._engine.side_streams
        self._main_hi = None

    # ------------------------------------------------------------------ accessors
    def get_prior_box(self):
        """float64 [8732, 4] numpy array, as the reference returns."""
        if self._prior_box is None:
            self._prior_box = self._pset.priors.cpu().numpy()
        return self._prior_box

    def get_log_dir(self):
        return self.cfg.log_dir

    def get_engine(self):
        return self._engine

    def set_background_prior(self, pi=0.01):
        """The engine's set_background_prior: every head's conf biases start so that softmax puts 1 - pi on the background
        (what a focal loss wants before the first step of a run from scratch).  Never called implicitly; tools/train.py calls
        it for `model.train.loss.background_prior`.  Under data parallelism every rank calls it (the replicas stay identical)."""
        self._engine.set_background_prior(pi)
        self._version += 1                           # a cached inference engine was made from the old biases

    def enable_ema(self, spec):
        """Keep an exponential moving average of the weights (ops.EmaSpec.of(spec); engine.enable_ema): it starts at the
        current weights with no updates -- or, right after load() of a checkpoint that carries an average, at that average
        and its update count.  TrainConfig(ema=...) calls this at the first step of a run that has not; called again it only
        replaces the spec (the decay schedule), the average goes on.  Under data parallelism every rank calls it."""
        spec = ops.EmaSpec.of(spec)
        if spec is None:
            raise ValueError("enable_ema needs a decay, a dict(decay, warmup) or an ops.EmaSpec, not None")
        eng = self._engine
        if eng.ema is None:
            eng.enable_ema()
            if self._loaded_ema is not None:
                eng.ema.copy_(self._loaded_ema[0])
                eng.ema_updates = int(self._loaded_ema[1])
        self._loaded_ema = None
        self.ema_spec = spec

    @contextlib.contextmanager
    def _weights(self, weights):
        """The weights the inference calls read: "live", or "ema" -- the block runs inside engine.averaged(), and _version is
        bumped on entry and on exit so that a cached folded network is rebuilt and never serves the other set."""
        if weights not in ("live", "ema"):
            raise ValueError("weights must be 'live' or 'ema', not %r" % (weights,))
        if weights == "live":
            yield
            return
        if self._engine.ema is None:
            raise ValueError("weights='ema' on a model without averaged weights: TrainConfig(ema=...) or enable_ema() first")
        self._version += 1
        try:
            with self._engine.averaged():
                yield
        finally:
            self._version += 1

    # ------------------------------------------------------------------ input pipeline (A8)
    def _rank_world(self):
        if self.distributed and torch.distributed.is_initialized():
            return torch.distributed.get_rank(), torch.distributed.get_world_size()
        return 0, 1

    def get_train_set(self, dataset, batch_size=1, shard=None, augment=None):
        """Iterable of (image f32[B,300,300,3] in [-1,1], (cls i32[B,A], loc f32[B,A,4], mask u8[B,A])) device
        batches; remainder dropped (reference :209-227: match_bbox -> apply_anchor_box -> (x-0.5)*2 -> batch).

        Data parallel (`distributed=True`, or an explicit shard=(rank, world)): batch_size is the GLOBAL batch and the
        iterable yields this rank's images of every global batch -- parallel.shard_range, positions
        [rank*b/world, (rank+1)*b/world) -- so all ranks see the same number of batches (the same remainder is dropped)
        and disjoint samples.  Samples of other ranks are skipped without being produced when the dataset offers
        lazy() (an iterable of zero-argument callables, one per sample, in iteration order).

        augment (ops.AugmentSpec, no reference counterpart): every batch is augmented on the device and the image comes back as
        the bf16 network input.  A sample's Philox counter is its position in the stream of samples this iterable produces,
        counted across batches and passes from augment.first_index, the same on every rank: an image is augmented the same
        way whatever the world size.  The count restarts with a new iterable (a resumed run does not replay the stream)."""
        model = self
        rank, world = shard if shard is not None else self._rank_world()
        assert batch_size % world == 0, "the global batch must divide evenly over the ranks"
        lo, hi = shard_range(batch_size, rank, world)
        raw = bool(getattr(dataset, "raw", False))     # reader-contract samples: /255, resize, box normalisation on the device

        class _Batches:
            produced = 0                               # samples of the global stream yielded so far (all ranks alike)

            def __iter__(self_inner):
                thunks = dataset.lazy() if hasattr(dataset, "lazy") else ((lambda s=s: s) for s in dataset)
                mine, pos = [], 0
                for thunk in thunks:
                    if lo <= pos < hi:
                        mine.append(thunk)
                    pos += 1
                    if pos == batch_size:
                        imgs, clss, boxes = [], [], []
                        for t in mine:
                            image, cls, box = t()[:3]                  # (a reader's crowd flags are the metric's business)
                            if raw:
                                imgs.append(image if isinstance(image, ops.EncodedImage) else np.asarray(image))
                            else:
                                imgs.append(np.asarray(image, np.float32))
                            clss.append(np.asarray(cls, np.float32))
                            boxes.append(np.asarray(box, np.float32))
                        make = model.make_batch_raw if raw else model.make_batch
                        if augment is None:
                            yield make(imgs, clss, boxes)
                        else:
                            first = augment.first_index + self_inner.produced + lo
                            self_inner.produced += batch_size
                            yield make(imgs, clss, boxes, augment=augment.at(first))
                        mine, pos = [], 0

        return _Batches()

    def match_async(self, gt, out=None):
        """Target assignment (A3-A5) for a packed ground-truth batch on the engine's side stream: it depends on nothing
        the network computes, so it runs underneath the forward pass; _train_step waits for it before the loss.
        gt = ops.pack_gt(...) tuple; out = optional (cls, loc, mask) buffers to reuse."""
        B, A, dev = gt[2].numel() - 1, self._pset.A, self.device
        if out is None:
            out = (torch.empty((B, A), dtype=torch.int32, device=dev),
                   torch.empty((B, A, 4), dtype=torch.float32, device=dev),
                   torch.empty((B, A), dtype=torch.uint8, device=dev))
        side = self._engine._side_stream() if self._engine.overlap_heads else None
        if side is None:
            return ops.match_encode(*gt, self._pset, self.cfg.thresh, out=out, ws=self._match_ws)
        start = torch.cuda.Event()
        start.record()                                 # everything that still reads `out` / gt is ahead of this point
        with torch.cuda.stream(side):
            side.wait_event(start)
            ops.match_encode(*gt, self._pset, self.cfg.thresh, out=out, ws=self._match_ws)
            self._targets_event = torch.cuda.Event()
            self._targets_event.record(side)
        return out

    def make_batch(self, images, cls_list, box_list, augment=None):
        """augment (ops.AugmentSpec): SSD data augmentation of the batch on the device (include/ssd_hip.h); the image then
        comes back as the bf16 network input [B,S,S,8], images f32 [H,W,3] in [0,1] of any one size."""
        img = torch.from_numpy(np.stack(images, 0)).to(self.device, non_blocking=True)
        if augment is not None:
            B, H, W = img.shape[0], img.shape[1], img.shape[2]
            hw = torch.tensor([[H, W]] * B, dtype=torch.int32).to(self.device)
            return self._augmented(img.contiguous(), 1, None, hw, box_list, cls_list, augment)
        img = (img - 0.5) * 2                          # reference :214 (exact in fp32); get_train_set's contract is f32
        gt = ops.pack_gt(box_list, cls_list, device=self.device)
        cls, loc, mask = ops.match_encode(*gt, self._pset, self.cfg.thresh)
        return img, (cls, loc, mask)

    def _augmented(self, src, kind, src_off, hw_d, box_list, cls_list, augment, tlwh=False):
        """Augment a batch (boxes relative cx,cy,w,h, or COCO pixels with tlwh) and assign its targets.  match_encode gets
        the un-augmented total and max_nt: upper bounds of the kept boxes, which is all it needs (include/ssd_hip.h)."""
        gt_box, gt_cls, gt_off, total, max_nt = ops.pack_gt(box_list, cls_list, device=self.device)
        if tlwh and total:
            gt_box = ops.box_prep(gt_box, gt_off, hw_d)
        params, box, cls_, off = ops.augment_plan(gt_box, gt_cls, gt_off, hw_d, total, augment.stages, augment.seed,
                                                  augment.first_index)
        x = ops.augment_image(src, kind, src_off, hw_d, params, int(self.cfg.input_shape[0]), True)
        cls, loc, mask = ops.match_encode(box, cls_, off, total, max_nt, self._pset, self.cfg.thresh)
        return x, (cls, loc, mask)

    decode_workers = 8                     # host threads of the JPEG entropy decode (ops.image_arena); never sized from the machine
    decode_fallback = "pil"                # streams the device decoder refuses: Pillow on the host, or None to refuse them too

    def _raw_arena(self, images, upload):
        """The ragged uint8 arena (flat u8, off i64 [B], hw i32 [B,2], all on the device) of a batch of reader-contract
        images: decoded uint8 arrays [H,W,3], images still encoded as JPEG (ops.EncodedImage), or a mix.  Decoded arrays
        alone are concatenated on the host and sent with `upload` (host array -> device tensor), three transfers; as soon as
        one image is encoded the batch goes through ops.image_arena: entropy decode on host threads, one transfer, the
        reconstruction kernels."""
        if any(isinstance(im, ops.EncodedImage) for im in images):
            flat, off, hw, self.last_decode_stats = ops.image_arena(list(images), self.device, self.decode_workers,
                                                                    self.decode_fallback)
            return flat, off, hw
        hw = np.array([im.shape[:2] for im in images], np.int32)
        sizes = [int(im.size) for im in images]
        off = np.zeros(len(sizes), np.int64)
        off[1:] = np.cumsum(sizes[:-1])
        flat = np.concatenate([np.ascontiguousarray(im, np.uint8).reshape(-1) for im in images])
        hw_d = upload(hw)
        return upload(flat), upload(off), hw_d

    def make_batch_raw(self, images_u8, cls_list, box_tlwh_list, augment=None):
        """The same from what the COCO reader yields before any preprocessing: uint8 RGB images of
        arbitrary sizes -- decoded arrays, ops.EncodedImage (JPEG bytes, decoded on the way: _raw_arena) or a mix -- and COCO
        [x, y, w, h] pixel boxes.  '/255', cv2.resize to the network size, '(x-0.5)*2'
        (reference data_loaders/coco/make_dataset.py:117, data_loaders/ssd/make_dataset.py:40-44, models/ssd_model.py:214)
        and the box conversion run on the device; returns the prepared bf16 network input instead of the f32 image.
        augment (ops.AugmentSpec): SSD data augmentation on the device as well (include/ssd_hip.h)."""
        dev = self.device
        flat_d, off_d, hw_d = self._raw_arena(images_u8, lambda a: torch.from_numpy(a).to(dev))
        if augment is not None:
            return self._augmented(flat_d, 0, off_d, hw_d, box_tlwh_list, cls_list, augment, tlwh=True)
        x = ops.image_resize_prep(flat_d, off_d, hw_d, int(self.cfg.input_shape[0]), True)
        gt_box, gt_cls, gt_off, total, max_nt = ops.pack_gt(box_tlwh_list, cls_list, device=dev)
        gt_box = ops.box_prep(gt_box, gt_off, hw_d) if total else gt_box
        cls, loc, mask = ops.match_encode(gt_box, gt_cls, gt_off, total, max_nt, self._pset, self.cfg.thresh)
        return x, (cls, loc, mask)

    # ------------------------------------------------------------------ loss (A6)
    @staticmethod
    def _ssd_loss(y_true, y_pred, heads=None, loss=None, priors=None):
        """Returns (total loss tensor, info) where info maps the reference's three names to device scalars and
        carries the gradients w.r.t. (pred_box, pred_cls) under 'dloc' / 'dconf' -- or, with `heads` (the engine's
        ops.HeadGradBuffers), as the compact per-level rows the heads' backward pass consumes ('heads').  `loss`: None,
        a kind name or an ops.LossSpec (None / "reference": the reference's loss).  `priors`: the model's ops.PriorSet, which the
        IoU box terms of a LossSpec (box="giou" | "diou" | "ciou") decode with; the other losses do not read it."""
        gt_cls, gt_box, gt_mask = y_true
        pred_box, pred_cls = y_pred
        assert gt_cls.shape[0] == gt_box.shape[0] == gt_mask.shape[0] == pred_box.shape[0] == pred_cls.shape[0]
        spec = None if loss is None else ops.LossSpec.of(loss)
        if spec is not None and spec.kind == "multibox":
            if heads is not None:
                out = ops.multibox_loss_heads(pred_cls, pred_box, gt_cls, gt_box, gt_mask, heads, spec.neg_pos_ratio,
                                              spec.loc_weight, box=spec.box, priors=priors)
                dconf = dloc = None
            else:
                out, dconf, dloc = ops.multibox_loss(pred_cls, pred_box, gt_cls, gt_box, gt_mask, spec.neg_pos_ratio,
                                                     spec.loc_weight, box=spec.box, priors=priors)
        elif spec is not None and spec.kind == "softmax_focal":
            if heads is not None:
                out = ops.softmax_focal_loss_heads(pred_cls, pred_box, gt_cls, gt_box, gt_mask, heads, spec.gamma, spec.alpha,
                                                   spec.loc_weight, box=spec.box, priors=priors)
                dconf = dloc = None
            else:
                out, dconf, dloc = ops.softmax_focal_loss(pred_cls, pred_box, gt_cls, gt_box, gt_mask, spec.gamma, spec.alpha,
                                                          spec.loc_weight, box=spec.box, priors=priors)
        elif heads is not None:
            out = ops.ssd_loss_heads(pred_cls, pred_box, gt_cls, gt_box, gt_mask, heads)
            dconf = dloc = None
        else:
            out, dconf, dloc = ops.ssd_loss(pred_cls, pred_box, gt_cls, gt_box, gt_mask)
        info = {"cls loss pos": out[1], "cls loss neg": out[2], "loc loss": out[0], "status": out[7],
                "dconf": dconf, "dloc": dloc, "heads": heads, "raw": out}
        return out[3], info

    # ------------------------------------------------------------------ train step (A7)
    def main_stream(self):
        """The high-priority stream the step's main chain runs on.  A training loop that issues its own per-step work (input
        preparation, target assignment, logging reads) inside `with torch.cuda.stream(model.main_stream())` saves the two
        cross-stream hand-overs per step (~15-25 us each) that `_train_step` otherwise makes from and back to the caller's
        stream.  None where the step runs on the caller's stream anyway."""
        if not self.high_priority_main or not torch.cuda.is_available():
            return None
        if self._main_hi is None:
            self._main_hi = torch.cuda.Stream(priority=-1)
        return self._main_hi

    def _train_step(self, *args, **kwargs):
        if not self.high_priority_main or not torch.cuda.is_available():
            return self._train_step_on_current(*args, **kwargs)
        if self._main_hi is None:
            self._main_hi = torch.cuda.Stream(priority=-1)
        cur = torch.cuda.current_stream()
        if cur == self._main_hi:                       # the caller already works on it (main_stream())
            return self._train_step_on_current(*args, **kwargs)
        self._main_hi.wait_stream(cur)
        with torch.cuda.stream(self._main_hi):
            out = self._train_step_on_current(*args, **kwargs)
        cur.wait_stream(self._main_hi)             # the caller's stream sees the step complete, as before
        return out

    def _train_step_on_current(self, image, gt_cls, gt_bbox, gt_mask, ssd_optimizer, stage="train", set_names=None,
                               set_colors=None, step=0, cfg=None):
        eng = self._engine
        batch_size = image.shape[0]
        batch_step = batch_size if (cfg is None or not cfg.split_batch) else cfg.split_batch_size
        n_micro = 0
        info = None
        world = torch.distributed.get_world_size() if self.distributed else 1
        single = world == 1 and batch_step >= batch_size
        overlap = world > 1 and batch_step >= batch_size           # one micro-batch per rank: bucketed, overlapped reduce
        clip = float(getattr(cfg, "clip", 0.01))       # tf.clip_by_norm(x, 0.01), reference :249; 0.0 = off
        self._clip = clip
        if overlap and self._reducer is None:
            blocks = [t.nblocks for t in eng.tensors]
            self._reducer = GradReducer(eng.grad, [t.block0 * eng.block for t in eng.tensors], blocks, eng.block,
                                        lambda t0, t1: eng.clip_range_in_place(t0, t1, self._clip))
        if getattr(cfg, "ema", None) is not None and cfg.ema is not self.ema_spec:
            self.enable_ema(cfg.ema)
        if self.ema_spec is not None:                  # this step's factor: every optimizer launch below is followed by the average's
            eng.ema_om = self.ema_spec.one_minus_decay(eng.ema_updates)
        self._loaded_ema = None                        # (a checkpoint's average nobody asked for before training went on)
        momentum = isinstance(ssd_optimizer, _opt.SGD) and ssd_optimizer.uses_slots     # the momentum / decay kernel
        decay = None
        if momentum and ssd_optimizer.weight_decay > 0.0:
            decay = eng.decay_table(ssd_optimizer.weight_decay, ssd_optimizer.decay_bias)
        per_bucket = (isinstance(ssd_optimizer, _opt.Adam) or momentum) and self.fused_optimizer and eng.bucket_optimizer
        fused = single and per_bucket
        fused_dp = overlap and per_bucket
        if fused_dp:
            self._adopt_slots(ssd_optimizer)
        if fused:                                      # the optimizer runs per bucket inside the backward pass
            self._adopt_slots(ssd_optimizer)
            eng.step_count = ssd_optimizer.iterations
            lr = ssd_optimizer.lr()
            if momentum:
                fused_adam = dict(kind="sgd_momentum", lr=lr, momentum=ssd_optimizer.momentum,
                                  nesterov=ssd_optimizer.nesterov, decay=decay, clip=clip)
            else:
                fused_adam = dict(lr=lr, beta1=ssd_optimizer.beta_1, beta2=ssd_optimizer.beta_2,
                                  eps=ssd_optimizer.epsilon, clip=clip)
        for i in range(0, batch_size, batch_step):
            if image.dtype == torch.bfloat16:          # already prepared on the device (make_batch_raw)
                x = image[i:i + batch_step]
            else:
                x = ops.image_prep(image[i:i + batch_step].contiguous(), normalize=False)
            pred_loc, pred_conf = self._forward_train(x)
            self._version += 1
            if self._targets_event is not None:        # targets assigned on the side stream (match_async)
                torch.cuda.current_stream().wait_event(self._targets_event)
                self._targets_event = None
            heads = eng.head_grad_buffers(pred_loc.shape[0]) if pred_conf.dtype == torch.bfloat16 else None
            _, info = self._ssd_loss((gt_cls[i:i + batch_step], gt_bbox[i:i + batch_step], gt_mask[i:i + batch_step]),
                                     (pred_loc, pred_conf), heads, getattr(cfg, "loss", None), self._pset)
            if overlap:
                post = gates = None
                if fused_dp:
                    # Adam of a bucket on the communication stream right behind its all-reduce, as soon as the last data
                    # gradient that reads the bucket's transposed weights is enqueued (engine.bucket_gates): the update of
                    # all but the last bucket runs underneath the rest of the backward pass
                    eng.step_count = ssd_optimizer.iterations + 1
                    t = eng.step_count
                    lr = ssd_optimizer.lr()
                    if momentum:
                        post = lambda t0, t1: eng.sgd_range(t0, t1, lr, ssd_optimizer.momentum, ssd_optimizer.nesterov,
                                                            decay, None, 1.0 / world)
                    else:
                        b1, b2 = ssd_optimizer.beta_1, ssd_optimizer.beta_2
                        lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
                        post = lambda t0, t1: eng.adam_range(t0, t1, lr_t, b1, b2, ssd_optimizer.epsilon, None, 1.0 / world)
                    gates = eng.bucket_gates(self._reducer.buckets)
                self._reducer.begin(post, gates)
                eng.backward(info["dloc"], info["dconf"], on_ready=self._reducer.tensor_ready, heads=info["heads"],
                             on_dgrad=self._reducer.dgrad_done if fused_dp else None, **self._backward_args)
                self._reducer.finish()                 # clipped per bucket, summed over ranks (RCCL over xGMI)
            elif fused:
                eng.backward(info["dloc"], info["dconf"], fused_adam=fused_adam, heads=info["heads"])
            else:
                eng.backward(info["dloc"], info["dconf"], heads=info["heads"], **self._backward_args)
                eng.clip_scales(clip)                  # tf.clip_by_norm(x, 0.01) per tensor, reference :249
                if not single:
                    eng.accumulate_clipped(first=(n_micro == 0))
            n_micro += 1
        self._version += 1                             # the optimizer has run, or runs below
        if fused or fused_dp:
            ssd_optimizer.iterations += 1
            return self._finish_step(info, lr, pred_conf, pred_loc)
        self._adopt_slots(ssd_optimizer)
        lr = ssd_optimizer.lr()
        if single:
            grad, gscale, use_clip = eng.grad, 1.0, True
        elif overlap:
            grad, gscale, use_clip = eng.grad, 1.0 / world, False
        else:
            grad, use_clip = eng.grad_acc, False
            if world > 1:
                torch.distributed.all_reduce(grad)     # RCCL over xGMI: sum of the ranks' clipped gradients
            gscale = 1.0 / (n_micro * world)           # reference :256
        if momentum:
            eng.step_count = ssd_optimizer.iterations
            eng.sgd_momentum(lr, grad, gscale, use_clip, ssd_optimizer.momentum, ssd_optimizer.nesterov, decay)
        elif isinstance(ssd_optimizer, _opt.SGD):
            eng.sgd(lr, grad, gscale, use_clip)
        else:
            eng.step_count = ssd_optimizer.iterations
            eng.adam(lr, grad, gscale, use_clip, ssd_optimizer.beta_1, ssd_optimizer.beta_2, ssd_optimizer.epsilon)
        ssd_optimizer.iterations += 1
        return self._finish_step(info, lr, pred_conf, pred_loc)

    def _adopt_slots(self, ssd_optimizer):
        eng = self._engine
        if self._slot_owner is _RESTORED:             # slots came from a checkpoint: the first optimizer adopts them ...
            self._slot_owner = ssd_optimizer
            plain = isinstance(ssd_optimizer, _opt.SGD) and not ssd_optimizer.uses_slots       # reads no slot
            kind = "sgd_momentum" if isinstance(ssd_optimizer, _opt.SGD) else "adam"
            # ... unless they are another optimizer's: Adam moments are not a velocity.  (All-zero slots -- a model that was
            # never trained, or only by plain SGD -- are nobody's: no warning.  One host read, at the first step after load)
            if not plain and eng.slots != kind and bool(eng.adam_m.any() or eng.adam_v.any()):
                logger.warning("checkpoint holds %s slots, the optimizer is %s: starting from zero slots", eng.slots, kind)
                eng.adam_m.zero_()
                eng.adam_v.zero_()
        elif self._slot_owner is not ssd_optimizer:   # Keras keeps separate slots per optimizer (warm-up vs train)
            eng.adam_m.zero_()
            eng.adam_v.zero_()
            self._slot_owner = ssd_optimizer

    def _finish_step(self, info, lr, pred_conf, pred_loc):
        if self.ema_spec is not None:                 # the optimizer step is enqueued, the average's update behind it
            self._engine.ema_updates += 1
            self._engine.ema_om = None
        self._last_raw = info["raw"]                  # device f32[8] row for the sync-free scalar log (N4)
        info = {k: v for k, v in info.items() if k in ("cls loss pos", "cls loss neg", "loc loss", "status")}
        info["lr"] = lr
        self.last_info = info
        return pred_conf, pred_loc, info

    # ------------------------------------------------------------------ trainer shell
    def _train(self, data_loader, cfg):
        train_set, val_set = data_loader.get_dataset()     # (the reference drops the validation split, :291)
        self._val_set = val_set if getattr(cfg, "val", None) else None
        set_names, set_colors = data_loader.get_names_and_colors()
        batches = self.get_train_set(train_set, batch_size=cfg.batch_size, augment=getattr(cfg, "augment", None))
        self._assert_replicas_identical()
        self._scalars = ScalarLog(self.cfg.log_dir, self.device, distributed=self.distributed,
                                  console_interval=cfg.visualization_log_interval, logger=logger)
        try:
            self._train_loop(batches, set_names, set_colors, cfg)
        except BaseException:
            self._scalars.close(collective=False)      # unwinding: the other ranks may not reach a collective
            raise
        self._scalars.close()

    def _assert_replicas_identical(self):
        """Data parallelism assumes every rank starts from the same weights and optimizer state (same seed / same
        checkpoint): compare a checksum of the flat buffers across ranks before the first step."""
        rank, world = self._rank_world()
        if world == 1:
            return
        eng = self._engine
        sums = [eng.param.double().sum(), eng.param.double().abs().sum(), eng.adam_m.double().abs().sum(),
                eng.adam_v.double().sum(), torch.tensor(float(eng.step_count), dtype=torch.float64, device=eng.param.device)]
        if eng.ema is not None:                                # every rank averages the same parameters
            sums += [eng.ema.double().sum(), eng.ema.double().abs().sum(),
                     torch.tensor(float(eng.ema_updates), dtype=torch.float64, device=eng.param.device)]
        if getattr(eng, "batchnorm", None) is not None:       # the running statistics are state too (per rank afterwards)
            sums += [eng.bn_running_mean.double().sum(), eng.bn_running_mean.double().abs().sum(),
                     eng.bn_running_var.double().sum()]
        sums = torch.stack(sums)
        lo, hi = sums.clone(), sums.clone()
        torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
        torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
        if not torch.equal(lo, hi):
            raise RuntimeError("data-parallel replicas differ before training (checksums %s vs %s): same seed / "
                               "checkpoint on every rank?" % (lo.tolist(), hi.tolist()))

    def _train_loop(self, batches, set_names, set_colors, cfg):
        ms = self.main_stream()
        if ms is None or torch.cuda.current_stream() == ms:
            return self._train_loop_on_current(batches, set_names, set_colors, cfg)
        cur = torch.cuda.current_stream()              # the whole loop (batch assembly, steps, scalar ring) on the step's stream
        ms.wait_stream(cur)
        try:
            with torch.cuda.stream(ms):
                return self._train_loop_on_current(batches, set_names, set_colors, cfg)
        finally:
            cur.wait_stream(ms)

    def _train_loop_on_current(self, batches, set_names, set_colors, cfg):
        if cfg.warmup and getattr(cfg, "start_epoch", 0) == 0:
            logger.info("Warm up for %s steps", cfg.warmup_step)
            step = 0
            while step < cfg.warmup_step:
                got = False
                for image, (gt_cls, gt_bbox, gt_mask) in batches:
                    got = True
                    step += 1
                    _, _, info = self._train_step(image, gt_cls, gt_bbox, gt_mask, cfg.warmup_optimizer, "warmup",
                                                  set_names, set_colors, step, cfg)
                    self._log(step, info, cfg, "warmup")
                    if step >= cfg.warmup_step:
                        break
                if not got:
                    break
        step = cfg.optimizer.iterations if getattr(cfg, "start_epoch", 0) else 0     # resumed runs keep counting
        for epoch in range(getattr(cfg, "start_epoch", 0), cfg.epoch):
            logger.info("Epoch %s/%s", epoch + 1, cfg.epoch)
            for image, (gt_cls, gt_bbox, gt_mask) in batches:
                step += 1
                _, _, info = self._train_step(image, gt_cls, gt_bbox, gt_mask, cfg.optimizer, "train", set_names,
                                              set_colors, step, cfg)
                self._log(step, info, cfg, "train")
            self._scalars.flush()                      # one device->host read per epoch (or per full ring)
            val = getattr(cfg, "val", None)
            if val and (epoch + 1) % val["every"] == 0:
                self._validate(val, cfg.optimizer.iterations)
            self.save(os.path.join(self.cfg.log_dir, "model_weight", "model_weight_epoch_%d.pt" % epoch),
                      extra=dict(epoch=epoch + 1, iterations=cfg.optimizer.iterations,
                                 warmup_iterations=cfg.warmup_optimizer.iterations if cfg.warmup_optimizer else 0))

    def _validate(self, val, step):
        """Validation inside a run: the kept validation split through evaluate(metric="device") on the step's stream, then
        val/mAP, val/AP50, val/AP75 in scalars.jsonl at the optimizer's step count, behind the epoch's train lines.  Data
        parallel: the replicas are identical, so every rank evaluates the whole split (no collective inside the pass) and
        rank 0 writes.  A run that keeps averaged weights validates them (val["weights"] absent or "ema"); "live" validates the
        live ones, "both" writes val/... for the averaged and val_live/... for the live ones (and returns the averaged)."""
        mode = val.get("weights") or ("ema" if self._engine.ema is not None else "live")
        if mode == "both":
            r = self._validate_with(val, step, "ema", "val")
            self._validate_with(val, step, "live", "val_live")
            return r
        return self._validate_with(val, step, mode, "val")

    def _validate_with(self, val, step, weights, family):
        samples = self._val_set
        if val["num_data"] > 0:
            import itertools
            raw = bool(getattr(samples, "raw", False))
            samples = list(itertools.islice(iter(samples), val["num_data"]))
            if raw:
                samples = _RawList(samples)
        r = self.evaluate(samples, batch_size=val["batch_size"], score_thresh=val["score_thresh"], iou_thresh=val["iou_thresh"],
                          max_dets=val["max_dets"], precision=val["precision"], metric="device",
                          scoring=val.get("scoring", "best"), protocol=val.get("protocol", "map"), weights=weights)
        what = "validation" if (weights, family) == ("live", "val") else "validation (%s weights)" % weights
        if val.get("protocol", "map") in ("voc07", "voc12"):
            self._scalars.write_values(family, step, {"mAP": r["mAP"]})
            logger.info("%s at step %d: %s mAP %.4f", what, step, val["protocol"], r["mAP"])
            return r
        if val.get("protocol", "map") == "coco":
            from ..utils.metrics import COCO_SUMMARY_KEYS
            self._scalars.write_values(family, step, {k: r[k] for k in COCO_SUMMARY_KEYS})
            logger.info("%s at step %d: %s", what, step, " ".join("%s %.4f" % (k, r[k]) for k in COCO_SUMMARY_KEYS))
            return r
        self._scalars.write_values(family, step, {k: r[k] for k in ("mAP", "AP50", "AP75")})
        logger.info("%s at step %d: mAP %.4f AP50 %.4f AP75 %.4f", what, step, r["mAP"], r["AP50"], r["AP75"])
        return r

    def _log(self, step, info, cfg, stage):
        """Reference :281-285 writes five scalars per step, each a host read; here a step enqueues one 32-byte device
        copy and utils/scalar_log.py reads the ring back once per epoch / 512 steps (the reference's status assert,
        :375, fires at that read)."""
        self._scalars.record(stage, step, self._last_raw, info["lr"])

    def train(self, data_loader, cfg):
        if cfg.warmup is True:
            assert cfg.warmup_optimizer is not None, "Define a warmup optimizer if you want to enable warmup!"
        try:
            self._train(data_loader, cfg)
        except Exception:
            self.save("error_exit_save.pt", collective=False)
            logger.critical("Error occurred while training, last model weight is saved to 'error_exit_save.pt'")
            raise

    # ------------------------------------------------------------------ inference (A9 + A9')
    def detect(self, image, score_thresh=0.3, iou_thresh=0.45, max_cand=400, precision="bf16", weights="live"):
        """image f32 [B,300,300,3] in [-1,1] -> (score, cls, box_px, keep) device tensors [B,A(,4)].
        Scoring/decoding as the reference's visualize(); `keep` adds per-class NMS (no reference counterpart).
        precision="mxfp8": the network forward runs most of its trunk on block-scaled fp8 operands (SSDEngine.forward; no
        reference counterpart); "bf16" (default) as in training.  Any other value raises ValueError.
        weights="ema": the network runs with the averaged weights (enable_ema / TrainConfig(ema=...); ValueError on a model
        that keeps none); "live" (default): with the weights the last optimizer step left."""
        with self._weights(weights):
            return self._detect_prepared(ops.image_prep(image.contiguous(), normalize=False), score_thresh, iou_thresh,
                                         max_cand, precision)

    def _forward_infer(self, x, precision):
        """(loc, conf) of the inference forward: the engine's own (running statistics for a batchnorm network); "mxfp8" on a
        batchnorm network runs the folded network (engine.folded(): fold_batchnorm_params of the current parameters and
        running statistics), cached until a training forward, an optimizer launch or load() changes what it was made from."""
        if precision == "mxfp8" and self.network.batchnorm is not None:
            if self._folded is None or self._folded[0] != self._version:
                self._folded = (self._version, self._engine.folded())
                self.folds_built += 1
            return self._folded[1].forward(x, "mxfp8")
        return self._engine.forward(x, precision)

    def _detect_prepared(self, x, score_thresh, iou_thresh, max_cand=400, precision="bf16"):
        """detect() from the prepared network input bf16 [B,S,S,8]."""
        loc, conf = self._forward_infer(x, precision)
        score, cls, box, cand = ops.score_decode(conf, loc, self._pset, score_thresh, float(self.cfg.input_shape[0]))
        keep = ops.nms(score, cls, box, cand, iou_thresh, max_cand)
        return score, cls, box, keep

    def detections(self, image, score_thresh=0.01, iou_thresh=0.45, max_cand=None, keep_top_k=200, precision="bf16",
                   weights="live"):
        """image f32 [B,300,300,3] in [-1,1] -> ops.DetectPairs(n_det, score, cls, anchor, box, valid, n_cand): the compact
        multi-label detection output (ops.detect_pairs; no reference counterpart).  Every (anchor, class) pair above
        score_thresh is a candidate, so an anchor may be reported under several classes; per-class NMS over the best max_cand
        pairs (None: the library maximum), then the best keep_top_k rows per image.  precision and weights as detect()."""
        with self._weights(weights):
            return self._detections_prepared(ops.image_prep(image.contiguous(), normalize=False), score_thresh, iou_thresh,
                                             max_cand, keep_top_k, precision)

    def _detections_prepared(self, x, score_thresh, iou_thresh, max_cand=None, keep_top_k=200, precision="bf16"):
        """detections() from the prepared network input bf16 [B,S,S,8]."""
        loc, conf = self._forward_infer(x, precision)
        return ops.detect_pairs(conf, loc, self._pset, score_thresh, iou_thresh, max_cand, keep_top_k,
                                float(self.cfg.input_shape[0]))

    def _to_device(self, array):
        """Host array -> device through pinned memory, stream-ordered: no host synchronisation."""
        t = torch.from_numpy(np.ascontiguousarray(array))
        if t.numel() == 0:
            return torch.empty(t.shape, dtype=t.dtype, device=self.device)
        return t.pin_memory().to(self.device, non_blocking=True)

    def _eval_batch_raw(self, buf):
        """Reader-contract samples (decoded uint8 images of any size, COCO top-left pixel boxes: RawSplit) -> the prepared
        network input and the relative centre-form boxes, by the device preprocessing of make_batch_raw (no augmentation).
        Returns (x bf16 [B,S,S,8], box f32 [total,4] device, counts)."""
        imgs = [b[0] if isinstance(b[0], ops.EncodedImage) else np.ascontiguousarray(b[0], np.uint8) for b in buf]
        flat_d, off_d, hw_d = self._raw_arena(imgs, self._to_device)
        x = ops.image_resize_prep(flat_d, off_d, hw_d, int(self.cfg.input_shape[0]), True)
        counts = [int(np.shape(b[2])[0]) for b in buf]
        gt_off = np.zeros(len(buf) + 1, np.int32)
        gt_off[1:] = np.cumsum(counts)
        box = np.concatenate([np.asarray(b[2], np.float32).reshape(-1, 4) for b in buf], 0)
        box_d = self._to_device(box)
        if box.shape[0]:
            box_d = ops.box_prep(box_d, self._to_device(gt_off), hw_d)
        return x, box_d, counts

    def _coco_batch_extras(self, buf, raw):
        """(crowd u8 [total] or None when no sample carries flags, area_scale f64 [B] or None for prepared samples) of a
        batch of evaluation samples: the COCO protocol's extra inputs."""
        crowd = None
        if any(len(b) > 3 and b[3] is not None for b in buf):
            crowd = np.concatenate([np.asarray(b[3]).astype(bool).reshape(-1) if len(b) > 3 and b[3] is not None
                                    else np.zeros(int(np.shape(b[1])[0]), bool) for b in buf]).astype(np.uint8)
        scale = None
        if raw:
            s2 = float(self.cfg.input_shape[0]) * float(self.cfg.input_shape[0])
            scale = np.array([float(np.shape(b[0])[1]) * float(np.shape(b[0])[0]) / s2 for b in buf], np.float64)
        return crowd, scale

    def evaluate_into(self, acc, samples, batch_size=32, score_thresh=0.05, iou_thresh=0.45, precision="bf16", scoring="best",
                      weights="live"):
        """The batch loop of evaluate(metric="device"): every batch of `samples` through the network, scoring/decoding, NMS
        and acc.add (utils.device_map.DeviceMapAccumulator) on the current stream.  Host arrays reach the device through
        pinned memory; nothing in the loop reads the device or waits for it.  scoring="all": the compact rows of
        ops.detect_pairs (keep_top_k = acc.max_dets) go to acc.add as they are -- ssd_eval_match takes any row count, and its
        (score desc, index asc) order is the rows' own.  An accumulator of the COCO protocol (DeviceCocoAccumulator) also gets
        the samples' crowd flags (a fourth element, absent = none) and, for reader-contract samples, the area scale
        (source width x source height) / (S x S).  An accumulator of the VOC protocol (DeviceVocAccumulator) gets the fourth
        element as the boxes' `difficult` flags.  weights as detect(): the whole loop runs with that set."""
        coco = getattr(acc, "protocol", "map") == "coco"
        voc = getattr(acc, "protocol", "map") == "voc"
        if precision not in ("bf16", "mxfp8"):
            raise ValueError("precision must be 'bf16' or 'mxfp8', not %r" % (precision,))
        if scoring not in ("best", "all"):
            raise ValueError("scoring must be 'best' or 'all', not %r" % (scoring,))
        size = float(self.cfg.input_shape[0])
        raw = bool(getattr(samples, "raw", False))
        buf = []

        def flush():
            if not buf:
                return
            gt_off = np.zeros(len(buf) + 1, np.int32)
            gt_off[1:] = np.cumsum([int(np.shape(b[1])[0]) for b in buf])
            gt_cls = np.concatenate([np.asarray(b[1]).reshape(-1) for b in buf]).astype(np.int32)
            if raw:
                x, box_d, _ = self._eval_batch_raw(buf)
            else:
                img = self._to_device(np.stack([np.asarray(b[0], np.float32) for b in buf], 0))
                x = ops.image_prep(((img - 0.5) * 2).contiguous(), normalize=False)
                box_d = self._to_device(np.concatenate([np.asarray(b[2], np.float32).reshape(-1, 4) for b in buf], 0))
            if scoring == "all":
                d = self._detections_prepared(x, score_thresh, iou_thresh, keep_top_k=acc.max_dets, precision=precision)
                score, cls, box, keep = d.score, d.cls, d.box, d.valid
            else:
                score, cls, box, keep = self._detect_prepared(x, score_thresh, iou_thresh, precision=precision)
            if coco:
                crowd, scale = self._coco_batch_extras(buf, raw)
                acc.add(score, cls, box, keep, self._to_device(gt_cls), box_d.double() * size, self._to_device(gt_off),
                        None if crowd is None else self._to_device(crowd), None if scale is None else self._to_device(scale))
            elif voc:
                hard = self._coco_batch_extras(buf, False)[0]
                acc.add(score, cls, box, keep, self._to_device(gt_cls), box_d.double() * size, self._to_device(gt_off),
                        None if hard is None else self._to_device(hard))
            else:
                acc.add(score, cls, box, keep, self._to_device(gt_cls), box_d.double() * size, self._to_device(gt_off))
            buf.clear()

        with self._weights(weights):
            for sample in samples:
                buf.append(sample)
                if len(buf) == batch_size:
                    flush()
            flush()

    def evaluate(self, samples, batch_size=32, score_thresh=0.05, iou_thresh=0.45, max_dets=100, return_detections=False,
                 precision="bf16", metric="host", scoring="best", protocol="map", weights="live"):
        """Evaluation pass (the reference fetches its val split at models/ssd_model.py:291 and drops it):
        samples = iterable of (image f32 [S,S,3] in [0,1], cls [n], box [n,4] relative cx,cy,w,h) as the loaders yield
        them, or a split of reader-contract samples (getattr(samples, "raw"): decoded uint8 images of any size, COCO top-left
        pixel boxes -- data_loaders RawSplit), which go through the device preprocessing of make_batch_raw.  Network forward,
        scoring/decoding and per-class NMS run on the device.
        metric="host": the kept detections go to utils.metrics.coco_map on the host.
        metric="device": top-max_dets selection, matching and AP run on the device as well (utils.device_map); no dense map
        is copied to the host and nothing synchronises before the result is read.  max_dets <= ops.eval_max_dets().
        Ground-truth boxes are float64(float32 relative box) * input size in both modes.
        Returns coco_map's dict (mAP = AP@[.5:.95], AP50, AP75, per_class); with return_detections also the per-image
        (score, cls, box_px) arrays: all kept detections with "host", the top-max_dets that were scored with "device".
        precision: detect()'s ("bf16" or "mxfp8").
        scoring="best" (default): one label per anchor, as detect().  scoring="all": the SSD detection-output protocol, as
        detections() -- every (anchor, class) pair above score_thresh, per-class NMS, the best max_dets rows per image
        (keep_top_k = max_dets <= ops.detect_max_keep(); the top max_dets rows of a longer list are the same rows); "host"
        then copies the compact rows once per batch.  Any other value raises ValueError.
        protocol="map" (default): the metric above.  protocol="coco": COCO's twelve box metrics (utils.metrics.coco_summary:
        AP, AP50, AP75, AP and AR by area range, AR at 1 / 10 / max_dets detections), with either metric mode; samples may
        carry a fourth element `crowd` (bool [n]); for reader-contract samples areas are in source pixels (area_scale =
        source width x source height / S^2), for prepared samples in evaluation pixels.  Returns coco_summary's dict.
        protocol="voc07" | "voc12": PASCAL VOC's mAP at IoU 0.5 (utils.metrics.voc_map: the 11-point metric of VOC2007, or the
        area under the monotone envelope of VOC2010 onward), with either metric mode; a sample's fourth element is read as the
        boxes' `difficult` flags -- so a COCO sample's crowd flags are treated as difficult.  Returns voc_map's dict (mAP,
        per_class, n_pos).  max_dets <= ops.eval_voc_max_dets() with metric="device".  Any other value raises ValueError.
        weights as detect(): "ema" evaluates the averaged weights (the whole pass inside engine.averaged())."""
        with self._weights(weights):
            return self._evaluate(samples, batch_size, score_thresh, iou_thresh, max_dets, return_detections, precision, metric,
                                  scoring, protocol)

    def _evaluate(self, samples, batch_size, score_thresh, iou_thresh, max_dets, return_detections, precision, metric, scoring,
                  protocol):
        from ..utils.metrics import coco_map
        if protocol not in ("map", "coco", "voc07", "voc12"):
            raise ValueError("protocol must be 'map', 'coco', 'voc07' or 'voc12', not %r" % (protocol,))
        voc = protocol in ("voc07", "voc12")
        if precision not in ("bf16", "mxfp8"):
            raise ValueError("precision must be 'bf16' or 'mxfp8', not %r" % (precision,))
        if scoring not in ("best", "all"):
            raise ValueError("scoring must be 'best' or 'all', not %r" % (scoring,))
        if metric == "device":
            from ..utils.device_map import DeviceCocoAccumulator, DeviceMapAccumulator, DeviceVocAccumulator
            if voc:
                acc = DeviceVocAccumulator(self.cfg.classes - 1, max_dets, self.device, year=protocol[3:])
            else:
                acc = (DeviceCocoAccumulator if protocol == "coco" else DeviceMapAccumulator)(self.cfg.classes - 1, max_dets,
                                                                                              self.device)
            self.evaluate_into(acc, samples, batch_size, score_thresh, iou_thresh, precision, scoring)
            result = acc.result()
            return (result, acc.detections()) if return_detections else result
        if metric != "host":
            raise ValueError("metric must be 'host' or 'device', not %r" % (metric,))
        size = float(self.cfg.input_shape[0])
        raw = bool(getattr(samples, "raw", False))
        dets, gts, buf = [], [], []
        crowds, scales = [], []                                       # protocol="coco": per image; voc: crowds = difficult

        def flush():
            if not buf:
                return
            if protocol == "coco":
                scale = self._coco_batch_extras(buf, raw)[1]
                scales.extend([1.0] * len(buf) if scale is None else scale.tolist())
            if protocol == "coco" or voc:
                crowds.extend(np.asarray(b[3]).astype(bool).reshape(-1) if len(b) > 3 and b[3] is not None
                              else np.zeros(int(np.shape(b[1])[0]), bool) for b in buf)
            if raw:
                x, box_d, counts = self._eval_batch_raw(buf)
                gboxes = np.split(box_d.cpu().numpy(), np.cumsum(counts)[:-1])
            else:
                gboxes = [b[2] for b in buf]
            if scoring == "all":
                if not raw:
                    img = torch.from_numpy(np.stack([b[0] for b in buf], 0)).to(self.device)
                    x = ops.image_prep(((img - 0.5) * 2).contiguous(), normalize=False)
                d = self._detections_prepared(x, score_thresh, iou_thresh, keep_top_k=max_dets, precision=precision)
                n, score, cls, box = d.n_det.cpu().numpy(), d.score.cpu().numpy(), d.cls.cpu().numpy(), d.box.cpu().numpy()
                for i, gcls in enumerate(b[1] for b in buf):
                    dets.append((score[i, :n[i]].copy(), cls[i, :n[i]].copy(), box[i, :n[i]].copy()))
                    gts.append((np.asarray(gcls), np.asarray(gboxes[i], np.float64) * size))
                buf.clear()
                return
            if raw:
                score, cls, box, keep = self._detect_prepared(x, score_thresh, iou_thresh, precision=precision)
            else:
                img = torch.from_numpy(np.stack([b[0] for b in buf], 0)).to(self.device)
                score, cls, box, keep = self.detect((img - 0.5) * 2, score_thresh, iou_thresh, precision=precision)
            score, cls, box, keep = score.cpu().numpy(), cls.cpu().numpy(), box.cpu().numpy(), keep.cpu().numpy().astype(bool)
            for i, gcls in enumerate(b[1] for b in buf):
                k = keep[i]
                dets.append((score[i][k], cls[i][k], box[i][k]))
                gts.append((np.asarray(gcls), np.asarray(gboxes[i], np.float64) * size))     # pixels, like the decoded boxes
            buf.clear()

        for sample in samples:
            buf.append(sample)
            if len(buf) == batch_size:
                flush()
        flush()
        if protocol == "coco":
            from ..utils.metrics import coco_summary
            result = coco_summary(dets, [g + (c,) for g, c in zip(gts, crowds)], max_dets=max_dets,
                                  area_scale=np.asarray(scales, np.float64))
        elif voc:
            from ..utils.metrics import voc_map
            result = voc_map(dets, [g + (c,) for g, c in zip(gts, crowds)], year=protocol[3:], max_dets=max_dets)
        else:
            result = coco_map(dets, gts, max_dets=max_dets)
        return (result, dets) if return_detections else result

    # ------------------------------------------------------------------ checkpoint
    def save(self, path="model_weight.pt", extra=None, collective=True, weights="live"):
        """Weights + Adam moments + step count (the reference's Keras .h5 has weights only, models/ssd_model.py:405-407);
        `extra` (e.g. optimizer iteration counters, epoch) is stored alongside for resume.
        Data parallel: the replicas are identical, rank 0 writes and the others wait for the file (collective=False on
        error paths, where the other ranks may never arrive).
        A model that keeps averaged weights saves them and their update count as well (`ema`, `ema_updates`), so a resumed run
        goes on averaging.  weights="ema": the deployable model instead -- `param` is the average, the optimizer slots and
        the step count are zero and there are no `ema` keys, so it loads into a model that keeps no average (ValueError on a
        model that has none to save)."""
        if weights not in ("live", "ema"):
            raise ValueError("weights must be 'live' or 'ema', not %r" % (weights,))
        if weights == "ema" and self._engine.ema is None:
            raise ValueError("save(weights='ema') on a model without averaged weights")
        rank, world = self._rank_world()
        if rank == 0:
            d = os.path.dirname(path)
            if d:
                os.makedirs(d, exist_ok=True)
            sd = self._engine.state_dict()
            if weights == "ema":
                sd["param"] = sd.pop("ema")
                del sd["ema_updates"]
                sd.update(adam_m=torch.zeros_like(sd["adam_m"]), adam_v=torch.zeros_like(sd["adam_v"]), step=0)
            sd["network"] = self.network.as_dict()
            if extra:
                sd["extra"] = dict(extra)
            torch.save(sd, path)
            logger.info("Model is saved to %s", path)
        if world > 1 and collective:
            torch.distributed.barrier()

    def load(self, path="model_weight.pt"):
        sd = torch.load(path, map_location="cpu", weights_only=True)     # tensors, lists, ints and strings only
        theirs = ops.NetworkSpec.of(sd.get("network"))                   # a checkpoint without the key is an ssd300 one
        if theirs.identity() != self.network.identity():
            raise ValueError("checkpoint %s holds the network %s, this model is %s" % (path, theirs.describe(),
                                                                                     self.network.describe()))
        self._engine.load_state_dict(sd)
        # a checkpoint's average, loaded before this model was told to keep one: enable_ema() (the first step of a run with
        # TrainConfig(ema=...)) takes it from here
        self._loaded_ema = (sd["ema"], sd.get("ema_updates", 0)) if "ema" in sd and self._engine.ema is None else None
        self._version += 1
        self._slot_owner = _RESTORED
        logger.info("Model is loaded from %s", path)
        return sd.get("extra", {})
