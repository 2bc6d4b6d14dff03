"""COCO-style mAP accumulated on the device: utils.metrics.coco_map without the dense maps on
the host and without its Python loops.

Per evaluated batch `add` enqueues one ssd_eval_match launch (top-max_dets detections per image + greedy matching at the ten
IoU thresholds) behind ssd_score_decode + ssd_nms and keeps its small record tensors; nothing synchronises.  `result` sorts
all rows by (class, score desc, image, rank) -- a stable device sort of a 64-bit key over rows that are already in (image,
rank) order --, runs ssd_eval_ap and reads one [C, 11] table back.  The definition, and the oracle of both kernels, is
utils.metrics.coco_map.  DeviceCocoAccumulator is the same shape for COCO's twelve metrics (utils.metrics.coco_summary) on
ssd_eval_match_coco / ssd_eval_ap_coco, and DeviceVocAccumulator for PASCAL VOC's AP (utils.metrics.voc_map) on
ssd_eval_match_voc / ssd_eval_ap_voc."""
import numpy as np
import torch

from .. import ops
from .metrics import COCO_AREA_RANGES, VOC_YEARS, coco_summary_from_tables, map_from_ap_table, voc_result


class DeviceMapAccumulator:
    def __init__(self, classes, max_dets=100, device="cuda"):
        """classes: number of object classes (ids 0 .. classes-1); max_dets: detections scored per image."""
        if not 1 <= int(max_dets) <= ops.eval_max_dets():
            raise ValueError("max_dets must be in 1 .. %d, not %r" % (ops.eval_max_dets(), max_dets))
        self.classes, self.max_dets, self.device = int(classes), int(max_dets), torch.device(device)
        self._records, self._gt_cls = [], []

    def add(self, score, cls, box, keep, gt_cls, gt_box, gt_off):
        """One batch: score f32 [B,A], cls i32 [B,A], box f32 [B,A,4] pixels, keep u8 [B,A] (ops.score_decode + ops.nms);
        ground truth as CSR: gt_cls i32 [total], gt_box f64 [total,4] (cx,cy,w,h pixels), gt_off i32 [B+1].  Enqueue only."""
        self._records.append(ops.eval_match(score, cls, box, keep, gt_cls, gt_box, gt_off, self.max_dets))
        self._gt_cls.append(gt_cls)

    def _cat(self, i):
        return torch.cat([r[i] for r in self._records], 0)

    def detections(self):
        """Per image (score [k], cls [k], box [k,4]) numpy arrays: the top-max_dets kept detections that were scored."""
        if not self._records:
            return []
        n = self._cat(0).cpu().numpy()
        score, cls, box = self._cat(1).cpu().numpy(), self._cat(2).cpu().numpy(), self._cat(3).cpu().numpy()
        return [(score[i, :k].copy(), cls[i, :k].copy(), box[i, :k].copy()) for i, k in enumerate(n)]

    def result(self):
        """The dict utils.metrics.coco_map returns for the same detections and ground truths."""
        C, dev = self.classes, self.device
        if not self._records:
            return map_from_ap_table({})
        score, cls, flags = self._cat(1).reshape(-1), self._cat(2).reshape(-1), self._cat(4).reshape(-1)
        # empty slots (class -1) sort behind every class; (score + 0.0) orders -0 as +0, as the comparison of floats does
        bits = (score + 0.0).view(torch.int32).to(torch.int64)
        ordered = torch.where(bits < 0, bits ^ 0x7fffffff, bits)               # signed order of the int32 = order of the floats
        cls_key = torch.where(cls < 0, torch.full_like(cls, C), cls).to(torch.int64)
        key = (cls_key << 32) | (0x7fffffff - ordered)                         # descending score inside a class
        order = torch.sort(key, stable=True).indices                           # rows are in (image, rank) order already
        flags_sorted = flags[order].contiguous()
        per_class = torch.bincount(cls_key, minlength=C + 1)[:C + 1]
        seg_off = torch.zeros((C + 1,), dtype=torch.int32, device=dev)
        seg_off[1:] = torch.cumsum(per_class[:C], 0).to(torch.int32)
        gt = torch.cat(self._gt_cls, 0).to(torch.int64)
        gt = gt[(gt >= 0) & (gt < C)]
        n_gt = torch.bincount(gt, minlength=C)[:C].to(torch.int32)
        ap = ops.eval_ap(flags_sorted, seg_off, n_gt)
        host = torch.cat([ap, n_gt.to(torch.float64).reshape(C, 1)], 1).cpu().numpy()      # the one device-to-host read
        return map_from_ap_table({c: host[c, :10].tolist() for c in np.nonzero(host[:, 10] > 0)[0].tolist()})


class DeviceCocoAccumulator:
    """COCO's twelve box metrics on the device: utils.metrics.coco_summary as DeviceMapAccumulator is coco_map.  `add` enqueues
    one ssd_eval_match_coco launch per batch (area ranges, crowd boxes, positions) and nothing synchronises; `result` sorts the
    rows as DeviceMapAccumulator does, counts the non-ignored ground truths per (area range, class) from the kernel's gt_ignore
    bits, runs ssd_eval_ap_coco and reads one table back."""
    protocol = "coco"

    def __init__(self, classes, max_dets=100, device="cuda", area_ranges=COCO_AREA_RANGES):
        if not 1 <= int(max_dets) <= ops.eval_max_dets():
            raise ValueError("max_dets must be in 1 .. %d, not %r" % (ops.eval_max_dets(), max_dets))
        self.classes, self.max_dets, self.device = int(classes), int(max_dets), torch.device(device)
        self.area_ranges = tuple((float(lo), float(hi)) for lo, hi in area_ranges)
        if len(self.area_ranges) != 4:
            raise ValueError("area_ranges must be four (lo, hi) pairs")
        self._records, self._gt_cls = [], []

    def add(self, score, cls, box, keep, gt_cls, gt_box, gt_off, gt_crowd=None, area_scale=None):
        """DeviceMapAccumulator.add's batch, and gt_crowd u8 [total] (None: no crowd box), area_scale f64 [B] (None: 1): per
        image (source width x source height) / (S x S).  Enqueue only."""
        self._records.append(ops.eval_match_coco(score, cls, box, keep, gt_cls, gt_box, gt_off, self.max_dets, gt_crowd,
                                                 area_scale, self.area_ranges))
        self._gt_cls.append(gt_cls)

    def _cat(self, i):
        return torch.cat([r[i] for r in self._records], 0)

    def detections(self):
        """Per image (score [k], cls [k], box [k,4]) numpy arrays: the top-max_dets kept detections that were scored."""
        if not self._records:
            return []
        n = self._cat(0).cpu().numpy()
        score, cls, box = self._cat(1).cpu().numpy(), self._cat(2).cpu().numpy(), self._cat(3).cpu().numpy()
        return [(score[i, :k].copy(), cls[i, :k].copy(), box[i, :k].copy()) for i, k in enumerate(n)]

    def result(self):
        """The dict utils.metrics.coco_summary returns for the same detections and ground truths."""
        C, dev = self.classes, self.device
        if not self._records:
            return coco_summary_from_tables(np.zeros((C, 4, 10)), np.zeros((C, 4, 3, 10), np.int32), np.zeros((4, C), np.int64))
        score, cls = self._cat(1).reshape(-1), self._cat(2).reshape(-1)
        tp, ig, pos = self._cat(5).reshape(-1, 4), self._cat(6).reshape(-1, 4), self._cat(7).reshape(-1)
        # DeviceMapAccumulator's key: (class, score desc), stable over rows in (image, rank) order; empty slots last
        bits = (score + 0.0).view(torch.int32).to(torch.int64)
        ordered = torch.where(bits < 0, bits ^ 0x7fffffff, bits)
        cls_key = torch.where(cls < 0, torch.full_like(cls, C), cls).to(torch.int64)
        key = (cls_key << 32) | (0x7fffffff - ordered)
        order = torch.sort(key, stable=True).indices
        per_class = torch.bincount(cls_key, minlength=C + 1)[:C + 1]
        seg_off = torch.zeros((C + 1,), dtype=torch.int32, device=dev)
        seg_off[1:] = torch.cumsum(per_class[:C], 0).to(torch.int32)
        # non-ignored ground truths per (range, class): one bincount over the keys a * C + class, ignored ones in a spare bin
        gt = torch.cat(self._gt_cls, 0).to(torch.int64)
        ign = self._cat(8).to(torch.int64)
        a = torch.arange(4, device=dev, dtype=torch.int64).reshape(4, 1)
        live = (((ign.reshape(1, -1) >> a) & 1) == 0) & ((gt >= 0) & (gt < C)).reshape(1, -1)
        n_gt = torch.bincount(torch.where(live, a * C + gt.reshape(1, -1), 4 * C).reshape(-1), minlength=4 * C + 1)[:4 * C]
        n_gt = n_gt.to(torch.int32).reshape(4, C).contiguous()
        ap, cnt = ops.eval_ap_coco(tp[order].contiguous(), ig[order].contiguous(), pos[order].contiguous(), seg_off, n_gt,
                                   self.max_dets)
        host = torch.cat([ap.reshape(-1), cnt.reshape(-1).to(torch.float64), n_gt.reshape(-1).to(torch.float64)]).cpu().numpy()
        ap_h = host[:C * 40].reshape(C, 4, 10)                                 # the one device-to-host read
        cnt_h = np.rint(host[C * 40:C * 160]).astype(np.int64).reshape(C, 4, 3, 10)
        return coco_summary_from_tables(ap_h, cnt_h, np.rint(host[C * 160:]).astype(np.int64).reshape(4, C))


class DeviceVocAccumulator:
    """PASCAL VOC's mAP on the device: utils.metrics.voc_map as DeviceMapAccumulator is coco_map.  `add` enqueues one
    ssd_eval_match_voc launch per batch and nothing synchronises; `result` sorts the rows as DeviceMapAccumulator does, counts
    the non-difficult boxes per class, runs ssd_eval_ap_voc and reads one table back."""
    protocol = "voc"

    def __init__(self, classes, max_dets=100, device="cuda", year="07", iou_thresh=0.5):
        if not 1 <= int(max_dets) <= ops.eval_voc_max_dets():
            raise ValueError("max_dets must be in 1 .. %d, not %r" % (ops.eval_voc_max_dets(), max_dets))
        if year not in VOC_YEARS:
            raise ValueError("year must be '07' or '12', not %r" % (year,))
        if not (np.isfinite(iou_thresh) and iou_thresh > 0):
            raise ValueError("iou_thresh must be finite and > 0, not %r" % (iou_thresh,))
        self.classes, self.max_dets, self.device = int(classes), int(max_dets), torch.device(device)
        self.year, self.iou_thresh = year, float(iou_thresh)
        self._records, self._gt_cls, self._gt_difficult = [], [], []

    def add(self, score, cls, box, keep, gt_cls, gt_box, gt_off, gt_difficult=None):
        """DeviceMapAccumulator.add's batch, and gt_difficult u8 [total] (None: no difficult box).  Enqueue only."""
        self._records.append(ops.eval_match_voc(score, cls, box, keep, gt_cls, gt_box, gt_off, self.max_dets, gt_difficult,
                                                self.iou_thresh))
        self._gt_cls.append(gt_cls)
        self._gt_difficult.append(torch.zeros_like(gt_cls, dtype=torch.uint8) if gt_difficult is None else gt_difficult)

    def _cat(self, i):
        return torch.cat([r[i] for r in self._records], 0)

    def detections(self):
        """Per image (score [k], cls [k], box [k,4]) numpy arrays: the top-max_dets kept detections that were scored."""
        if not self._records:
            return []
        n = self._cat(0).cpu().numpy()
        score, cls, box = self._cat(1).cpu().numpy(), self._cat(2).cpu().numpy(), self._cat(3).cpu().numpy()
        return [(score[i, :k].copy(), cls[i, :k].copy(), box[i, :k].copy()) for i, k in enumerate(n)]

    def result(self):
        """The dict utils.metrics.voc_map returns for the same detections and ground truths."""
        C, dev = self.classes, self.device
        if not self._records:
            return voc_result({}, {})
        score, cls, flags = self._cat(1).reshape(-1), self._cat(2).reshape(-1), self._cat(4).reshape(-1)
        # DeviceMapAccumulator's key: (class, score desc), stable over rows in (image, rank) order; empty slots last
        bits = (score + 0.0).view(torch.int32).to(torch.int64)
        ordered = torch.where(bits < 0, bits ^ 0x7fffffff, bits)
        cls_key = torch.where(cls < 0, torch.full_like(cls, C), cls).to(torch.int64)
        key = (cls_key << 32) | (0x7fffffff - ordered)
        order = torch.sort(key, stable=True).indices
        per_class = torch.bincount(cls_key, minlength=C + 1)[:C + 1]
        seg_off = torch.zeros((C + 1,), dtype=torch.int32, device=dev)
        seg_off[1:] = torch.cumsum(per_class[:C], 0).to(torch.int32)
        gt = torch.cat(self._gt_cls, 0).to(torch.int64)
        gt = gt[(gt >= 0) & (gt < C) & (torch.cat(self._gt_difficult, 0) == 0)]
        n_pos = torch.bincount(gt, minlength=C)[:C].to(torch.int32)
        ap = ops.eval_ap_voc(flags[order].contiguous(), seg_off, n_pos, self.year)
        host = torch.stack([ap, n_pos.to(torch.float64)], 1).cpu().numpy()                  # the one device-to-host read
        live = np.nonzero(host[:, 1] > 0)[0].tolist()
        return voc_result({c: host[c, 0] for c in live}, {c: int(host[c, 1]) for c in live})
