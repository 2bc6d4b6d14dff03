"""Entry point with the reference's command line: `python tools/train.py <config.yml>` (reference tools/train.py:
73-81) and the same YAML schema (config/default.yml of the reference; keys read at :23-69).

Run from the repository root as
    python -m ssd_object_detection_amd.tools.train ssd-object-detection_amd/config/default.yml
Data parallel (one process per GPU, RCCL over xGMI):
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 -m ssd_object_detection_amd.tools.train <cfg>
`model.train.batch_size` is then the GLOBAL batch: rank r trains on its image shard of every batch (one micro-batch
of the reference's split_batch loop per rank, models/ssd_model.py:240-256), one log directory is shared, and only rank 0
writes config.json and checkpoints."""
import argparse
import json
import logging
import os

import yaml

logger = logging.getLogger(__name__)

# TrainConfig field  <-  path into the YAML document (the reference's schema, config/default.yml:17-41)
TRAIN_CONFIG_KEYS = {
    "epoch": "model/train/epoch",
    "batch_size": "model/train/batch_size",
    "warmup": "model/warmup/enable",
    "warmup_step": "model/warmup/step",
    "visualization_log_interval": "model/log_interval",
    "split_batch": "model/split_train/enable",
    "split_batch_size": "model/split_train/batch_size",
}


def load_config(yaml_file):
    with open(yaml_file, "r") as f:
        return yaml.safe_load(f)


def cfg_get(config, path):
    node = config
    for key in path.split("/"):
        node = node[key]
    return node


def augment_from_config(config):
    """`data: augment: {enable, seed}` (no reference counterpart) -> ops.AugmentSpec with all four stages, or None when the
    key is absent or enable is false: the default trains without augmentation, as the reference does."""
    section = (config.get("data") or {}).get("augment")
    if not section or not section.get("enable", False):
        return None
    from ..ops import AugmentSpec
    return AugmentSpec(seed=int(section.get("seed", 0) or 0))


VAL_DEFAULTS = dict(every=1, batch_size=32, score_thresh=0.05, iou_thresh=0.45, max_dets=100, num_data=0, precision="bf16")


def val_from_config(config):
    """`model: eval: {enable, every, batch_size, score_thresh, iou_thresh, max_dets, num_data, precision}` (no reference
    counterpart: the reference drops its validation split) -> the `val` dict of TrainConfig, or None when the key is absent or
    enable is false: the default run does not validate, as the reference does not.  The optional key `scoring` ("best": one
    label per anchor, the default when absent; "all": the multi-label detection output, evaluate(scoring="all")) is in the
    dict only when the config gives it, and so is `protocol` ("map", the default when absent: val/mAP, val/AP50, val/AP75;
    "coco": COCO's twelve box metrics, evaluate(protocol="coco"); "voc07" / "voc12": PASCAL VOC's mAP, val/mAP only), and so is
    `weights` ("ema" | "live" | "both": which weights a run with `model: train: ema:` validates; absent = the averaged ones)."""
    section = (config.get("model") or {}).get("eval")
    if not section or not section.get("enable", False):
        return None
    unknown = set(section) - set(VAL_DEFAULTS) - {"enable", "scoring", "protocol", "weights"}
    if unknown:
        raise ValueError("unknown model.eval keys: %s" % sorted(unknown))
    val = {k: type(d)(section.get(k, d)) for k, d in VAL_DEFAULTS.items()}
    if val["precision"] not in ("bf16", "mxfp8"):
        raise ValueError("model.eval.precision must be 'bf16' or 'mxfp8', not %r" % (val["precision"],))
    if val["every"] < 1:
        raise ValueError("model.eval.every must be >= 1")
    if "scoring" in section:
        if section["scoring"] not in ("best", "all"):
            raise ValueError("model.eval.scoring must be 'best' or 'all', not %r" % (section["scoring"],))
        val["scoring"] = str(section["scoring"])
    if "protocol" in section:
        if section["protocol"] not in ("map", "coco", "voc07", "voc12"):
            raise ValueError("model.eval.protocol must be 'map', 'coco', 'voc07' or 'voc12', not %r" % (section["protocol"],))
        val["protocol"] = str(section["protocol"])
    if "weights" in section:
        if section["weights"] not in ("ema", "live", "both"):
            raise ValueError("model.eval.weights must be 'ema', 'live' or 'both', not %r" % (section["weights"],))
        val["weights"] = str(section["weights"])
    return val


def _loss_section(config):
    section = ((config.get("model") or {}).get("train") or {}).get("loss")
    if section is not None and not isinstance(section, dict):
        raise ValueError("model.train.loss must be a mapping, not %r" % (section,))
    return section


def loss_from_config(config):
    """`model: train: loss: {kind, neg_pos_ratio, loc_weight, box}` or `{kind: softmax_focal, gamma, alpha, loc_weight, box,
    background_prior}` (no reference counterpart) -> ops.LossSpec, or None when the section is absent: the default run trains
    with the reference's loss.  kind "multibox" is the SSD paper's loss, "softmax_focal" the softmax focal loss over every
    anchor.  ValueError for an unknown key, an unknown kind, bad values, or a key of another kind: gamma, alpha and
    background_prior belong to softmax_focal alone, neg_pos_ratio to the mined losses, box (smooth_l1 | giou | diou | ciou: the
    box term) to multibox and softmax_focal.  background_prior itself is read by background_prior_from_config."""
    section = _loss_section(config)
    if section is None:
        return None
    focal_keys = {"gamma", "alpha", "background_prior"}
    unknown = set(section) - {"kind", "neg_pos_ratio", "loc_weight", "box"} - focal_keys
    if unknown:
        raise ValueError("unknown model.train.loss keys: %s" % sorted(unknown))
    kind = section.get("kind", "reference")
    foreign = set(section) & ({"neg_pos_ratio"} if kind == "softmax_focal" else focal_keys)
    if kind == "reference":
        foreign |= set(section) & {"box"}
    if foreign:
        raise ValueError("model.train.loss keys %s do not apply to the loss kind %r" % (sorted(foreign), kind))
    from ..ops import LossSpec
    return LossSpec(kind=kind, neg_pos_ratio=section.get("neg_pos_ratio", 3), loc_weight=section.get("loc_weight", 1.0),
                    gamma=section.get("gamma", 2.0), alpha=section.get("alpha", 0.25), box=section.get("box", "smooth_l1"))


def background_prior_from_config(config):
    """`model: train: loss: background_prior` (softmax_focal only: loss_from_config refuses it elsewhere) -> the foreground
    prior pi in (0, 1) for model.set_background_prior, or None when the key is absent.  A run applies it once, when it
    starts from scratch; a resumed run keeps its checkpoint's biases."""
    section = _loss_section(config)
    if section is None or section.get("background_prior") is None:
        return None
    loss_from_config(config)
    pi = section["background_prior"]
    if isinstance(pi, bool) or not isinstance(pi, (int, float)) or not 0.0 < pi < 1.0:
        raise ValueError("model.train.loss.background_prior must be a number in (0, 1), not %r" % (pi,))
    return float(pi)


def ema_from_config(config):
    """`model: train: ema: {enable, decay, warmup}` (no reference counterpart: an exponential moving average of the weights for
    validation, detection and the saved model) -> ops.EmaSpec, or None when the key is absent or enable is false: the default
    run keeps no average.  ValueError for an unknown key or bad values."""
    section = ((config.get("model") or {}).get("train") or {}).get("ema")
    if section is None:
        return None
    if not isinstance(section, dict):
        raise ValueError("model.train.ema must be a mapping, not %r" % (section,))
    unknown = set(section) - {"enable", "decay", "warmup"}
    if unknown:
        raise ValueError("unknown model.train.ema keys: %s" % sorted(unknown, key=str))
    from ..ops import EmaSpec
    spec = EmaSpec(**{k: section[k] for k in ("decay", "warmup") if k in section})     # (bad values raise when disabled too)
    enable = section.get("enable", False)
    if not isinstance(enable, bool):
        raise ValueError("model.train.ema.enable must be true or false, not %r" % (enable,))
    return spec if enable else None


def l2norm_from_config(config):
    """`model: l2norm: {enable, init, eps}` (no reference counterpart: the SSD paper's L2 normalisation of the 38x38 map) ->
    ops.L2NormSpec, or None when the key is absent or enable is false: the default network has no such layer, as the
    reference has none.  ValueError for an unknown key or bad values."""
    section = (config.get("model") or {}).get("l2norm")
    if section is None:
        return None
    if not isinstance(section, dict):
        raise ValueError("model.l2norm must be a mapping, not %r" % (section,))
    unknown = set(section) - {"enable", "init", "eps"}
    if unknown:
        raise ValueError("unknown model.l2norm keys: %s" % sorted(unknown))
    from ..ops import L2NormSpec
    spec = L2NormSpec(**{k: section[k] for k in ("init", "eps") if k in section})      # (bad values raise when disabled too)
    enable = section.get("enable", False)
    if not isinstance(enable, bool):
        raise ValueError("model.l2norm.enable must be true or false, not %r" % (enable,))
    return spec if enable else None


def fp8_inference_from_config(config):
    """`model: fp8_inference: true` (no reference counterpart) -> the model's fp8_inference switch: the VGG-16 SSD300 network then
    plans its block-scaled fp8 inference forward (validation or detection with precision "mxfp8").  False when the key is
    absent.  ValueError for anything but true or false."""
    value = (config.get("model") or {}).get("fp8_inference", False)
    if not isinstance(value, bool):
        raise ValueError("model.fp8_inference must be true or false, not %r" % (value,))
    return value


def network_from_config(config):
    """`model: network: {kind, in_size, batchnorm: {enable, momentum, eps}, precision, dgrad_precision}` (no reference
    counterpart) -> ops.NetworkSpec, or None when the key is absent: the default run builds the reference's 300 x 300 network.
    kind "vgg16_ssd300" (the SSD paper's network) goes together with `model: l2norm:`, as "ssd300" does; the ResNet refuses it.
    kind "mobilenet_v1_ssd300" (MobileNet-v1 SSD300: in_size 300, bf16, no batchnorm) refuses `l2norm` and `fp8_inference`.
    `batchnorm` absent, null or with enable false: no batch normalisation.  ValueError for an unknown key, a section that is
    no mapping or bad values."""
    section = (config.get("model") or {}).get("network")
    if section is None:
        return None
    if not isinstance(section, dict):
        raise ValueError("model.network must be a mapping, not %r" % (section,))
    from ..ops import BatchNormSpec, NetworkSpec
    unknown = set(section) - set(NetworkSpec.FIELDS)
    if unknown:
        raise ValueError("unknown model.network keys: %s" % sorted(unknown, key=str))
    fields = dict(section)
    bn = fields.get("batchnorm")
    if bn is not None:
        if not isinstance(bn, dict):
            raise ValueError("model.network.batchnorm must be a mapping, not %r" % (bn,))
        unknown = set(bn) - {"enable", "momentum", "eps"}
        if unknown:
            raise ValueError("unknown model.network.batchnorm keys: %s" % sorted(unknown, key=str))
        spec = BatchNormSpec(**{k: bn[k] for k in ("momentum", "eps") if k in bn})     # (bad values raise when disabled too)
        enable = bn.get("enable", False)
        if not isinstance(enable, bool):
            raise ValueError("model.network.batchnorm.enable must be true or false, not %r" % (enable,))
        fields["batchnorm"] = spec if enable else None
    return NetworkSpec.of(fields, l2norm=l2norm_from_config(config))


def schedule_from_config(section):
    """`model: train: lr:` -> a learning-rate schedule.  `kind: exponential` (the default when the key is absent: the
    reference's schema) reads `initial`, `decay_step`, `decay_rate`; `kind: piecewise` (no reference counterpart: the SSD
    paper's step schedule) reads `boundaries` and `values`, Keras PiecewiseConstantDecay.  ValueError for an unknown kind or
    missing keys."""
    from .. import optimizers
    if not isinstance(section, dict):
        raise ValueError("model.train.lr must be a mapping, not %r" % (section,))
    kind = section.get("kind", "exponential")
    need = {"exponential": ("initial", "decay_step", "decay_rate"), "piecewise": ("boundaries", "values")}.get(kind)
    if need is None:
        raise ValueError("model.train.lr.kind must be 'exponential' or 'piecewise', not %r" % (kind,))
    missing = [k for k in need if k not in section]
    if missing:
        raise ValueError("model.train.lr (kind %s) lacks %s" % (kind, missing))
    if kind == "piecewise":
        return optimizers.PiecewiseConstantDecay(section["boundaries"], section["values"])
    return optimizers.ExponentialDecay(section["initial"], section["decay_step"], section["decay_rate"])


def clip_from_config(config):
    """`model: train: clip_norm` (no reference counterpart) -> TrainConfig's clip: the per-tensor clip norm, `null` or 0 for no
    clipping; absent = the reference's 0.01.  ValueError for anything but a non-negative number or null."""
    section = (config.get("model") or {}).get("train") or {}
    if "clip_norm" not in section:
        return 0.01
    clip = section["clip_norm"]
    if clip is not None and (isinstance(clip, bool) or not isinstance(clip, (int, float)) or not clip >= 0):
        raise ValueError("model.train.clip_norm must be a number >= 0 or null, not %r" % (clip,))
    return clip


def decode_from_config(config):
    """`data: decode` ("device" | "host") and `data: decode_workers` (host threads of the JPEG entropy decode) -> (decode,
    workers); both optional, absent = ("device", 8).  Read only for `dataset: "coco"` and `"pascal_voc"`: any other dataset gets
    the defaults whatever the keys say.  ValueError for an unknown mode or a worker count that is not a positive integer."""
    data = config.get("data") or {}
    if not (isinstance(data.get("dataset"), str) and data["dataset"].lower() in ("coco", "pascal_voc")):
        return "device", 8
    decode, workers = data.get("decode", "device"), data.get("decode_workers", 8)
    if decode not in ("device", "host"):
        raise ValueError("data.decode must be 'device' or 'host', not %r" % (decode,))
    if isinstance(workers, bool) or not isinstance(workers, int) or workers < 1:
        raise ValueError("data.decode_workers must be a positive integer, not %r" % (workers,))
    return decode, workers


OPTIMIZER_KEYS = {"Adam": {"name", "beta_1", "beta_2", "epsilon"},
                  "SGD": {"name", "momentum", "nesterov", "weight_decay", "decay_bias"}}


def _make_optimizer(section, schedule):
    """`optimizer: {name, ...}`: Adam reads beta_1, beta_2, epsilon; SGD reads momentum, nesterov, weight_decay, decay_bias
    (optimizers.SGD raises ValueError for bad values)."""
    from .. import optimizers
    kinds = {"adam": optimizers.Adam, "sgd": optimizers.SGD}
    kind = kinds.get(section["name"].lower())
    if kind is None:
        raise ValueError                     # reference tools/train.py:47,53
    # the optimizers take **_ as Keras' do: a key they do not read (a misspelt `momentun`) would vanish without a word
    unread = sorted(set(section) - OPTIMIZER_KEYS[kind.__name__])
    if unread:
        logger.warning("optimizer %s does not read the config keys %s: ignored", kind.__name__, unread)
    return kind(schedule, **section)


def _init_distributed():
    """(rank, world); joins the process group when launched under torch.distributed.run."""
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1
    # RCCL needs one GPU per rank ON THIS NODE; with fewer GPUs than local ranks (a one-GPU box rehearsing the multi-rank
    # path) ranks share a device and the exchange goes over gloo.  The count that matters is the node's rank count
    # (LOCAL_WORLD_SIZE, set by torch.distributed.run), not the job's: 2 nodes x 8 GPUs is 16 ranks on 8 devices each.
    n_dev = torch.cuda.device_count()
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    backend = os.environ.get("SSD_DIST_BACKEND", "nccl" if n_dev >= local_world else "gloo")
    logger.info("distributed backend %s (%d ranks, %d on this node, %d devices)", backend, world,
                                     local_world, n_dev)
    if torch.cuda.is_available():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % n_dev)
    if not torch.distributed.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group(backend)
    return torch.distributed.get_rank(), torch.distributed.get_world_size()


def train(config):
    from .. import optimizers
    from ..data_loaders import SSDDataLoader
    from ..models import SSDObjectDetectionModel

    rank, world = _init_distributed()
    data_cfg, model_cfg = config["data"], config["model"]
    subset = data_cfg["mini_batch"]
    network = network_from_config(config)
    decode, decode_workers = decode_from_config(config)
    data = SSDDataLoader(dataset_root=data_cfg["dataset_root"], dataset=data_cfg["dataset"], shuffle=data_cfg["shuffle"],
                         mini_batch=subset["num_data"] if subset["enable"] else 0,
                         input_size=network.in_size if network is not None else 300, decode=decode)
    if isinstance(data_cfg["dataset"], str) and data_cfg["dataset"].lower() == "coco":
        n_cat = len(data.get_names_and_colors()[0])
        if n_cat != data_cfg["num_classes"]:
            raise ValueError("data.num_classes is %r but the annotation files list %d categories" % (data_cfg["num_classes"], n_cat))
    if isinstance(data_cfg["dataset"], str) and data_cfg["dataset"].lower() == "pascal_voc" and data_cfg["num_classes"] != 20:
        raise ValueError("data.num_classes is %r but PASCAL VOC has 20 classes" % (data_cfg["num_classes"],))
    model = SSDObjectDetectionModel(classes=data_cfg["num_classes"], log_dir=model_cfg["log_dir"], distributed=world > 1,
                                    l2norm=l2norm_from_config(config), network=network,
                                    fp8_inference=fp8_inference_from_config(config))
    model.decode_workers = decode_workers
    ema = ema_from_config(config)
    if ema is not None:                      # before a resume: the checkpoint's average goes where the engine keeps one
        model.enable_ema(ema)

    lr, wlr = model_cfg["train"]["lr"], model_cfg["warmup"]["lr"]
    optimizer = _make_optimizer(model_cfg["train"]["optimizer"], schedule_from_config(lr))
    warmup_optimizer = _make_optimizer(model_cfg["warmup"]["optimizer"],
                                       optimizers.PolynomialDecay(wlr["start"], model_cfg["warmup"]["step"], wlr["end"]))

    # resume (the reference has load() but no resume path): `model.resume: <checkpoint>` in the YAML
    # restores weights, Adam moments, step counters and continues with the epoch after the saved one
    start_epoch = 0
    resume = model_cfg.get("resume")
    if resume:
        extra = model.load(resume)
        optimizer.iterations = int(extra.get("iterations", model.get_engine().step_count))
        warmup_optimizer.iterations = int(extra.get("warmup_iterations", 0))
        start_epoch = int(extra.get("epoch", 0))
        logger.info("Resuming from %s at epoch %d (optimizer step %d)", resume, start_epoch, optimizer.iterations)
    prior = background_prior_from_config(config)
    if prior is not None and not resume:     # a run from scratch: the conf biases start at the prior (a resumed run keeps its own)
        model.set_background_prior(prior)

    if rank == 0:                            # the run's configuration next to its logs (reference tools/train.py:55-56)
        os.makedirs(model.get_log_dir(), exist_ok=True)
        text = json.dumps(config, sort_keys=True, indent=4, separators=(",", ":"))
        with open(os.path.join(model.get_log_dir(), "config.json"), "w") as f:
            f.write(text)

    fields = {name: cfg_get(config, path) for name, path in TRAIN_CONFIG_KEYS.items()}
    fields.update(optimizer=optimizer, warmup_optimizer=warmup_optimizer, start_epoch=start_epoch,
                  augment=augment_from_config(config), val=val_from_config(config), loss=loss_from_config(config),
                  clip=clip_from_config(config), ema=ema)
    model.train(data_loader=data, cfg=SSDObjectDetectionModel.TrainConfig(**fields))
    model.save(os.path.join(model.get_log_dir(), model_cfg["save"]))      # rank 0 writes; the others wait
    return model


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO)
    parser = argparse.ArgumentParser(description="train ssd model")
    parser.add_argument("config", type=str, help="yaml config file")
    args = parser.parse_args()
    train(load_config(args.config))
