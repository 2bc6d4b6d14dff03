"""CPU: the momentum SGD recipe without a device -- the float64 oracle's known answers, optimizers.SGD and
PiecewiseConstantDecay, the YAML parsing of tools/train.py, and the host-side refusals of ssd_sgd_momentum_step."""
import copy
import ctypes
import os

import numpy as np
import pytest

from tests.sgd_oracle import sgd_momentum_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- oracle -----------------------------------------------------------------------------------------------------------
def two_steps(**kw):
    p, v = np.array([1.0]), np.array([0.0])
    out = []
    for _ in range(2):
        p, v = sgd_momentum_step(p, np.array([1.0]), v, 0.125, 0.5, **kw)
        out += [float(p[0]), float(v[0])]
    return out


def test_oracle_known_answers():
    """p = 1, g = 1, v = 0, lr = 1/8, momentum = 1/2, two steps by hand (every number is exact in binary)."""
    # v1 = -1/8, p1 = 7/8;  v2 = -1/16 - 1/8 = -3/16, p2 = 11/16
    assert two_steps() == [0.875, -0.125, 0.6875, -0.1875]
    # p1 = 1 + (-1/16 - 1/8) = 13/16;  v2 = -3/16, p2 = 13/16 + (-3/32 - 1/8) = 19/32
    assert two_steps(nesterov=True) == [0.8125, -0.125, 0.59375, -0.1875]
    # decay 1/2: ge1 = 3/2, v1 = -3/16, p1 = 13/16;  ge2 = 1 + 13/32 = 45/32, v2 = -3/32 - 45/256 = -69/256, p2 = 139/256
    assert two_steps(decay=0.5) == [0.8125, -0.1875, 0.54296875, -0.26953125]
    # sc scales the gradient, not the decay term: ge = 1 * 1/2 + 1/2 * 1 = 1
    p, v = sgd_momentum_step([1.0], [1.0], [0.0], 0.125, 0.5, sc=0.5, decay=0.5)
    assert (float(p[0]), float(v[0])) == (0.875, -0.125)


def test_oracle_without_momentum_is_plain_sgd():
    rng = np.random.default_rng(0)
    p, g, v = rng.normal(size=100), rng.normal(size=100), rng.normal(size=100)
    sc = rng.uniform(0.1, 1.0, size=100)
    for nesterov in (False, True):
        p1, v1 = sgd_momentum_step(p, g, v, 0.01, 0.0, nesterov=nesterov, sc=sc)
        assert np.array_equal(p1, p - 0.01 * (g * sc)) and np.array_equal(v1, -0.01 * (g * sc))


# ---- optimizers --------------------------------------------------------------------------------------------------------
def test_sgd_attributes_and_refusals():
    from ssd_object_detection_amd import optimizers
    o = optimizers.SGD(momentum=0.9)
    assert o.momentum == 0.9 and o.nesterov is False and o.weight_decay == 0.0 and o.decay_bias is False and o.name == "SGD"
    assert o.uses_slots and o.lr() == 0.01 and o.iterations == 0
    o = optimizers.SGD(1e-3, momentum=0.5, nesterov=True, weight_decay=5e-4, decay_bias=True, name="sgd", beta_1=0.9)
    assert (o.momentum, o.nesterov, o.weight_decay, o.decay_bias, o.name, o.lr()) == (0.5, True, 5e-4, True, "sgd", 1e-3)
    assert not optimizers.SGD().uses_slots                                  # the defaults: plain SGD, no slot
    o = optimizers.SGD(momentum=np.float32(0.5), weight_decay=np.float64(1e-4))      # numpy scalars are numbers
    assert (o.momentum, o.weight_decay) == (0.5, 1e-4) and type(o.momentum) is float
    assert optimizers.SGD(weight_decay=1e-4).uses_slots
    for bad in (dict(momentum=1.0), dict(momentum=-0.1), dict(momentum=float("nan")), dict(momentum="0.9"),
                dict(weight_decay=-1e-4), dict(weight_decay=None), dict(nesterov=1), dict(nesterov="true"),
                dict(decay_bias=0), dict(decay_bias=None)):
        with pytest.raises(ValueError):
            optimizers.SGD(**bad)


def test_piecewise_constant_decay():
    from ssd_object_detection_amd.optimizers import PiecewiseConstantDecay, SGD
    s = PiecewiseConstantDecay([10, 20], [1e-3, 1e-4, 1e-5])
    assert [s(t) for t in (0, 9, 10, 11, 19, 20, 21, 1000)] == [1e-3, 1e-3, 1e-3, 1e-4, 1e-4, 1e-4, 1e-5, 1e-5]
    assert s(10.0) == 1e-3 and s(np.nextafter(10.0, 11.0)) == 1e-4 and s(np.nextafter(10.0, 9.0)) == 1e-3
    assert PiecewiseConstantDecay([], [0.5])(7) == 0.5
    opt = SGD(s, momentum=0.9)
    opt.iterations = 11
    assert opt.lr() == 1e-4
    for b, v in (([10, 20], [1.0, 2.0]), ([10], [1.0]), ([], []), ([10, 10], [1.0, 2.0, 3.0]), ([20, 10], [1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            PiecewiseConstantDecay(b, v)


# ---- YAML --------------------------------------------------------------------------------------------------------------
def default_config():
    from ssd_object_detection_amd.tools import train as T
    return T.load_config(os.path.join(os.path.dirname(T.__file__), "..", "config", "default.yml"))


def test_default_config_is_unchanged():
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.tools import train as T
    cfg = default_config()
    sched = T.schedule_from_config(cfg["model"]["train"]["lr"])
    assert isinstance(sched, optimizers.ExponentialDecay)
    assert (sched.initial_learning_rate, sched.decay_steps, sched.decay_rate) == (0.001, 100, 0.99)
    opt = T._make_optimizer(cfg["model"]["train"]["optimizer"], sched)
    assert isinstance(opt, optimizers.Adam) and (opt.beta_1, opt.beta_2, opt.epsilon) == (0.9, 0.999, 1e-7)
    assert isinstance(T._make_optimizer(cfg["model"]["warmup"]["optimizer"], 1e-3), optimizers.Adam)
    assert T.clip_from_config(cfg) == 0.01
    assert "clip_norm" not in cfg["model"]["train"] and "kind" not in cfg["model"]["train"]["lr"]


def test_yaml_optimizer_schedule_and_clip():
    import yaml
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.tools import train as T
    doc = yaml.safe_load("""
model:
  train:
    optimizer: {name: SGD, momentum: 0.9, nesterov: true, weight_decay: 0.0005, decay_bias: false}
    clip_norm: null
    lr: {kind: piecewise, boundaries: [80000, 100000], values: [0.001, 0.0001, 0.00001]}
""")
    tr = doc["model"]["train"]
    sched = T.schedule_from_config(tr["lr"])
    assert isinstance(sched, optimizers.PiecewiseConstantDecay)
    assert (sched(80000), sched(80001), sched(100001)) == (1e-3, 1e-4, 1e-5)
    opt = T._make_optimizer(tr["optimizer"], sched)
    assert isinstance(opt, optimizers.SGD)
    assert (opt.momentum, opt.nesterov, opt.weight_decay, opt.decay_bias, opt.lr()) == (0.9, True, 5e-4, False, 1e-3)
    assert T.clip_from_config(doc) is None
    plain = T._make_optimizer({"name": "sgd"}, 0.01)
    assert isinstance(plain, optimizers.SGD) and not plain.uses_slots
    with pytest.raises(ValueError):
        T._make_optimizer({"name": "SGD", "momentum": 1.5}, 0.01)
    with pytest.raises(ValueError):
        T._make_optimizer({"name": "SGD", "nesterov": "yes"}, 0.01)
    # clip_norm: a number, 0, null; refusals
    for given, want in ((0.05, 0.05), (0, 0), (None, None), (1, 1)):
        assert T.clip_from_config({"model": {"train": {"clip_norm": given}}}) == want
    for bad in (-0.01, "0.01", True, [0.01]):
        with pytest.raises(ValueError):
            T.clip_from_config({"model": {"train": {"clip_norm": bad}}})
    # lr: exponential by name, unknown kind, missing keys
    e = T.schedule_from_config({"kind": "exponential", "initial": 0.01, "decay_step": 10, "decay_rate": 0.5})
    assert isinstance(e, optimizers.ExponentialDecay) and e(10) == 0.005
    for bad in ({"kind": "cosine", "initial": 0.01}, {"kind": "piecewise", "boundaries": [1]}, {"kind": "piecewise", "values": [1]},
                {"initial": 0.01, "decay_step": 10}, {"kind": "piecewise", "boundaries": [5, 5], "values": [1, 2, 3]}, [0.001]):
        with pytest.raises(ValueError):
            T.schedule_from_config(copy.deepcopy(bad))


def test_train_config_clip():
    pytest.importorskip("torch")
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    TC = SSDObjectDetectionModel.TrainConfig
    assert TC(1, 4, None, warmup=False).clip == 0.01
    assert TC(1, 4, None, warmup=False, clip=0.05).clip == 0.05
    assert TC(1, 4, None, warmup=False, clip=None).clip == 0.0 and TC(1, 4, None, warmup=False, clip=0).clip == 0.0
    for bad in (-1.0, "0.01", True):
        with pytest.raises(ValueError):
            TC(1, 4, None, warmup=False, clip=bad)


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_sgd_momentum_step_refuses_on_the_host():
    """Every refusal of include/ssd_hip.h comes back as SSD_ERR_VALUE before anything touches a device (the pointers are never
    dereferenced on these paths)."""
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    blk = L.ssd_opt_block_elems()
    d = ctypes.c_void_p(0x1000)
    good = dict(param=d, grad=d, velocity=d, bf16=d, n=2 * blk, bt=d, scale=d, decay=d, gs=1.0, lr=0.01, mom=0.9, nesterov=0)

    def call(**kw):
        a = dict(good, **kw)
        return L.ssd_sgd_momentum_step(a["param"], a["grad"], a["velocity"], a["bf16"], a["n"], a["bt"], a["scale"], a["decay"],
                                       a["gs"], a["lr"], a["mom"], a["nesterov"], None)

    for bad in (dict(param=None), dict(grad=None), dict(velocity=None), dict(n=0), dict(n=-blk), dict(n=blk + 4), dict(n=blk - 1),
                dict(bt=None), dict(bt=None, decay=None), dict(bt=None, scale=None),
                dict(mom=1.0), dict(mom=-0.5), dict(mom=1.5), dict(mom=float("nan")),
                dict(nesterov=2), dict(nesterov=-1)):
        assert call(**bad) == _lib.SSD_ERR_VALUE, bad


def test_unread_optimizer_keys_are_reported(caplog):
    """The optimizers keep Keras' **kwargs, so a misspelt key cannot raise; tools/train.py names it in a warning instead."""
    from ssd_object_detection_amd.tools import train as T
    with caplog.at_level("WARNING"):
        opt = T._make_optimizer({"name": "SGD", "momentun": 0.9}, 0.01)
    assert not opt.uses_slots
    assert [r.getMessage() for r in caplog.records if "momentun" in r.getMessage()]
    caplog.clear()
    cfg = default_config()
    with caplog.at_level("WARNING"):
        T._make_optimizer(cfg["model"]["train"]["optimizer"], 1e-3)
        T._make_optimizer(cfg["model"]["warmup"]["optimizer"], 1e-3)
        T._make_optimizer({"name": "SGD", "momentum": 0.9, "nesterov": True, "weight_decay": 5e-4, "decay_bias": False}, 0.01)
    assert not caplog.records
