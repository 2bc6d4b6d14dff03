"""CPU: the exponential moving average of the weights without a device -- ops.EmaSpec and its per-step factor against
tests/ema_oracle.py, the YAML section of tools/train.py, TrainConfig(ema=...) and the host-side refusals of ssd_ema_step."""
import ctypes

import numpy as np
import pytest

from tests import ema_oracle as E


# ---- oracle -----------------------------------------------------------------------------------------------------------
def test_oracle_known_answers():
    """e = 1, p = 3, om = 1/4: 1 + (3 - 1) / 4 = 3/2; then om = 1/2 towards p = -1/2: 3/2 - 1 = 1/2 (all exact in binary)."""
    e = E.ema_update([1.0], [3.0], np.float32(0.25))
    assert e.tolist() == [1.5]
    assert E.ema_update(e, [-0.5], np.float32(0.5)).tolist() == [0.5]
    assert E.ema_update([2.0, -0.0], [7.0, 5.0], np.float32(1.0)).tolist() == [7.0, 5.0]
    assert E.ema_update([2.0, -3.0], [7.0, 5.0], np.float32(0.0)).tolist() == [2.0, -3.0]
    # TF's rule: (1 + t) / (10 + t) until it crosses the decay
    assert [E.decay_at(t, 0.9998) for t in (0, 1, 8, 90)] == [0.1, 2.0 / 11.0, 0.5, 0.91]
    assert E.decay_at(10 ** 6, 0.9998) == 0.9998 and E.decay_at(0, 0.9998, warmup=False) == 0.9998
    e, bound = E.ema_chain([1.0], [[3.0], [3.0]], 0.5, warmup=False)
    assert e.tolist() == [2.5] and bound.tolist() == [2 * 4 * E.U * (3.0 + 2.5)]


# ---- spec -------------------------------------------------------------------------------------------------------------
def test_ema_spec_of():
    pytest.importorskip("torch")
    from ssd_object_detection_amd import ops
    assert ops.EmaSpec.of(None) is None
    s = ops.EmaSpec.of(0.99)
    assert (s.decay, s.warmup) == (0.99, True) and type(s.decay) is float
    assert ops.EmaSpec.of(s) is s
    d = ops.EmaSpec.of({"decay": 0.5, "warmup": False})
    assert (d.decay, d.warmup) == (0.5, False)
    assert (ops.EmaSpec.of({}).decay, ops.EmaSpec.of({}).warmup) == (0.9998, True) == (ops.EmaSpec().decay, ops.EmaSpec().warmup)
    assert ops.EmaSpec.of(np.float32(0.5)).decay == 0.5
    assert "0.5" in repr(d)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), True, False, "0.99", [0.99], {"decay": 2.0}, {"decay": 0.9, "warmup": 1},
                {"decay": 0.9, "momentum": 0.1}, {"warm_up": True}):
        with pytest.raises(ValueError):
            ops.EmaSpec.of(bad)
    with pytest.raises(ValueError):
        ops.EmaSpec(decay=1.0)


@pytest.mark.parametrize("decay", [0.9998, 0.5, 0.9])
def test_factor_sequence_equals_the_oracle(decay):
    """d_t for t = 0..50 and on both sides of the crossover (1 + t) / (10 + t) = decay, warm-up on and off; the factor handed to
    the kernel is float32(1 - d_t) with the difference taken in double."""
    pytest.importorskip("torch")
    from ssd_object_detection_amd import ops
    cross = next(t for t in range(10 ** 6) if (1.0 + t) / (10.0 + t) >= decay)      # the crossover with the constant decay
    ts = list(range(51)) + [max(cross - 1, 0), cross, cross + 1, 10 * cross + 7, 10 ** 7]
    for warmup in (True, False):
        spec = ops.EmaSpec(decay, warmup)
        for t in ts:
            assert spec.decay_at(t) == E.decay_at(t, decay, warmup), (t, warmup)
            om = spec.one_minus_decay(t)
            assert type(om) is float and np.float32(om) == E.one_minus_decay(t, decay, warmup) and float(np.float32(om)) == om
            assert 0.0 < om < 1.0
    warm = ops.EmaSpec(decay, True)
    assert warm.decay_at(0) == min(decay, 0.1) and warm.decay_at(10 * cross + 7) == decay
    if cross > 0:
        assert warm.decay_at(cross - 1) < decay
    with pytest.raises(ValueError):
        warm.decay_at(-1)


# ---- YAML and TrainConfig ---------------------------------------------------------------------------------------------
def test_yaml_section():
    pytest.importorskip("torch")
    import yaml
    from ssd_object_detection_amd.tools import train as T
    doc = yaml.safe_load("""
model:
  train:
    ema: {enable: true, decay: 0.999, warmup: false}
""")
    s = T.ema_from_config(doc)
    assert (s.decay, s.warmup) == (0.999, False)
    assert T.ema_from_config({"model": {"train": {"ema": {"enable": True}}}}).decay == 0.9998
    assert T.ema_from_config({"model": {"train": {}}}) is None and T.ema_from_config({"model": {}}) is None
    assert T.ema_from_config({"model": {"train": {"ema": {"enable": False, "decay": 0.9}}}}) is None
    assert T.ema_from_config({"model": {"train": {"ema": {"decay": 0.9}}}}) is None          # enable defaults to false
    for bad in ({"enable": True, "decy": 0.9}, {"enable": True, "decay": 1.0}, {"enable": False, "decay": 0.0},
                {"enable": "yes"}, {"enable": True, "warmup": "no"}, 0.9998, [True]):
        with pytest.raises(ValueError):
            T.ema_from_config({"model": {"train": {"ema": bad}}})
    # the shipped default keeps no average, and validation's `weights` key parses
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = T.load_config(os.path.join(root, "ssd-object-detection_amd", "config", "default.yml"))
    assert T.ema_from_config(cfg) is None
    assert "weights" not in T.val_from_config({"model": {"eval": {"enable": True}}})
    for w in ("ema", "live", "both"):
        assert T.val_from_config({"model": {"eval": {"enable": True, "weights": w}}})["weights"] == w
    with pytest.raises(ValueError):
        T.val_from_config({"model": {"eval": {"enable": True, "weights": "average"}}})


def test_train_config_ema():
    pytest.importorskip("torch")
    from ssd_object_detection_amd import ops
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    TC = SSDObjectDetectionModel.TrainConfig
    assert TC(1, 4, None, warmup=False).ema is None
    assert TC(1, 4, None, warmup=False, ema=0.999).ema.decay == 0.999
    spec = ops.EmaSpec(0.5, warmup=False)
    assert TC(1, 4, None, warmup=False, ema=spec).ema is spec
    got = TC(1, 4, None, warmup=False, ema=dict(decay=0.9, warmup=False)).ema
    assert (got.decay, got.warmup) == (0.9, False)
    for bad in (1.0, True, "0.9", dict(decay=0.9, extra=1)):
        with pytest.raises(ValueError):
            TC(1, 4, None, warmup=False, ema=bad)
    assert TC(1, 4, None, warmup=False, val=dict(weights="both")).val["weights"] == "both"
    assert "weights" not in TC(1, 4, None, warmup=False, val=dict(every=2)).val
    with pytest.raises(ValueError):
        TC(1, 4, None, warmup=False, val=dict(weights="average"))


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_ema_step_refuses_on_the_host():
    """Every refusal of include/ssd_hip.h comes back as SSD_ERR_VALUE before anything touches a device (the pointers are never
    dereferenced on these paths)."""
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    blk = L.ssd_opt_block_elems()
    n = 2 * blk
    e, p = 0x100000, 0x100000 + 4 * n                                 # adjacent, not overlapping
    good = dict(ema=e, param=p, n=n, om=0.5)

    def call(**kw):
        a = dict(good, **kw)
        return L.ssd_ema_step(ctypes.c_void_p(a["ema"]), ctypes.c_void_p(a["param"]), a["n"], a["om"], None)

    for bad in (dict(ema=None), dict(param=None), dict(n=0), dict(n=-blk), dict(n=blk + 4), dict(n=blk - 1),
                dict(om=float("nan")), dict(om=-1e-6), dict(om=1.0 + 1e-6), dict(om=float("inf")),
                dict(param=e), dict(param=e + 4), dict(param=e + 4 * n - 4), dict(ema=p + 4 * n - 4), dict(param=e - 4 * n + 4)):
        assert call(**bad) == _lib.SSD_ERR_VALUE, bad
    # om == 0 keeps ema as it is: accepted, nothing to launch (the pointers stay undereferenced)
    assert call(om=0.0) == _lib.SSD_OK
    assert "ssd_ema_step" in _lib._SIGNATURES and len(_lib._SIGNATURES["ssd_ema_step"][1]) == 5
