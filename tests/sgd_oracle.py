"""float64 oracle of the momentum SGD update (ssd_sgd_momentum_step, include/ssd_hip.h), restated in numpy.

Keras SGD(momentum, nesterov) -- also Caffe's form, the learning rate folded into the velocity -- with an optional L2 term:
    sc = grad_scale * scale            (scale: per element, 1 where the kernel is given none)
    ge = g * sc;   if decay is given: ge = ge + decay * p
    v' = momentum * v - lr * ge
    p' = nesterov ? p + (momentum * v' - lr * ge) : p + v'
"""
import numpy as np


def sgd_momentum_step(p, g, v, lr, momentum, nesterov=False, sc=1.0, decay=None):
    """One step; p, g, v arrays (any float dtype, computed in float64); sc and decay scalars or arrays broadcast against p.
    Returns (p', v')."""
    p, g, v = np.asarray(p, np.float64), np.asarray(g, np.float64), np.asarray(v, np.float64)
    ge = g * np.asarray(sc, np.float64)
    if decay is not None:
        ge = ge + np.asarray(decay, np.float64) * p
    v1 = momentum * v - lr * ge
    p1 = p + (momentum * v1 - lr * ge) if nesterov else p + v1
    return p1, v1
