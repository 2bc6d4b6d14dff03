"""float64 oracle of the exponential moving average of the weights (ssd_ema_step, include/ssd_hip.h; ops.EmaSpec), restated in
numpy.  Independent of the package: the host rule for the factor is written out here again, not imported."""
import numpy as np

U = 2.0 ** -24                      # one fp32 rounding, relative to its result


def decay_at(t, decay, warmup=True):
    """The decay of update t (t updates made before it): TF ExponentialMovingAverage's num_updates rule, or the constant."""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def one_minus_decay(t, decay, warmup=True):
    """The host rule: 1 - d_t in double, then ONE rounding to fp32 -- the factor the kernel receives."""
    return np.float32(1.0 - decay_at(t, decay, warmup))


def ema_update(e, p, om):
    """One update in float64: e' = e + om (p - e); om as the kernel receives it (an fp32 number)."""
    e, p = np.asarray(e, np.float64), np.asarray(p, np.float64)
    return e + float(om) * (p - e)


def step_bound(e, p):
    """What one fp32 update may differ from ema_update by, per element: one rounding of the difference, one of the product
    and one of the sum, each at most 2^-24 (|p| + |e|) since om <= 1 -- 2^-22 (|p| + |e|) with one to spare."""
    return 4.0 * U * (np.abs(np.asarray(p, np.float64)) + np.abs(np.asarray(e, np.float64)))


def ema_chain(e0, params, decay, warmup=True, t0=0):
    """T updates from e0 with the parameter snapshots `params` (update k uses the factor of t0 + k).  Returns (e, bound): the
    float64 average, and T times the one-step bound taken at the running maxima of |p| and |e| -- an update contracts the
    error it inherits (factor 1 - om <= 1), so the steps' bounds add."""
    e = np.asarray(e0, np.float64)
    emax, pmax = np.abs(e), np.zeros_like(e)
    for k, p in enumerate(params):
        p = np.asarray(p, np.float64)
        e = ema_update(e, p, one_minus_decay(t0 + k, decay, warmup))
        emax, pmax = np.maximum(emax, np.abs(e)), np.maximum(pmax, np.abs(p))
    return e, len(params) * 4.0 * U * (pmax + emax)
