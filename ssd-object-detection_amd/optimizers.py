"""Learning-rate schedules and optimizer descriptors with the Keras names tools/train.py uses
(reference tools/train.py:31-53).  They only carry hyper-parameters; the update itself is the fused
HIP kernel (ssd_adam_step / ssd_sgd_step / ssd_sgd_momentum_step) driven by SSDEngine."""
import numbers


class ExponentialDecay:
    """tf.keras.optimizers.schedules.ExponentialDecay, staircase=False: lr0 * rate ** (step / decay_steps)."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate):
        self.initial_learning_rate, self.decay_steps, self.decay_rate = initial_learning_rate, decay_steps, decay_rate

    def __call__(self, step):
        return self.initial_learning_rate * self.decay_rate ** (step / self.decay_steps)


class PolynomialDecay:
    """tf.keras.optimizers.schedules.PolynomialDecay, power=1, cycle=False."""

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=0.0001, power=1.0):
        self.initial_learning_rate, self.decay_steps = initial_learning_rate, decay_steps
        self.end_learning_rate, self.power = end_learning_rate, power

    def __call__(self, step):
        s = min(step, self.decay_steps)
        return (self.initial_learning_rate - self.end_learning_rate) * (1 - s / self.decay_steps) ** self.power \
            + self.end_learning_rate


class PiecewiseConstantDecay:
    """tf.keras.optimizers.schedules.PiecewiseConstantDecay: values[0] while step <= boundaries[0], values[i] while
    boundaries[i-1] < step <= boundaries[i], values[-1] beyond the last boundary (the SSD paper's 1e-3, 1e-4, 1e-5)."""

    def __init__(self, boundaries, values):
        boundaries, values = list(boundaries), list(values)
        if len(values) != len(boundaries) + 1:
            raise ValueError("PiecewiseConstantDecay needs len(values) == len(boundaries) + 1, got %d values for %d boundaries"
                             % (len(values), len(boundaries)))
        if any(b1 <= b0 for b0, b1 in zip(boundaries, boundaries[1:])):
            raise ValueError("PiecewiseConstantDecay boundaries must be strictly increasing: %r" % (boundaries,))
        self.boundaries, self.values = boundaries, [float(v) for v in values]

    def __call__(self, step):
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return v
        return self.values[-1]


class _Optimizer:
    def __init__(self, learning_rate):
        self._lr = learning_rate
        self.iterations = 0                       # Keras: optimizer.iterations

    def lr(self, step=None):
        """Learning rate at the optimizer's own iteration count (Keras evaluates schedules there)."""
        it = self.iterations if step is None else step
        return self._lr(it) if callable(self._lr) else float(self._lr)


class Adam(_Optimizer):
    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, name="Adam", **_):
        super().__init__(learning_rate)
        self.beta_1, self.beta_2, self.epsilon, self.name = beta_1, beta_2, epsilon, name


class SGD(_Optimizer):
    """tf.keras.optimizers.SGD(learning_rate, momentum, nesterov) plus an L2 term on the filters (weight_decay; on the biases
    too with decay_bias -- Caffe SSD gives them decay_mult 0).  With the defaults it is plain p -= lr * g (ssd_sgd_step) and
    keeps no slot; with momentum > 0 or weight_decay > 0 the update is ssd_sgd_momentum_step and the velocity is a slot."""

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, weight_decay=0.0, decay_bias=False, name="SGD", **_):
        super().__init__(learning_rate)
        if isinstance(momentum, bool) or not isinstance(momentum, numbers.Real) or not 0.0 <= momentum < 1.0:
            raise ValueError("SGD momentum must be a number in [0, 1), not %r" % (momentum,))
        if isinstance(weight_decay, bool) or not isinstance(weight_decay, numbers.Real) or not weight_decay >= 0.0:
            raise ValueError("SGD weight_decay must be a number >= 0, not %r" % (weight_decay,))
        if not isinstance(nesterov, bool) or not isinstance(decay_bias, bool):
            raise ValueError("SGD nesterov and decay_bias must be booleans, not %r / %r" % (nesterov, decay_bias))
        self.momentum, self.nesterov = float(momentum), nesterov
        self.weight_decay, self.decay_bias, self.name = float(weight_decay), decay_bias, name

    @property
    def uses_slots(self):
        """Whether the update is the momentum / decay kernel (which keeps a velocity) rather than plain SGD."""
        return self.momentum > 0.0 or self.weight_decay > 0.0
