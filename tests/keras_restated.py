"""Float64 restatements of the Keras losses, optimizers and learning-rate schedules the engine lowers
beside MeanSquaredError / Adam / ExponentialDecay (oracle/train_oracle.py restates those): the
yardstick of test_learning_options.py and test_gpu_losses_optimizers.py.

Losses: Keras' default constructor arguments, eps = 1e-7, the mean over the flat predictions; the
float64 formula itself (``log1p``), not TensorFlow's float32 rounding of it.  Optimizers:
optimizer_v2 semantics with t = iteration + 1, on flat float64 vectors, in place."""
import math

import numpy as np

EPS = 1e-7
LOSSES = ["MeanSquaredError", "MeanAbsoluteError", "MeanAbsolutePercentageError", "MeanSquaredLogarithmicError",
          "Huber", "LogCosh", "BinaryCrossentropy", "Poisson"]
OPTIMIZERS = ["Adam", "SGD", "RMSprop", "Adagrad", "Adadelta", "Adamax"]
DEFAULTS = {
    "SGD": {"learning_rate": 0.01, "momentum": 0.0, "nesterov": False},
    "RMSprop": {"learning_rate": 0.001, "rho": 0.9, "momentum": 0.0, "epsilon": 1e-7, "centered": False},
    "Adagrad": {"learning_rate": 0.001, "initial_accumulator_value": 0.1, "epsilon": 1e-7},
    "Adadelta": {"learning_rate": 0.001, "rho": 0.95, "epsilon": 1e-7},
    "Adamax": {"learning_rate": 0.001, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7},
}


def _f64(*xs):
    return [np.asarray(x, np.float64).reshape(-1) for x in xs]


def loss_terms(name, p, y):
    p, y = _f64(p, y)
    d = p - y
    if name == "MeanSquaredError":
        return d * d
    if name == "MeanAbsoluteError":
        return np.abs(d)
    if name == "MeanAbsolutePercentageError":
        return 100.0 * np.abs(d) / np.maximum(np.abs(y), EPS)
    if name == "MeanSquaredLogarithmicError":
        return (np.log1p(np.maximum(p, EPS)) - np.log1p(np.maximum(y, EPS))) ** 2
    if name == "Huber":
        return np.where(np.abs(d) <= 1.0, d * d / 2.0, np.abs(d) - 0.5)
    if name == "LogCosh":   # d + softplus(-2d) - log 2, softplus(x) = max(x, 0) + log1p(exp(-|x|))
        return d + np.maximum(-2.0 * d, 0.0) + np.log1p(np.exp(-np.abs(2.0 * d))) - math.log(2.0)
    if name == "BinaryCrossentropy":
        q = np.clip(p, EPS, 1.0 - EPS)
        return -(y * np.log(q + EPS) + (1.0 - y) * np.log(1.0 - q + EPS))
    if name == "Poisson":
        return p - y * np.log(p + EPS)
    raise KeyError(name)


def loss(name, p, y) -> float:
    return float(np.mean(loss_terms(name, p, y)))


def dpred(name, p, y):
    """d loss / d p: the table's column over n."""
    p, y = _f64(p, y)
    d = p - y
    n = p.size
    if name == "MeanSquaredError":
        g = 2.0 * d
    elif name == "MeanAbsoluteError":
        g = np.sign(d)
    elif name == "MeanAbsolutePercentageError":
        g = 100.0 * np.sign(d) / np.maximum(np.abs(y), EPS)
    elif name == "MeanSquaredLogarithmicError":
        l = np.log1p(np.maximum(p, EPS)) - np.log1p(np.maximum(y, EPS))
        g = np.where(p > EPS, 2.0 * l / (1.0 + p), 0.0)
    elif name == "Huber":
        g = np.clip(d, -1.0, 1.0)
    elif name == "LogCosh":
        g = np.tanh(d)
    elif name == "BinaryCrossentropy":
        q = np.clip(p, EPS, 1.0 - EPS)
        g = np.where((p > EPS) & (p < 1.0 - EPS), -(y / (q + EPS) - (1.0 - y) / (1.0 - q + EPS)), 0.0)
    elif name == "Poisson":
        g = 1.0 - y / (p + EPS)
    else:
        raise KeyError(name)
    return g / n


def dpred_is_zero(name, p, y):
    """Where the table says dpred is 0 (exactly)."""
    p, y = _f64(p, y)
    if name in ("MeanAbsoluteError", "MeanAbsolutePercentageError"):
        return p == y
    if name == "MeanSquaredLogarithmicError":
        return ~(p > EPS)
    if name == "BinaryCrossentropy":
        return ~((p > EPS) & (p < 1.0 - EPS))
    return np.zeros(p.shape, bool)


# ---------------------------------------------------------------------------------------------
def hyper(name, **given):
    """The optimizer's hyper-parameters: Keras' defaults overridden by ``given``."""
    h = dict(DEFAULTS[name])
    for k, v in given.items():
        if k not in h:
            raise KeyError("%s does not take %s" % (name, k))
        h[k] = v
    return h


def num_slots(name, h) -> int:
    if name == "SGD":
        return 1 if h["momentum"] > 0 else 0
    if name == "RMSprop":
        return 1 + bool(h["centered"]) + (h["momentum"] > 0)
    return {"Adagrad": 1, "Adadelta": 2, "Adamax": 2, "Adam": 2}[name]


def init_slots(name, h, n) -> list:
    """rms, then mg (centered), then mom (momentum > 0) for RMSprop; v for SGD; acc for Adagrad;
    acc, accu for Adadelta; m, u for Adamax."""
    v0 = h["initial_accumulator_value"] if name == "Adagrad" else 0.0
    return [np.full(n, v0, np.float64) for _ in range(num_slots(name, h))]


def optimizer_step(name, h, w, g, slots, iteration, lr):
    """One update in float64, in place on ``w`` and ``slots``."""
    g = np.asarray(g, np.float64)
    t = iteration + 1
    if name == "SGD":
        mu = h["momentum"]
        if mu > 0:
            v = slots[0]
            v[:] = mu * v - lr * g
            w += mu * v - lr * g if h["nesterov"] else v
        else:
            w -= lr * g
    elif name == "RMSprop":
        rho, mu, eps = h["rho"], h["momentum"], h["epsilon"]
        rms = slots[0]
        rms[:] = rho * rms + (1 - rho) * g * g
        den = rms
        k = 1
        if h["centered"]:
            mg = slots[k]
            k += 1
            mg[:] = rho * mg + (1 - rho) * g
            den = np.maximum(rms - mg * mg, 0.0)
        if mu > 0:
            mom = slots[k]
            mom[:] = mu * mom + lr * g / np.sqrt(den + eps)
            w -= mom
        else:
            w -= lr * g / (np.sqrt(den) + eps)
    elif name == "Adagrad":
        acc = slots[0]
        acc += g * g
        w -= lr * g / (np.sqrt(acc) + h["epsilon"])
    elif name == "Adadelta":
        rho, eps = h["rho"], h["epsilon"]
        acc, accu = slots
        acc[:] = rho * acc + (1 - rho) * g * g
        u = np.sqrt(accu + eps) / np.sqrt(acc + eps) * g
        accu[:] = rho * accu + (1 - rho) * u * u
        w -= lr * u
    elif name == "Adamax":
        b1, b2, eps = h["beta_1"], h["beta_2"], h["epsilon"]
        m, u = slots
        m[:] = b1 * m + (1 - b1) * g
        u[:] = np.maximum(b2 * u, np.abs(g))
        w -= lr / (1 - b1 ** t) * m / (u + eps)
    else:
        raise KeyError(name)


# ---------------------------------------------------------------------------------------------
def piecewise_constant_decay(step, boundaries, values):
    for b, v in zip(boundaries, values):
        if step <= b:
            return v
    return values[-1]


def polynomial_decay(step, initial_learning_rate, decay_steps, end_learning_rate=1e-4, power=1.0, cycle=False):
    if cycle:
        decay_steps = decay_steps * max(1, math.ceil(step / decay_steps))
    else:
        step = min(step, decay_steps)
    return (initial_learning_rate - end_learning_rate) * (1 - step / decay_steps) ** power + end_learning_rate


def inverse_time_decay(step, initial_learning_rate, decay_steps, decay_rate, staircase=False):
    p = step / decay_steps
    if staircase:            # truthy test, as Keras does (a "False" string is truthy too)
        p = math.floor(p)
    return initial_learning_rate / (1 + decay_rate * p)
