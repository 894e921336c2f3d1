"""learning_options on the CPU: the C ABI's loss / optimizer name tables, training.learning_options,
the learning-rate schedules against hand-computed values, and the float64 restatement
(tests/keras_restated.py) that the GPU tests measure the kernels against."""
import copy
import ctypes as C

import numpy as np
import pytest

from ignnition_amd import _lib, model_examples, training, workloads
from ignnition_amd.engine import UnsupportedModel
from ignnition_amd.json_operations import Model_information
from tests import keras_restated as kr


def _kind(fn, name):
    k = C.c_int32(-7)
    rc = fn(name.encode(), C.byref(k))
    return rc, k.value, _lib.lib.ign_last_error().decode()


def test_name_tables():
    for i, n in enumerate(kr.LOSSES):
        assert _kind(_lib.lib.ign_loss_kind, n)[:2] == (0, i), n
    for i, n in enumerate(kr.OPTIMIZERS):
        assert _kind(_lib.lib.ign_optimizer_kind, n)[:2] == (0, i), n
    assert tuple(kr.LOSSES) == training.SUPPORTED_LOSSES
    for fn, names in ((_lib.lib.ign_loss_kind, kr.LOSSES), (_lib.lib.ign_optimizer_kind, kr.OPTIMIZERS)):
        for bad in ("Nadam", "CosineSimilarity", "", "adam", "Ftrl", "meansquarederror"):
            rc, k, msg = _kind(fn, bad)
            assert rc == -2 and k == -7, bad
            for n in names:
                assert n in msg, (bad, msg)
    assert _lib.lib.ign_loss_kind(None, None) == -1
    for n in ("ign_loss_kind", "ign_optimizer_kind", "ign_loss", "ign_optimizer_num_slots", "ign_optimizer_step"):
        assert n in _lib.SYMBOLS and hasattr(_lib.lib, n)
    assert _lib.lib.ign_abi_version() == 13


def _mi(loss="MeanSquaredError", optimizer=None):
    desc = model_examples.routenet()
    desc["learning_options"]["loss"] = loss
    if optimizer is not None:
        desc["learning_options"]["optimizer"] = optimizer
    _, dims, _ = workloads.model("routenet")
    return Model_information(copy.deepcopy(desc), dims)


@pytest.mark.parametrize("loss", kr.LOSSES)
def test_learning_options_losses(loss):
    lo = training.learning_options(_mi(loss))
    assert (lo.loss, lo.loss_kind) == (loss, kr.LOSSES.index(loss))
    assert (lo.optimizer, lo.desc.kind, lo.num_slots, lo.slot_init) == ("Adam", 0, 2, 0.0)
    assert lo.lr.kind == "ExponentialDecay"


F32 = lambda x: float(np.float32(x))   # noqa: E731  (the desc carries the hyper-parameters as float)


@pytest.mark.parametrize("opt,slots,init,rate,fields", [
    ({"type": "Adam"}, 2, 0.0, 0.001, {"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7}),
    ({"type": "SGD"}, 0, 0.0, 0.01, {"momentum": 0.0, "nesterov": 0}),
    ({"type": "SGD", "momentum": 0.9}, 1, 0.0, 0.01, {"momentum": 0.9, "nesterov": 0}),
    ({"type": "SGD", "momentum": 0.5, "nesterov": True, "learning_rate": 0.1}, 1, 0.0, 0.1, {"momentum": 0.5, "nesterov": 1}),
    ({"type": "RMSprop"}, 1, 0.0, 0.001, {"rho": 0.9, "momentum": 0.0, "epsilon": 1e-7, "centered": 0}),
    ({"type": "RMSprop", "centered": True}, 2, 0.0, 0.001, {"centered": 1}),
    ({"type": "RMSprop", "momentum": 0.8, "rho": 0.95}, 2, 0.0, 0.001, {"momentum": 0.8, "rho": 0.95}),
    ({"type": "RMSprop", "momentum": 0.8, "centered": True, "name": "x"}, 3, 0.0, 0.001, {"centered": 1}),
    ({"type": "Adagrad"}, 1, 0.1, 0.001, {"initial_accumulator_value": 0.1, "epsilon": 1e-7}),
    ({"type": "Adagrad", "initial_accumulator_value": 0.5}, 1, 0.5, 0.001, {}),
    ({"type": "Adadelta"}, 2, 0.0, 0.001, {"rho": 0.95, "epsilon": 1e-7}),
    ({"type": "Adamax", "beta_1": 0.8}, 2, 0.0, 0.001, {"beta_1": 0.8, "beta_2": 0.999, "epsilon": 1e-7}),
])
def test_learning_options_optimizers(opt, slots, init, rate, fields):
    lo = training.learning_options(_mi("Huber", opt))
    assert lo.optimizer == opt["type"] and lo.desc.kind == kr.OPTIMIZERS.index(opt["type"])
    assert lo.num_slots == slots and lo.slot_init == F32(init)
    assert lo.desc.reserved == 0
    assert lo.lr.kind == "constant" and lo.lr(0) == lo.lr(10 ** 6) == rate
    for k, v in fields.items():
        assert getattr(lo.desc, k) == (F32(v) if isinstance(v, float) else v), k


@pytest.mark.parametrize("loss,opt,match", [
    ("CosineSimilarity", {"type": "Adam"}, "MeanAbsolutePercentageError"),
    ("MeanSquaredError", {"type": "Nadam"}, "Adamax"),
    ("MeanSquaredError", {"type": "Ftrl"}, "RMSprop"),
    ("MeanSquaredError", {"type": "SGD", "clipnorm": 1.0}, "clipnorm"),
    ("MeanSquaredError", {"type": "Adam", "clipvalue": 0.5}, "clipvalue"),
    ("MeanSquaredError", {"type": "RMSprop", "beta_1": 0.9}, "beta_1"),
    ("MeanSquaredError", {"type": "SGD", "amsgrad": False}, "amsgrad"),
    ("MeanSquaredError", {"type": "Adam", "amsgrad": True}, "amsgrad"),
    ("MeanSquaredError", {"type": "Adam", "schedule": {"type": "CosineDecay", "initial_learning_rate": 0.1,
                                                       "decay_steps": 10}}, "PolynomialDecay"),
])
def test_learning_options_refusals(loss, opt, match, monkeypatch):
    with pytest.raises(UnsupportedModel, match=match):
        training.learning_options(_mi(loss, opt))
    # the Trainer refuses before it touches the GPU
    import torch

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    with pytest.raises(UnsupportedModel, match=match):
        training.Trainer(_mi(loss, opt))


def test_learning_options_needs_no_gpu():
    import torch
    was = torch.cuda.is_initialized()
    training.learning_options(_mi("Poisson", {"type": "Adadelta"}))
    assert torch.cuda.is_initialized() == was


def _lr(schedule, optimizer="Adam"):
    return training.LearningRate({"type": optimizer, "schedule": schedule})


def test_piecewise_constant_decay():
    lr = _lr({"type": "PiecewiseConstantDecay", "boundaries": [2, 4], "values": [0.1, 0.01, 0.001]})
    assert [lr(s) for s in (0, 2, 3, 4, 5, 100)] == [0.1, 0.1, 0.01, 0.01, 0.001, 0.001]
    assert [kr.piecewise_constant_decay(s, [2, 4], [0.1, 0.01, 0.001]) for s in (0, 2, 3, 4, 5, 100)] == \
        [0.1, 0.1, 0.01, 0.01, 0.001, 0.001]


@pytest.mark.parametrize("cycle,expected", [
    # (0.1 - 0.01) (1 - p)^2 + 0.01 with p = step / 10 capped at 1 ...
    (False, {0: 0.1, 5: 0.0325, 10: 0.01, 11: 0.01, 21: 0.01}),
    # ... or with the decay steps times max(1, ceil(step / 10)): 11 -> p = 11/20, 21 -> p = 21/30
    (True, {0: 0.1, 5: 0.0325, 10: 0.01, 11: 0.09 * 0.45 ** 2 + 0.01, 21: 0.09 * 0.3 ** 2 + 0.01}),
])
def test_polynomial_decay(cycle, expected):
    cfg = {"initial_learning_rate": 0.1, "decay_steps": 10, "end_learning_rate": 0.01, "power": 2, "cycle": cycle}
    lr = _lr(dict(cfg, type="PolynomialDecay"))
    for s, v in expected.items():
        assert lr(s) == pytest.approx(v, rel=1e-12), s
        assert kr.polynomial_decay(s, **cfg) == pytest.approx(v, rel=1e-12), s
    # the defaults: end_learning_rate 1e-4, power 1, cycle false
    lr = _lr({"type": "PolynomialDecay", "initial_learning_rate": 0.1, "decay_steps": 10})
    assert lr(5) == pytest.approx(0.05005, rel=1e-12) and lr(10) == lr(21) == pytest.approx(1e-4, rel=1e-12)


def test_inverse_time_decay():
    cfg = {"initial_learning_rate": 0.1, "decay_steps": 4, "decay_rate": 0.5}
    stairs = _lr(dict(cfg, type="InverseTimeDecay", staircase="False"))   # a string: truthy, as in Keras
    smooth = _lr(dict(cfg, type="InverseTimeDecay"))
    for s, v in {0: 0.1, 4: 0.1 / 1.5, 5: 0.1 / 1.5, 9: 0.05, 400: 0.1 / 51}.items():
        assert stairs(s) == pytest.approx(v, rel=1e-12), s
        assert kr.inverse_time_decay(s, staircase="False", **cfg) == pytest.approx(v, rel=1e-12), s
    for s, v in {0: 0.1, 4: 0.1 / 1.5, 5: 0.1 / 1.625, 400: 0.1 / 51}.items():
        assert smooth(s) == pytest.approx(v, rel=1e-12), s


def test_exponential_decay_unchanged():
    lr = _lr({"type": "ExponentialDecay", "initial_learning_rate": 0.01, "decay_steps": 2, "decay_rate": 0.5,
              "staircase": "True"})
    assert [lr(s) for s in range(5)] == [0.01, 0.01, 0.005, 0.005, 0.0025]


def _domain(name, rng, n):
    """Random O(1) inputs in the loss's domain, away from its kinks."""
    if name == "BinaryCrossentropy":
        return rng.uniform(0.05, 0.95, n), rng.uniform(0.05, 0.95, n)
    if name in ("Poisson", "MeanSquaredLogarithmicError", "MeanAbsolutePercentageError"):
        p, y = rng.uniform(0.2, 2.0, n), rng.uniform(0.2, 2.0, n)
    else:
        p, y = rng.normal(0, 1.5, n), rng.normal(0, 1.5, n)
    d = p - y
    near = (np.abs(d) < 1e-2) | (np.abs(np.abs(d) - 1.0) < 1e-2)   # |d| = 0 (MAE, MAPE), |d| = 1 (Huber)
    p[near] += 0.1
    return p, y


@pytest.mark.parametrize("name", kr.LOSSES)
def test_restated_dpred_is_the_derivative_of_the_restated_loss(name):
    rng = np.random.default_rng(kr.LOSSES.index(name))
    p, y = _domain(name, rng, 64)
    g = kr.dpred(name, p, y)
    h = 1e-6
    fd = np.empty_like(p)
    for i in range(p.size):
        e = np.zeros_like(p)
        e[i] = h
        fd[i] = (kr.loss(name, p + e, y) - kr.loss(name, p - e, y)) / (2 * h)
    # float64 rounding of the O(1) (MAPE: O(100)) loss over 2h leaves 1e-10 .. 1e-8 absolute in fd
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-9)
    assert not kr.dpred_is_zero(name, p, y).any()
    # the package's host loss (Trainer.evaluate) is the same formula
    assert training.host_loss(kr.LOSSES.index(name), p, y) == pytest.approx(kr.loss(name, p, y), rel=1e-13)
    assert training.host_loss(0, p, y) == float(np.mean((y - p) ** 2))   # what evaluate computed for MeanSquaredError


def test_restated_optimizers_zero_gradient_is_a_zero_update():
    w0 = np.linspace(-1, 1, 7)
    cases = [("SGD", {}), ("SGD", {"momentum": 0.9}), ("SGD", {"momentum": 0.9, "nesterov": True}), ("RMSprop", {}),
             ("RMSprop", {"centered": True, "momentum": 0.5}), ("Adagrad", {}), ("Adadelta", {}), ("Adamax", {})]
    for name, given in cases:
        h = kr.hyper(name, **given)
        w, slots = w0.copy(), kr.init_slots(name, h, w0.size)
        kr.optimizer_step(name, h, w, np.zeros_like(w), slots, 0, 0.1)
        np.testing.assert_array_equal(w, w0, err_msg=name)
