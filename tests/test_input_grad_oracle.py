"""tests/input_grad_oracle.py against the unchanged oracle (CPU): the feature gradients autograd gives
through the helper's leaf tensors equal central differences of TorchOracle's own float64 ``forward``.

RouteNet, T = 2, one NSFNET graph, the MSE loss of tests/test_gpu_training.py.  Central differences at
eps = 1e-6: truncation ~ eps^2 f''' / 6 ~ 1e-12 and rounding ~ 2^-53 L / eps ~ 1e-10 of the loss scale,
so the 1e-5 of the tensor's largest |g| allowed here leaves room and still catches a wrong column, row
or sign.  8 random coordinates per feature, and 2 random unit directions over all features."""
import copy

import numpy as np
import pytest
import torch

from ignnition_amd import model_examples, synthetic, workloads
from ignnition_amd.engine import MPPlan
from ignnition_amd.json_operations import Model_information
from oracle.train_oracle import TorchOracle
from tests.input_grad_oracle import InputGradOracle

EPS = 1e-6
TOL = 1e-5


@pytest.fixture(scope="module")
def case():
    desc = model_examples.routenet(iterations=2)
    _, dims, _ = workloads.model("routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, labels = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", 0)])
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(7, bias_scale=0.1)
    o = InputGradOracle(desc, dims, prm)
    loss, _, pgrads, pred = o.loss_and_grads(graphs, labels)
    parent = TorchOracle(desc, dims, prm)
    y = np.concatenate([np.asarray(l, np.float64).reshape(-1) for l in labels])

    def parent_loss(x):
        with torch.no_grad():
            return float(((torch.tensor(y) - parent.forward([x])) ** 2).mean())

    return plan, graphs[0], parent_loss, loss, pgrads, pred, o.feature_grads(), parent, labels


def _f64(x, plan):
    x = dict(x)
    for feats in plan.features:
        for name, size in feats:
            x[name] = np.asarray(x[name], np.float64).reshape(-1, size).copy()
    return x


def test_helper_forward_is_the_parents(case):
    """The same loss, predictions and parameter gradients as the unchanged oracle, to the bit: the
    helper only swaps how the feature columns are created."""
    plan, x, parent_loss, loss, pgrads, pred, _, parent, labels = case
    p_loss, _, p_grads, p_pred = parent.loss_and_grads([x], labels)
    assert loss == p_loss
    assert np.array_equal(pred, p_pred)
    for k, g in p_grads.items():
        assert np.array_equal(pgrads[k], g), k


def test_coordinates_match_central_differences(case):
    plan, x, parent_loss, _, _, _, fg, _, _ = case
    rng = np.random.default_rng(0)
    for ent, feats in zip(plan.entities, plan.features):
        for name, size in feats:
            g = fg[ent][name]
            assert g.shape == (np.asarray(x[name]).size // size, size)
            scale = np.abs(g).max()
            assert scale > 0
            worst = 0.0
            for _ in range(8):
                r, c = int(rng.integers(g.shape[0])), int(rng.integers(size))
                hi, lo = _f64(x, plan), _f64(x, plan)
                hi[name][r, c] += EPS
                lo[name][r, c] -= EPS
                fd = (parent_loss(hi) - parent_loss(lo)) / (2 * EPS)
                worst = max(worst, abs(fd - g[r, c]) / scale)
            print("%s: worst |fd - g| / max|g| = %.3g" % (name, worst))
            assert worst <= TOL, name


def test_directions_match_central_differences(case):
    plan, x, parent_loss, _, _, _, fg, _, _ = case
    rng = np.random.default_rng(1)
    names = [(ent, name) for ent, feats in zip(plan.entities, plan.features) for name, _ in feats]
    scale = max(np.abs(fg[ent][name]).max() for ent, name in names)
    for _ in range(2):
        d = {name: rng.standard_normal(fg[ent][name].shape) for ent, name in names}
        norm = np.sqrt(sum((v * v).sum() for v in d.values()))
        d = {k: v / norm for k, v in d.items()}
        hi, lo = _f64(x, plan), _f64(x, plan)
        for k, v in d.items():
            hi[k] += EPS * v
            lo[k] -= EPS * v
        fd = (parent_loss(hi) - parent_loss(lo)) / (2 * EPS)
        an = sum((fg[ent][name] * d[name]).sum() for ent, name in names)
        print("direction: fd %.9g autograd %.9g" % (fd, an))
        assert abs(fd - an) <= TOL * scale
