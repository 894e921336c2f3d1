"""tests/edge_param_grad_oracle.py against the unchanged oracle (CPU): the edge-parameter gradients
autograd gives through the helper's leaf tensors equal central differences of TorchOracle's own float64
``forward``, and the helper's forward is the parent's to the bit.

Cases of tests/edge_param_cases.py, one NSFNET graph each (T = 2, the MSE loss of
tests/test_gpu_training.py): a slice listed twice, a network under attention, the ordered form, and
two MPs reading one adjacency, so that a leaf read several times per iteration sums its uses.
Central differences at eps = 1e-6: truncation ~ eps^2 f''' / 6 ~ 1e-12 and rounding ~ 2^-53 L / eps ~
1e-10 of the loss scale, so the 1e-5 of the tensor's largest |g| allowed here leaves room and still
catches a wrong row, column, sign or a use left out of the sum.  8 random coordinates and 2 random unit
directions per case."""
import numpy as np
import pytest
import torch

from oracle import train_oracle
from oracle.train_oracle import TorchOracle
from tests import edge_param_cases as ec
from tests.edge_param_grad_oracle import EdgeParamGradOracle

EPS = 1e-6
TOL = 1e-5
NAMES = ["sum_p3_twice", "ordered_p1_middle", "attention_p2_last", "two_mps_p2"]


@pytest.fixture(scope="module", params=NAMES)
def case(request):
    desc, dims, graphs, labels, prm = ec.case_inputs(request.param)
    x, labels = graphs[0], labels[:1]
    key = "params_" + ec.ADJ[request.param]
    o = EdgeParamGradOracle(desc, dims, prm)
    loss, _, pgrads, pred = o.loss_and_grads([x], labels)
    parent = TorchOracle(desc, dims, prm)
    y = np.concatenate([np.asarray(l, np.float64).reshape(-1) for l in labels])

    def parent_loss(values):
        xx = dict(x)
        xx[key] = values
        with torch.no_grad():
            return float(((torch.tensor(y) - parent.forward([xx])) ** 2).mean())

    g = o.edge_param_grads()
    assert list(g) == [key]
    return x, key, labels, parent, parent_loss, loss, pgrads, pred, g[key]


def test_helper_forward_is_the_parents(case):
    """The same loss, predictions and parameter gradients as the unchanged oracle, to the bit: the
    helper only swaps how the parameter tensor is created, and puts the module's torch back."""
    x, key, labels, parent, _, loss, pgrads, pred, _ = case
    assert train_oracle.torch is torch
    p_loss, _, p_grads, p_pred = parent.loss_and_grads([x], labels)
    assert loss == p_loss
    assert np.array_equal(pred, p_pred)
    for k, g in p_grads.items():
        assert np.array_equal(pgrads[k], g), k


def test_coordinates_match_central_differences(case):
    x, key, _, _, parent_loss, _, _, _, g = case
    v0 = np.asarray(x[key], np.float64).reshape(g.shape)
    assert g.shape[0] == len(np.asarray(x["src_" + key[len("params_"):]]).reshape(-1))
    scale = np.abs(g).max()
    assert scale > 0
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(8):
        r, c = int(rng.integers(g.shape[0])), int(rng.integers(g.shape[1]))
        hi, lo = v0.copy(), v0.copy()
        hi[r, c] += EPS
        lo[r, c] -= EPS
        fd = (parent_loss(hi) - parent_loss(lo)) / (2 * EPS)
        worst = max(worst, abs(fd - g[r, c]) / scale)
    print("%s: worst |fd - g| / max|g| = %.3g" % (key, worst))
    assert worst <= TOL


def test_directions_match_central_differences(case):
    x, key, _, _, parent_loss, _, _, _, g = case
    v0 = np.asarray(x[key], np.float64).reshape(g.shape)
    rng = np.random.default_rng(1)
    for _ in range(2):
        d = rng.standard_normal(g.shape)
        d /= np.linalg.norm(d)
        fd = (parent_loss(v0 + EPS * d) - parent_loss(v0 - EPS * d)) / (2 * EPS)
        an = (g * d).sum()
        print("direction: fd %.9g autograd %.9g" % (fd, an))
        assert abs(fd - an) <= TOL * np.abs(g).max()
