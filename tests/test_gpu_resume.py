"""Resuming a run exactly: Trainer.state() / load_state() through a state file, and train_and_evaluate's
resume_from, each held bitwise to the uninterrupted run.

What a resume that dropped one part of the state would change, per optimizer case of the Trainer test
(the model has a readout Dropout and an ExponentialDecay rate with decay_steps 2, and the resumed
Trainer is built with another seed, so other initial parameters and another dropout seed):

* the slots: every case below owns at least one slot (SGD through its momentum) that is non-zero
  after three steps, so steps 4-6 and the final slot tensors differ in every case;
* ``iterations``: the per-step learning_rate restarts at its initial value in every case, and the
  Dropout masks of steps 4-6 are drawn for steps 1-3; Adam and Adamax also restart their bias
  correction;
* the dropout seed: the masks of steps 4-6 come from the new Trainer's own seed in every case, which
  moves the step-6 loss and, through the gradient, the parameters and slots."""
import copy
import json
import os

import numpy as np
import pytest

from examples.make_example import make
from ignnition_amd import checkpoint, model_examples, synthetic, workloads
from ignnition_amd import framework_operations as fo
from ignnition_amd import generate_model as gm
from ignnition_amd.engine import MPPlan, device_count
from ignnition_amd.json_operations import Model_information
from ignnition_amd.training import Trainer, slot_names
from tests.dropout_cases import insert_dropout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


OPTIMIZERS = [{"type": "Adam"}, {"type": "SGD", "momentum": 0.9, "nesterov": True},
              {"type": "RMSprop", "centered": True, "momentum": 0.5}, {"type": "Adagrad"}, {"type": "Adadelta"},
              {"type": "Adamax"}]
SCHEDULE = {"type": "ExponentialDecay", "initial_learning_rate": 0.01, "decay_steps": 2, "decay_rate": 0.5}


def _model(optimizer):
    desc = insert_dropout(model_examples.routenet(hidden=16, iterations=2), [(1, 0.25, {})])
    desc["learning_options"] = {"loss": "MeanSquaredError", "optimizer": dict(optimizer, schedule=dict(SCHEDULE))}
    _, dims, _ = workloads.model("routenet")
    return Model_information(copy.deepcopy(desc), dims)


def _steps(tr, data):
    out = [tr.train_step(graphs, labels) for graphs, labels in data]
    return [o["learning_rate"] for o in out], out[-1]["loss"]


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)


@pytest.mark.parametrize("optimizer", OPTIMIZERS, ids=[o["type"] for o in OPTIMIZERS])
def test_trainer_resumes_bitwise(optimizer, tmp_path):
    mi = _model(optimizer)
    data = [workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", 2 * k + g) for g in range(2)])
            for k in range(6)]
    prm = MPPlan.from_model_info(mi).init_params(7, bias_scale=0.1)
    a = Trainer(mi, params=prm, seed=11)
    try:
        lr_a, loss_a = _steps(a, data)
        want = a.state()
    finally:
        a.engine.close()
    assert len(set(lr_a)) == 6   # the schedule moves with every step
    names = slot_names(a.options.optimizer, a.options.hyper)
    assert names
    for s in names:   # every slot has left its initial value: dropping one would show
        assert np.any(want["tensors"]["path_update/kernel/%s/%s" % (optimizer["type"], s)] != a.options.slot_init), s

    b = Trainer(mi, params=prm, seed=11)
    path = str(tmp_path / "state-3.safetensors")
    try:
        lr_b, _ = _steps(b, data[:3])
        checkpoint.save_training_state(b.state(), path)
    finally:
        b.engine.close()
    c = Trainer(mi, seed=99)   # other initial parameters, another dropout seed
    try:
        assert c.dropout_seed != 11 and not np.array_equal(c.params()["path_update/kernel"], prm["path_update/kernel"])
        c.load_state(checkpoint.load_training_state(path))
        assert c.iterations == 3 and c.dropout_seed == 11
        lr_c, loss_c = _steps(c, data[3:])
        got = c.state()
    finally:
        c.engine.close()
    assert got["meta"] == want["meta"] and got["meta"]["iterations"] == 6
    assert lr_b + lr_c == lr_a
    assert loss_c == loss_a
    _same_bits(got["tensors"], want["tensors"])


def test_load_state_refuses_another_model(tmp_path):
    """The refusals on a live Trainer (tests/test_training_state_host.py has each by its text): nothing
    of the trainer changes."""
    mi = _model({"type": "Adam"})
    tr = Trainer(mi, seed=1)
    try:
        st = tr.state()
        before = tr.params()
        other = {"meta": dict(st["meta"], optimizer="Adamax"), "tensors": st["tensors"]}
        with pytest.raises(ValueError, match="optimizer"):
            tr.load_state(other)
        less = {"meta": st["meta"], "tensors": {k: v for k, v in st["tensors"].items() if not k.endswith("bias/Adam/m")}}
        with pytest.raises(ValueError, match="lacks"):
            tr.load_state(less)
        _same_bits(tr.params(), before)
        assert tr.iterations == 0
    finally:
        tr.engine.close()


# ---------------------------------------------------------------------------------------------
# the loop
_KEYS = ("save_checkpoints_steps", "input_seed", "native_reader", "check_finite")


@pytest.fixture()
def example_dir(tmp_path):
    d = make("routenet", str(tmp_path / "rn"), "nsfnet", 3)   # 3 samples, batches of 2: they cross the epochs
    model_examples.write(model_examples.routenet(hidden=16, iterations=2), os.path.join(d, "model_description.json"))
    fo.load_config(os.path.join(d, "train_options.ini"))
    gm.register_user_functions(workloads.USER_FUNCTIONS)
    yield d
    fo.CONFIG.remove_option("PATHS", "resume_from")
    for key in _KEYS:
        fo.CONFIG.remove_option("TRAINING_OPTIONS", key)


@pytest.mark.parametrize("native", ["True", "False"], ids=["native_reader", "python_generator"])
def test_loop_resumes_bitwise(example_dir, native):
    opts = fo.CONFIG["TRAINING_OPTIONS"]
    opts["input_seed"], opts["shuffle_train_samples"], opts["batch_size"] = "7", "True", "2"
    opts["save_checkpoints_steps"], opts["eval_samples"], opts["native_reader"] = "2", "2", native
    mi = fo.create_model()
    opts["train_steps"] = "4"
    whole = fo.train_and_evaluate(mi)
    assert {"ckpt-2.safetensors", "state-2.safetensors", "ckpt-4.safetensors", "state-4.safetensors"} <= set(
        os.listdir(whole["model_dir"]))
    opts["train_steps"] = "2"
    first = fo.train_and_evaluate(mi)
    assert first["model_dir"] != whole["model_dir"] and first["trainer"].iterations == 2
    fo.CONFIG["PATHS"]["resume_from"] = first["model_dir"]
    opts["train_steps"] = "4"
    resumed = fo.train_and_evaluate(mi)
    assert resumed["model_dir"] == first["model_dir"] and resumed["trainer"].iterations == 4

    a, b = whole["model_dir"], resumed["model_dir"]
    _same_bits(checkpoint.load_params(os.path.join(a, "ckpt-4.safetensors")),
               checkpoint.load_params(os.path.join(b, "ckpt-4.safetensors")))
    sa = checkpoint.load_training_state(os.path.join(a, "state-4.safetensors"))
    sb = checkpoint.load_training_state(os.path.join(b, "state-4.safetensors"))
    assert sa["meta"] == sb["meta"] and sa["meta"]["iterations"] == 4
    assert sa["meta"]["input"] == {"seed": 7, "world": 1, "batch_size": 2, "shuffle_train_samples": True}
    _same_bits(sa["tensors"], sb["tensors"])
    # the parameter checkpoint holds the parameters only, as before: the state's tensors without the slots
    ck = checkpoint.load_params(os.path.join(b, "ckpt-4.safetensors"))
    assert set(ck) == {n for n, _ in MPPlan.from_model_info(mi).param_specs()}
    # the resumed directory holds both evaluations, the uninterrupted one its own
    steps = [json.loads(l)["step"] for l in open(os.path.join(b, "metrics.jsonl"))]
    assert steps == [2, 4]
    assert [json.loads(l) for l in open(os.path.join(a, "metrics.jsonl"))][-1] == resumed["final_metrics"]
