"""Training state without a GPU: the slot names, the state file (checkpoint.save_training_state /
load_training_state / latest_state), the layout-independent packing of the optimizer's slot buffers
(training.pack_state / unpack_state, which Trainer.state / load_state go through) with each refusal,
the input streams' skip, and train_and_evaluate's resume_from validation."""
import copy
import itertools
import os

import numpy as np
import pytest

from examples.make_example import make
from ignnition_amd import checkpoint, model_examples, workloads
from ignnition_amd import framework_operations as fo
from ignnition_amd import generate_model as gm
from ignnition_amd.json_operations import Model_information
from ignnition_amd.training import (cut_flat, fill_flat, learning_options, pack_state, slot_names, unpack_state)

F32 = np.float32


def _options(optimizer):
    desc = model_examples.routenet(hidden=16, iterations=2)
    desc["learning_options"] = {"loss": "MeanSquaredError", "optimizer": dict(optimizer)}
    _, dims, _ = workloads.model("routenet")
    return learning_options(Model_information(copy.deepcopy(desc), dims))


# two layouts of the same three tensors: other gaps, another total
SHAPES = [("a/kernel", (3, 5)), ("a/bias", (5,)), ("b/kernel", (2, 2))]
LAYOUT_A = [(n, s, off) for (n, s), off in zip(SHAPES, (0, 64, 128))]
LAYOUT_B = [(n, s, off) for (n, s), off in zip(SHAPES, (7, 22, 40))]
N_A, N_B = 192, 50


def _gaps(layout, n):
    used = np.zeros(n, bool)
    for _, shape, off in layout:
        used[off:off + int(np.prod(shape))] = True
    return ~used


def _fake_state(lo, layout, n, seed=0, iterations=3):
    rng = np.random.default_rng(seed)
    params = {name: rng.normal(size=shape).astype(F32) for name, shape, _ in layout}
    slots = []
    for _ in range(lo.num_slots):
        flat = np.full(n, 123.0, F32)   # what a gap holds must not reach the file
        for _, shape, off in layout:
            flat[off:off + int(np.prod(shape))] = rng.normal(size=int(np.prod(shape))).astype(F32)
        slots.append(flat)
    return pack_state(params, slots, lo, layout, iterations, 0xFEDCBA9876543210), params, slots


@pytest.mark.parametrize("optimizer,names", [
    ({"type": "Adam"}, ["m", "v"]), ({"type": "Adamax"}, ["m", "v"]), ({"type": "SGD"}, []),
    ({"type": "SGD", "momentum": 0.9}, ["momentum"]), ({"type": "RMSprop"}, ["rms"]),
    ({"type": "RMSprop", "centered": True}, ["rms", "mg"]), ({"type": "RMSprop", "momentum": 0.5}, ["rms", "momentum"]),
    ({"type": "RMSprop", "centered": True, "momentum": 0.5}, ["rms", "mg", "momentum"]),
    ({"type": "Adagrad"}, ["accumulator"]), ({"type": "Adadelta"}, ["accum_grad", "accum_var"])])
def test_slot_names_follow_the_engines_slot_order(optimizer, names):
    lo = _options(optimizer)
    assert slot_names(lo.optimizer, lo.hyper) == names
    assert len(names) == lo.num_slots   # ign_optimizer_num_slots
    st, _, _ = _fake_state(lo, LAYOUT_A, N_A)
    want = {n for n, _, _ in LAYOUT_A} | {"%s/%s/%s" % (n, lo.optimizer, s) for n, _, _ in LAYOUT_A for s in names}
    assert set(st["tensors"]) == want


def test_state_file_round_trip(tmp_path):
    lo = _options({"type": "RMSprop", "centered": True, "momentum": 0.5, "rho": 0.85})
    st, _, _ = _fake_state(lo, LAYOUT_A, N_A)
    st["meta"]["input"] = {"seed": 12345, "world": 1, "batch_size": 2, "shuffle_train_samples": True}
    path = str(tmp_path / "state-3.safetensors")
    checkpoint.save_training_state(st, path)
    assert sorted(os.listdir(tmp_path)) == ["state-3.safetensors"]   # no .tmp left behind
    back = checkpoint.load_training_state(path)
    assert back["meta"] == st["meta"]
    assert back["meta"]["dropout_seed"] == 0xFEDCBA9876543210 and back["meta"]["iterations"] == 3
    assert back["meta"]["hyper"] == lo.hyper and back["meta"]["optimizer"] == "RMSprop"
    assert back["meta"]["loss"] == "MeanSquaredError" and back["meta"]["slot_init"] == 0.0
    assert set(back["tensors"]) == set(st["tensors"])
    for k, v in st["tensors"].items():
        assert back["tensors"][k].dtype == np.float32 and back["tensors"][k].shape == v.shape
        np.testing.assert_array_equal(back["tensors"][k].view(np.uint32), v.view(np.uint32))
    # a parameter checkpoint is not a state
    checkpoint.save_params({"a/kernel": np.zeros((3, 5), F32)}, str(tmp_path / "ckpt-3.safetensors"), {"step": 3})
    with pytest.raises(ValueError, match="holds no training state"):
        checkpoint.load_training_state(str(tmp_path / "ckpt-3.safetensors"))


def test_state_does_not_depend_on_the_layouts_gaps():
    """Packed through one layout and unpacked through another: every tensor lands at the other layout's
    offset and the gaps hold slot_init, whatever the source buffer's gaps held."""
    lo = _options({"type": "Adagrad", "initial_accumulator_value": 0.25})
    assert lo.slot_init == 0.25
    st, params, slots = _fake_state(lo, LAYOUT_A, N_A)
    p2, s2 = unpack_state(st, lo, LAYOUT_B, N_B)
    assert len(s2) == 1 and s2[0].shape == (N_B,) and s2[0].dtype == np.float32
    gaps = _gaps(LAYOUT_B, N_B)
    assert gaps.any() and np.all(s2[0][gaps] == F32(0.25))
    for name, shape, off in LAYOUT_B:
        np.testing.assert_array_equal(p2[name], params[name])
        src = dict((n, o) for n, _, o in LAYOUT_A)[name]
        k = int(np.prod(shape))
        np.testing.assert_array_equal(s2[0][off:off + k], slots[0][src:src + k])
    # and cut_flat / fill_flat are each other's inverse on the tensors
    again = cut_flat(fill_flat(cut_flat(slots[0], LAYOUT_A), LAYOUT_A, N_A, 9.0), LAYOUT_A)
    for name, shape, off in LAYOUT_A:
        np.testing.assert_array_equal(again[name].reshape(-1), slots[0][off:off + int(np.prod(shape))])


def test_load_state_refusals():
    lo = _options({"type": "Adam"})
    st, _, _ = _fake_state(lo, LAYOUT_A, N_A)
    unpack_state(st, lo, LAYOUT_A, N_A)
    with pytest.raises(ValueError, match="trained with optimizer Adam, the model description names Adamax"):
        unpack_state(st, _options({"type": "Adamax"}), LAYOUT_A, N_A)
    with pytest.raises(ValueError, match="hyper-parameter beta_2 is 0.999 in the state and 0.99 in the model"):
        unpack_state(st, _options({"type": "Adam", "beta_2": 0.99}), LAYOUT_A, N_A)
    less = {"meta": st["meta"], "tensors": {k: v for k, v in st["tensors"].items() if k != "a/bias/Adam/v"}}
    with pytest.raises(ValueError, match=r"the state lacks tensor\(s\) a/bias/Adam/v"):
        unpack_state(less, lo, LAYOUT_A, N_A)
    more = {"meta": st["meta"], "tensors": dict(st["tensors"], **{"c/kernel": np.zeros(2, F32)})}
    with pytest.raises(ValueError, match="the model does not have: c/kernel"):
        unpack_state(more, lo, LAYOUT_A, N_A)
    bad = {"meta": st["meta"], "tensors": dict(st["tensors"], **{"a/kernel/Adam/m": np.zeros((5, 3), F32)})}
    with pytest.raises(ValueError, match=r"a/kernel/Adam/m has shape \(5, 3\) in the state, the model needs \(3, 5\)"):
        unpack_state(bad, lo, LAYOUT_A, N_A)


def test_latest_state_skips_a_truncated_file(tmp_path, caplog):
    lo = _options({"type": "Adam"})
    assert checkpoint.latest_state(str(tmp_path)) is None
    for step in (2, 4, 10):
        st, _, _ = _fake_state(lo, LAYOUT_A, N_A, seed=step, iterations=step)
        checkpoint.save_training_state(st, str(tmp_path / ("state-%d.safetensors" % step)))
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    path, st = checkpoint.latest_state(str(tmp_path))
    assert path.endswith("state-10.safetensors") and st["meta"]["iterations"] == 10   # by number, not by name
    newest = tmp_path / "state-10.safetensors"
    data = newest.read_bytes()
    newest.write_bytes(data[:len(data) // 2])
    with caplog.at_level("WARNING", logger="ignnition_amd"):
        path, st = checkpoint.latest_state(str(tmp_path))
    assert path.endswith("state-4.safetensors") and st["meta"]["iterations"] == 4
    assert "state-10.safetensors" in caplog.text


# ---------------------------------------------------------------------------------------------
# the input position
@pytest.fixture()
def example_dir(tmp_path):
    d = make("routenet", str(tmp_path / "rn"), "nsfnet", 3)
    fo.load_config(os.path.join(d, "train_options.ini"))
    gm.register_user_functions(workloads.USER_FUNCTIONS)
    yield d
    for section, key in (("PATHS", "resume_from"), ("PATHS", "warm_start_path")):
        fo.CONFIG.remove_option(section, key)


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("shuffle", [False, True])
def test_skip_is_the_tail_of_the_full_stream(example_dir, shuffle, world):
    """3 samples, batches of 2 per rank: skipping 2 batches (4 or 8 samples) crosses an epoch end."""
    mi = fo.create_model()
    gm.set_model_info(mi)
    path = fo.CONFIG["PATHS"]["train_dataset"]
    k, take = 2, 4
    for rank in range(world):
        kw = dict(shuffle=shuffle, batch_size=2, seed=17, rank=rank, world=world)
        full = list(itertools.islice(gm.NativeInput(path, **kw).ids(), k + take))
        assert list(itertools.islice(gm.NativeInput(path, **kw).ids(skip=k), take)) == full[k:]
        assert list(itertools.islice(gm.NativeInput(path, **kw).ids(skip=0), k + take)) == full
        if shuffle:   # the stream really is shuffled and crosses epochs, or the comparison shows nothing
            assert len({tuple(b) for b in full}) > 2
        lab = lambda ys: [np.asarray(y, np.float64).reshape(-1).tolist() for y in ys]
        whole = [lab(ys) for _, ys in itertools.islice(gm.input_fn(path, **kw), k + take)]
        assert [lab(ys) for _, ys in itertools.islice(gm.input_fn(path, skip=k, **kw), take)] == whole[k:]
        assert [lab(ys) for _, ys in itertools.islice(gm.input_fn(path, skip=0, **kw), k + take)] == whole


def test_resume_from_validation(example_dir, tmp_path):
    mi = fo.create_model()
    exp = tmp_path / "experiment_x"
    exp.mkdir()
    lo = _options({"type": "Adam"})
    st, _, _ = _fake_state(lo, LAYOUT_A, N_A)
    st["meta"]["input"] = {"seed": 5, "world": 2, "batch_size": 8, "shuffle_train_samples": True}
    checkpoint.save_training_state(st, str(exp / "state-3.safetensors"))
    fo.CONFIG["PATHS"]["resume_from"] = str(exp)
    with pytest.raises(ValueError, match="written with world 2, this run has 1"):
        fo.train_and_evaluate(mi)
    fo.CONFIG["PATHS"]["resume_from"] = str(exp / "state-3.safetensors")   # the file itself, too
    with pytest.raises(ValueError, match="written with world 2, this run has 1"):
        fo.train_and_evaluate(mi)
    st["meta"]["input"]["world"] = 1
    checkpoint.save_training_state(st, str(exp / "state-3.safetensors"))
    fo.CONFIG["TRAINING_OPTIONS"]["batch_size"] = "4"
    with pytest.raises(ValueError, match="written with batch_size 8, this run has 4"):
        fo.train_and_evaluate(mi)
    fo.CONFIG["TRAINING_OPTIONS"]["batch_size"] = "8"
    fo.CONFIG["TRAINING_OPTIONS"]["shuffle_train_samples"] = "False"
    with pytest.raises(ValueError, match="written with shuffle_train_samples True, this run has False"):
        fo.train_and_evaluate(mi)
    fo.CONFIG["PATHS"]["warm_start_path"] = str(exp / "state-3.safetensors")
    with pytest.raises(ValueError, match="resume_from and warm_start_path are both set"):
        fo.train_and_evaluate(mi)
    fo.CONFIG.remove_option("PATHS", "warm_start_path")
    fo.CONFIG["PATHS"]["resume_from"] = str(tmp_path)   # a directory without state files
    with pytest.raises(ValueError, match="no readable state"):
        fo.train_and_evaluate(mi)
