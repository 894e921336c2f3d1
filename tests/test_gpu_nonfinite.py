"""The non-finite guard on the GPU: ign_nonfinite_count (Engine.nonfinite_count) against numpy's
isfinite over the kernel's head / body / tail and block edges, Trainer(check_finite=True) raising
NonFiniteTraining at the next step the host waits on, and train_and_evaluate refusing to write a
checkpoint of a poisoned run.  The poison is an infinite label: arithmetic NaNs and Infs only."""
import copy
import glob
import os
import threading

import numpy as np
import pytest
import torch

from examples.make_example import make
from ignnition_amd import _lib, checkpoint, model_examples, synthetic, workloads
from ignnition_amd import framework_operations as fo
from ignnition_amd import generate_model as gm
from ignnition_amd.engine import Engine, MPPlan, device_count
from ignnition_amd.json_operations import Model_information
from ignnition_amd.training import NonFiniteTraining, Trainer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _mi():
    desc = model_examples.routenet(hidden=16, iterations=2)
    _, dims, _ = workloads.model("routenet")
    return Model_information(copy.deepcopy(desc), dims)


@pytest.fixture(scope="module")
def engine():
    eng = Engine(MPPlan.from_model_info(_mi()), 0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)   # the tensors below are torch's
    yield eng
    eng.close()


# ---------------------------------------------------------------------------------------------
# the kernel
NONFINITE = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFABCDEF, 0x7F800000, 0xFF800000]   # NaNs (both signs, payloads), +Inf, -Inf
# finite values one bit away from the exponent test: FLT_MAX (both signs), the largest denormal, the
# smallest one, -0.0, exponent 0xFE with an empty mantissa, the smallest normal
LOOKALIKES = [0x7F7FFFFF, 0xFF7FFFFF, 0x007FFFFF, 0x80000001, 0x80000000, 0x7F000000, 0x00800000]
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2 ** 20 + 3]
BLOCK, GRID = 256 * 4, 256 * 256 * 4   # elements of one block's pass, and of the whole grid's


def _values(n, head):
    """n float32 bit patterns: seeded finite values with the look-alikes spread through them, and a
    non-finite value at the first and last element, on either side of both ends of the 16-byte body,
    of the first block boundary and of the grid's second pass (where n reaches them)."""
    rng = np.random.default_rng(n)
    bits = rng.normal(0, 1e3, n).astype(np.float32).view(np.uint32).copy()
    for k, i in enumerate(range(0, n, 7)):
        bits[i] = LOOKALIKES[k % len(LOOKALIKES)]
    body_end = head + (n - head) // 4 * 4 if n >= head else 0
    at = [0, n - 1, head - 1, head, body_end - 1, body_end, head + BLOCK - 1, head + BLOCK, head + GRID - 1, head + GRID]
    at = sorted({i for i in at if 0 <= i < n})
    for k, i in enumerate(at):
        bits[i] = NONFINITE[k % len(NONFINITE)]
    return bits, len(at)


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "plus4bytes"])
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_count_kernel(engine, n, misaligned):
    head = 3 if misaligned else 0   # scalars in front of the first 16-byte boundary
    bits, planted = _values(n, min(head, n))
    x = bits.view(np.float32)
    expect = int(np.count_nonzero(~np.isfinite(x)))
    assert expect == planted and (n == 0 or expect > 0)
    base = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    t = base[1:] if misaligned else base[:n]
    assert n == 0 or t.data_ptr() % 16 == (4 if misaligned else 0)
    t.copy_(torch.from_numpy(x))
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    engine.nonfinite_count(t, counter)
    assert int(counter.item()) == expect
    engine.nonfinite_count(t, counter)            # two calls into one counter accumulate
    assert int(counter.item()) == 2 * expect
    # every element non-finite: each lane, wave and block contributes
    t.copy_(torch.from_numpy(np.resize(np.array(NONFINITE, np.uint32), n).view(np.float32)))
    counter.zero_()
    engine.nonfinite_count(t, counter)
    assert int(counter.item()) == n
    # and none: the look-alikes alone count nothing
    t.copy_(torch.from_numpy(np.resize(np.array(LOOKALIKES, np.uint32), n).view(np.float32)))
    counter.zero_()
    engine.nonfinite_count(t, counter)
    assert int(counter.item()) == 0


def test_nonfinite_count_argument_checks(engine):
    x = torch.zeros(8, device="cuda")
    c = torch.zeros(1, dtype=torch.int32, device="cuda")
    for dev, cnt in ((None, c.data_ptr()), (x.data_ptr(), None)):
        rc = _lib.lib.ign_nonfinite_count(engine.handle, dev, 8, cnt)
        assert rc == -1 and b"null" in _lib.lib.ign_last_error()
    assert _lib.lib.ign_nonfinite_count(None, x.data_ptr(), 8, c.data_ptr()) == -1
    assert _lib.lib.ign_nonfinite_count(engine.handle, x.data_ptr() + 2, 1, c.data_ptr()) == -1
    assert _lib.lib.ign_nonfinite_count(engine.handle, x.data_ptr(), -1, c.data_ptr()) == -1
    assert _lib.lib.ign_nonfinite_count(engine.handle, x.data_ptr(), 0, c.data_ptr()) == 0   # n == 0: no launch
    with pytest.raises(ValueError, match="float32"):
        engine.nonfinite_count(x.double(), c)
    with pytest.raises(ValueError, match="counter"):
        engine.nonfinite_count(x, torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert int(c.item()) == 0


# ---------------------------------------------------------------------------------------------
# the Trainer
def _batches(mi, poison_step=None):
    out = []
    for k in range(4):
        graphs, labels = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", 2 * k + g) for g in range(2)])
        if poison_step == k + 1:
            labels[0] = labels[0].copy()
            labels[0][0] = np.inf
        out.append((graphs, labels))
    return out


def _run(monkeypatch, check_finite, poison_step):
    """Four steps, only the last one waited for.  Returns (trainer, count launches, the exception or None)."""
    mi = _mi()
    calls = []
    real = Engine.nonfinite_count
    monkeypatch.setattr(Engine, "nonfinite_count", lambda self, t, c: (calls.append(t.numel()), real(self, t, c))[1])
    tr = Trainer(mi, params=MPPlan.from_model_info(mi).init_params(3, bias_scale=0.1), check_finite=check_finite)
    err = None
    try:
        for k, (graphs, labels) in enumerate(_batches(mi, poison_step)):
            tr.train_prepared(*tr.prepare(graphs, labels), want_loss=k == 3)
    except NonFiniteTraining as e:
        err = e
    return tr, calls, err


def test_trainer_raises_at_the_next_waited_step(monkeypatch):
    tr, calls, err = _run(monkeypatch, True, 2)
    try:
        assert isinstance(err, FloatingPointError) and isinstance(err, NonFiniteTraining)
        assert err.first_possible_step <= 2 <= err.detected_step
        assert (err.first_possible_step, err.detected_step) == (1, 4)   # no reading before step 4's loss wait
        assert calls == [tr.engine.n_params] * 3 and tr.iterations == 3  # step 4 was not applied
        with pytest.raises(NonFiniteTraining):
            tr.state()
    finally:
        tr.engine.close()


def test_trainer_without_the_guard_launches_no_count(monkeypatch):
    """check_finite=False: the poisoned run raises nothing and never calls the count.  Engine.stats()
    counts only the forward's timed launches (not the loss / optimizer kernels, nor this one), so the
    launch is counted at the binding, the one place that enqueues it."""
    tr, calls, err = _run(monkeypatch, False, 2)
    try:
        assert err is None and calls == [] and tr.iterations == 4 and tr.nonfinite is None
        st = tr.state()   # the unguarded trainer hands out what it has
        assert not all(np.isfinite(v).all() for v in st["tensors"].values())
    finally:
        tr.engine.close()


def test_guard_leaves_a_clean_run_unchanged(monkeypatch):
    on, calls, err = _run(monkeypatch, True, None)
    off, _, err_off = _run(monkeypatch, False, None)
    try:
        assert err is None and err_off is None and len(calls) == 4
        a, b = on.state(), off.state()
        assert a["meta"] == b["meta"] and a["meta"]["iterations"] == 4
        for k in a["tensors"]:
            np.testing.assert_array_equal(a["tensors"][k].view(np.uint32), b["tensors"][k].view(np.uint32), err_msg=k)
    finally:
        on.engine.close()
        off.engine.close()


# ---------------------------------------------------------------------------------------------
# the loop
@pytest.fixture()
def example_dir(tmp_path):
    d = make("routenet", str(tmp_path / "rn"), "nsfnet", 3)
    model_examples.write(model_examples.routenet(hidden=16, iterations=2), os.path.join(d, "model_description.json"))
    fo.load_config(os.path.join(d, "train_options.ini"))
    gm.register_user_functions(workloads.USER_FUNCTIONS)
    yield d
    gm.register_user_functions(workloads.USER_FUNCTIONS)
    for key in ("save_checkpoints_steps", "input_workers", "input_seed", "check_finite"):
        fo.CONFIG.remove_option("TRAINING_OPTIONS", key)


def test_loop_writes_nothing_after_the_poisoned_step(example_dir):
    """The label normalisation returns Inf for the third training batch (the training stream's loads
    run on the one builder thread, the evaluation's on the main thread).  The checkpoint at step 2 is
    clean and stays the newest; the one at step 4 raises instead of writing."""
    seen = []

    def log(feature, feature_name):
        out = np.log(feature)
        if threading.current_thread() is not threading.main_thread():
            seen.append(feature_name)
            if len(seen) == 3:
                out = np.full_like(out, np.inf)
        return out

    gm.register_user_functions({"log": log})
    opts = fo.CONFIG["TRAINING_OPTIONS"]
    opts["train_steps"], opts["batch_size"], opts["eval_samples"] = "6", "2", "2"
    opts["save_checkpoints_steps"], opts["input_workers"], opts["input_seed"] = "2", "1", "3"
    mi = fo.create_model()
    with pytest.raises(NonFiniteTraining) as ei:
        fo.train_and_evaluate(mi, log_every=100)
    assert ei.value.first_possible_step <= 3 <= ei.value.detected_step == 4
    (exp,) = glob.glob(os.path.join(example_dir, "CheckPoints", "experiment_*"))
    assert sorted(os.listdir(exp)) == ["ckpt-2.safetensors", "state-2.safetensors"]
    path, st = checkpoint.latest_state(exp)
    assert path.endswith("state-2.safetensors") and st["meta"]["iterations"] == 2
    assert all(np.isfinite(v).all() for v in st["tensors"].values())
