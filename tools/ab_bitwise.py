"""Bitwise A/B of two library builds (GPU box): the default RouteNet synth50 batch (or --model /
--topology / --graphs) through each ignnition_amd/ab/lib_<name>.so in its own process
(IGN_LIB_PATH), predictions compared bit for bit.  --train compares the parameter gradients of one backward instead (dpred = a
fixed seeded vector).
    python tools/ab_bitwise.py base new [--graphs 512] [--model routenet] [--topology synth50] [--train]
--cases runs the models of the tests' case modules instead (predict_cases and its H = 64 model, test_gpu_dropout's GRAD_CASES
with its mask stream, layernorm_cases' GRAD_CASES, readout_cases, test_gpu_training's message-network
parameter sets, aggregation_cases' and readout_op_cases' tables), all of them in one process per library, and compares per case the training forward's
predictions and the flat gradient of one backward; for the H = 64, LayerNormalization, readout-operation
and message-network cases the inference forward too.
(Against a parent commit: tools/build_ab.sh base in a checkout of it, its lib_base.so copied to this ab/.)
    python tools/ab_bitwise.py base new --cases"""
import argparse
import copy
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r)
from ignnition_amd import workloads
from ignnition_amd.engine import Batch, Engine, MPPlan
desc, dims, mi, graphs, _ = workloads.make_batch_inputs(%r, %r, %d)
plan = MPPlan.from_model_info(mi)
prm = plan.init_params(1, bias_scale=0.05)
eng = Engine(plan, 0); eng.set_params(prm)
b = Batch(eng, graphs)
if not %r:
    np.save(%r, b.forward().reshape(-1))
else:
    import torch
    b.enable_training()
    pred = b.forward_train(to_host=False)
    n = b.predictions * b.output_units
    dpred = torch.from_numpy(np.random.default_rng(3).standard_normal(n).astype(np.float32)).cuda()
    grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    b.backward(dpred, grads)
    torch.cuda.synchronize()
    np.save(%r, grads.cpu().numpy())
'''


def cases():
    """(name, description, dimensions, graphs, parameters, Dropout stream or None, inference too)"""
    from ignnition_amd import model_examples, synthetic, workloads
    from ignnition_amd.engine import MPPlan
    from ignnition_amd.json_operations import Model_information
    from tests import dropout_cases as dc, layernorm_cases as lc, predict_cases as pc
    from tests import test_gpu_dropout as td, test_gpu_layernorm as tl, test_gpu_training as tt
    from tests.readout_cases import READOUT_CASES
    for c in sorted(pc.PREDICT_CASES):
        desc, dims, _, graphs, _, prm = pc.predict_inputs(c)
        yield "predict/" + c, desc, dims, graphs, prm, None, False
    desc, dims, _, graphs, _, prm = pc.predict_inputs(*pc.WIDE)   # H = 64: IGN_SUM_VARIANT's three kernels
    yield "predict/%s_h%d" % pc.WIDE, desc, dims, graphs, prm, None, True
    for c in sorted(td.GRAD_CASES):
        desc = td.GRAD_CASES[c]()
        dims, _, graphs, _, prm = dc.inputs(desc)
        yield "dropout/" + c, desc, dims, graphs, prm, (td.SEED, td.STEP), False
    for c in sorted(lc.GRAD_CASES):   # (the mask stream where the case has a Dropout)
        desc = lc.GRAD_CASES[c]()
        dims, plan, graphs, _, prm = lc.inputs(desc)
        yield "layernorm/" + c, desc, dims, graphs, prm, (tl.SEED, tl.STEP) if plan.dropout_sites() else None, True
    for c in sorted(READOUT_CASES):   # test_gradients_readout_operations' batch
        ops, pin, nets = READOUT_CASES[c]
        desc = model_examples.routenet_readout(ops, pin, nets, iterations=3)
        _, dims, _ = workloads.model("routenet")
        mi = Model_information(copy.deepcopy(desc), dims)
        graphs, _ = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet" if g % 2 == 0 else "geant2", g)
                                                for g in range(3)])
        yield "readout/" + c, desc, dims, graphs, MPPlan.from_model_info(mi).init_params(11, bias_scale=0.1), None, True
    for k, args in enumerate(tt.test_gradients_message_networks.pytestmark[0].args[1]):
        desc, dims, graphs, _, prm = tt._msg_net_case(*args)
        yield "msgnet/%d" % k, desc, dims, graphs, prm, None, True
    for k, inputs in enumerate(tt.test_gradients_attention_over_message_network.pytestmark[0].args[1]):
        desc, dims, graphs, _, _ = tt._msg_net_case(inputs, (32,), "tanh")
        desc["message_passing"]["stages"][1]["stage_mp"][0]["aggregation"] = {"type": "attention"}
        prm = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)).init_params(8, bias_scale=0.1)
        yield "attention_msgnet/%d" % k, desc, dims, graphs, prm, None, True
    from tests import aggregation_cases as ac   # attention, convolution and concat MPs on their kernels' edges
    for c in sorted(ac.CASES):
        desc, dims, _, _, graphs, _, prm = ac.case_inputs(c)
        yield "aggregation/" + c, desc, dims, graphs, prm, None, True
    from tests import readout_op_cases as rc   # the readout operations on their kernels' edges
    for c in rc.ALL:
        desc, dims, _, _, graphs, _, prm = rc.case_inputs(c)
        yield "readout_op/" + c, desc, dims, graphs, prm, None, True


def run_cases(out):
    import torch
    from ignnition_amd.engine import Batch, Engine, MPPlan
    from ignnition_amd.json_operations import Model_information
    res = {}
    for name, desc, dims, graphs, prm, stream, infer in cases():
        eng = Engine(MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)), 0)
        eng.set_params(prm)
        b = Batch(eng, graphs)
        if infer:
            res[name + " infer"] = b.forward().reshape(-1).copy()
        b.enable_training()
        if stream:
            b.set_dropout(*stream)
        res[name + " pred"] = b.forward_train().reshape(-1).copy()
        n = b.predictions * b.output_units
        dpred = torch.from_numpy(np.random.default_rng(3).standard_normal(n).astype(np.float32)).cuda()
        grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
        b.backward(dpred, grads)
        torch.cuda.synchronize()
        res[name + " grad"] = grads.cpu().numpy()
        b.close()
        eng.close()
        print("ran", name, file=sys.stderr, flush=True)
    np.savez(out, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--model", default="routenet")
    ap.add_argument("--topology", default="synth50")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--cases", action="store_true")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, REPO)
        return run_cases(a.child)
    outs = {}
    os.makedirs(os.path.join(REPO, "gpurun_out", "ab"), exist_ok=True)
    for name in a.libs:
        f = os.path.join(REPO, "gpurun_out", "ab", "pred_%s.npy" % name)
        if a.cases:
            f = os.path.splitext(f)[0] + ".npz"   # one array per case and output
        env = dict(os.environ, IGN_AB_LIB="1", IGN_LIB_PATH=os.path.join(REPO, "ignnition_amd", "ab", "lib_%s.so" % name))
        if a.cases:
            subprocess.run([sys.executable, os.path.abspath(__file__), name, "--child", f], env=env, check=True, timeout=500)
            outs[name] = dict(np.load(f))
        else:
            subprocess.run([sys.executable, "-c", CHILD % (REPO, a.model, a.topology, a.graphs, a.train, f, f)], env=env,
                           check=True, timeout=300)
            outs[name] = {"": np.load(f)}
    base = a.libs[0]
    for name in a.libs[1:]:
        assert outs[name].keys() == outs[base].keys()
        for k, ref in outs[base].items():
            got = outs[name][k]
            d = got.view(np.uint32) != ref.view(np.uint32)   # bits: a NaN equals itself, -0 is not +0
            print("%s%s vs %s: %d of %d values differ (max |diff| %.3g)" % (k and k + ": ", name, base, int(d.sum()), d.size,
                  float(np.abs(got.astype(np.float64) - ref).max())), flush=True)


if __name__ == "__main__":
    main()
