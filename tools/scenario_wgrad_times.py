"""Times of Batch.scenario_parameter_gradients under §3p's protocol: one RouteNet synth50 graph,
T = 8, S random feature sets and cotangents; a host clock around calls that return host results; two warm-up
rounds, then seven rounds alternating the ways in one process; median [min, max] ms.  The ways: the pass in its
default form, with IGN_SCEN_WGRAD_FUSED=0, scenario_gradients on the same inputs, and S rounds of set_features +
forward_train + backward on a training-enabled batch.

    python tools/scenario_wgrad_times.py [--hidden 32] [--scenarios 16 64 200]"""
import argparse
import copy
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ignnition_amd import workloads   # noqa: E402
from ignnition_amd.engine import Batch, Engine, MPPlan   # noqa: E402
from ignnition_amd.json_operations import Model_information   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--scenarios", type=int, nargs="+", default=[16, 64, 200])
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    desc, dims, _, graphs, _ = workloads.make_batch_inputs("routenet", "synth50", 1)
    desc = copy.deepcopy(desc)
    for e in desc["entities"]:
        e["hidden_state_dimension"] = args.hidden
    plan = MPPlan.from_model_info(Model_information(desc, dims))
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(0, bias_scale=0.05))
    b, bt = Batch(eng, graphs), Batch(eng, graphs)
    bt.enable_training()
    grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(0)
    for S in args.scenarios:
        feats = {ent: rng.uniform(-1, 1, (S, rows, sum(size for _, size in fs))).astype(np.float32)
                 for ent, fs, rows in zip(plan.entities, plan.features, b.rows) if fs}
        w = rng.standard_normal((S, b.predictions, b.output_units)).astype(np.float32)
        wd = torch.tensor(w, device="cuda")

        def params(fused):
            os.environ["IGN_SCEN_WGRAD_FUSED"] = fused
            try:
                return b.scenario_parameter_gradients(feats, w)[1]
            finally:
                del os.environ["IGN_SCEN_WGRAD_FUSED"]

        def training():
            total = torch.zeros_like(grads)
            for s in range(S):
                for ent, a in feats.items():
                    bt.set_features(ent, a[s])
                bt.forward_train(to_host=False)
                bt.backward(wd[s].reshape(-1), grads)
                total += grads
            return total.cpu().numpy()

        ways = {"params": lambda: params("1"), "params unfused": lambda: params("0"),
                "scenario_gradients": lambda: b.scenario_gradients(feats, w), "S training rounds": training}
        ms = {k: [] for k in ways}
        for r in range(2 + args.rounds):
            for k, f in ways.items():
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                if r >= 2:
                    ms[k].append(1e3 * (time.perf_counter() - t0))
        got, ref = params("1"), training()
        flat = np.concatenate([got[name].reshape(-1) for name, _, _ in eng.layout])
        want = np.concatenate([ref[off:off + int(np.prod(shape))] for _, shape, off in eng.layout])
        print("H %d S %d: " % (args.hidden, S) + "; ".join("%s %.2f [%.2f, %.2f]" % (k, np.median(v), min(v), max(v)) for k, v in ms.items())
              + "; against the training rounds' summed gradient, relative L2 %.3g" % (np.linalg.norm(flat - want) / np.linalg.norm(want)),
              flush=True)


if __name__ == "__main__":
    main()
