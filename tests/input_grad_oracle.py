"""The torch-autograd oracle with the input features as leaves: d loss / d(feature values).

oracle/train_oracle.py builds each feature column from numpy inside ``forward_graph``, so autograd
cannot reach it, and oracle/ is not edited.  ``InputGradMixin.forward_graph`` repeats the parent's
state-initialisation lines (h0 = [feature columns | zeros], GM:396-400) with every feature column a
float64 leaf tensor that requires a gradient, then runs the parent's ``_message_passing`` and
``_readout`` unchanged.  The leaves of the last ``forward`` stay in ``self.leaves`` (one dict per
graph); ``feature_grads`` stacks their ``.grad`` per entity in batch row order and plan column order,
the layout of ``Batch.feature_gradients``.

tests/test_input_grad_oracle.py pins the helper to the unchanged oracle by central differences of
the parent's own ``forward``."""
import numpy as np
import torch

from oracle.train_oracle import _T, TorchOracle
from tests import gru_cases


class InputGradMixin:
    def forward_graph(self, x: dict):
        state, leaves = {}, {}
        for ent in self.d["entities"]:
            n = int(np.asarray(x["num_" + ent["name"]]))
            cols, total = [], 0
            for f in ent["features"]:
                size = int(self.dims.get(f["name"], 1))
                total += size
                leaf = torch.tensor(np.asarray(x[f["name"]], np.float64).reshape(n, size), dtype=_T, requires_grad=True)
                leaves[f["name"]] = leaf
                cols.append(leaf)
            H = int(ent["hidden_state_dimension"])
            cols.append(torch.zeros((n, H - total), dtype=_T))
            state[ent["name"]] = torch.cat(cols, 1)
        self.leaves.append(leaves)
        mp_cfg = self.d["message_passing"]
        for _ in range(int(mp_cfg["num_iterations"])):
            for stage in mp_cfg["stages"]:
                for mp in stage["stage_mp"]:
                    self._message_passing(mp, state, x)
        return self._readout(state, x)

    def forward(self, graphs):
        self.leaves = []
        return super().forward(graphs)

    def feature_grads(self):
        """{entity: {feature: d loss / d values [rows of the batch, size]}} of the last backward through
        the last ``forward`` (``loss_and_grads`` runs both).  Entities without features are left out."""
        out = {}
        for ent in self.d["entities"]:
            if not ent["features"]:
                continue
            out[ent["name"]] = {}
            for f in ent["features"]:
                parts = [l[f["name"]].grad if l[f["name"]].grad is not None else torch.zeros_like(l[f["name"]])
                         for l in self.leaves]
                out[ent["name"]][f["name"]] = torch.cat(parts, 0).numpy().copy()
        return out

    def sum_grads(self, graphs, dpred=None):
        """(predictions, feature_grads) for the loss sum(dpred * predictions), dpred default ones."""
        pred = self.forward(graphs)
        w = torch.ones_like(pred) if dpred is None else torch.tensor(np.asarray(dpred, np.float64).reshape(-1), dtype=_T)
        (pred * w).sum().backward()
        return pred.detach().numpy(), self.feature_grads()


class InputGradOracle(InputGradMixin, TorchOracle):
    pass


class CellInputGradOracle(InputGradMixin, gru_cases.CellTorchOracle):
    """The same over tests/gru_cases.py's restatement of a GRU cell with options."""
