"""The torch-autograd oracle with the per-edge parameters as leaves: d loss / d(params_<adj>).

oracle/train_oracle.py turns ``x["params_<adj>"]`` into a constant inside ``_message_passing``
(``torch.tensor(np.asarray(x[...], np.float64).reshape(len(src_idx), -1))``), once per MP source and
iteration, so autograd cannot reach it, and oracle/ is not edited.  ``EdgeParamGradMixin.forward_graph``
hands the parent a copy of the graph whose ``params_<adj>`` arrays are float64 arrays the helper owns,
and for the time of the parent's ``forward_graph`` the name ``torch`` in the oracle's module is a proxy
whose ``tensor`` answers a view of exactly such an array (``np.asarray`` returns a float64 array as it
is, ``reshape`` a view whose base it is) with the array's float64 leaf tensor, reshaped alike, and is
``torch.tensor`` for everything else; every other attribute is torch's.  Each read of the array, by
whichever MP source and iteration, thus reads the one leaf, and ``.grad`` is the gradient with respect
to the ``params_<adj>`` the caller supplied.  The leaves of the last ``forward`` stay in ``self.leaves``
(one dict per graph); ``edge_param_grads`` stacks their ``.grad`` in batch edge order, the layout of
``Batch.edge_param_gradients``.

tests/test_edge_param_grad_oracle.py pins the helper to the unchanged oracle: the same forward to the
bit, and central differences of the parent's own ``forward``."""
import numpy as np
import torch

from oracle import train_oracle
from oracle.train_oracle import _T, TorchOracle


class _TorchWithLeaves:
    """``torch`` with ``tensor`` answering the registered arrays' views by their leaves."""

    def __init__(self, leaves):
        self._leaves = leaves   # [(array, leaf)]

    def __getattr__(self, name):
        return getattr(torch, name)

    def tensor(self, data, *args, **kwargs):
        if isinstance(data, np.ndarray):
            for arr, leaf in self._leaves:
                if data is arr or data.base is arr:
                    return leaf.reshape(data.shape)
        return torch.tensor(data, *args, **kwargs)


class EdgeParamGradMixin:
    def forward_graph(self, x: dict):
        x = dict(x)
        leaves, pairs = {}, []
        for key in [k for k in x if k.startswith("params_")]:
            n = len(np.asarray(x["src_" + key[len("params_"):]]).reshape(-1))
            arr = np.array(x[key], np.float64).reshape(n, -1).copy()   # owns its data: the base of its views
            leaf = torch.tensor(arr, dtype=_T, requires_grad=True)
            x[key] = arr
            leaves[key] = leaf
            pairs.append((arr, leaf))
        self.leaves.append(leaves)
        train_oracle.torch = _TorchWithLeaves(pairs)
        try:
            return super().forward_graph(x)
        finally:
            train_oracle.torch = torch

    def forward(self, graphs):
        self.leaves = []
        return super().forward(graphs)

    def edge_param_grads(self):
        """{"params_<adj>": d loss / d values [edges of the batch, param_dim]} of the last backward
        through the last ``forward`` (``loss_and_grads`` runs both); an array nothing read: zeros."""
        out = {}
        for key in self.leaves[0]:
            parts = [l[key].grad if l[key].grad is not None else torch.zeros_like(l[key]) for l in self.leaves]
            out[key] = torch.cat(parts, 0).numpy().copy()
        return out

    def sum_grads(self, graphs, dpred=None):
        """(predictions, edge_param_grads) for the loss sum(dpred * predictions), dpred default ones."""
        pred = self.forward(graphs)
        w = torch.ones_like(pred) if dpred is None else torch.tensor(np.asarray(dpred, np.float64).reshape(-1), dtype=_T)
        (pred * w).sum().backward()
        return pred.detach().numpy(), self.edge_param_grads()


class EdgeParamGradOracle(EdgeParamGradMixin, TorchOracle):
    pass
