"""Parameter checkpoints and training-state files (safetensors, Keras-style tensor names).

Replaces the reference's Estimator checkpoints / Saver restore (FO:126-129, 141-145,
218-221), which need TensorFlow.  Tensor names follow the engine layout
(``path_update/kernel``, ``readout_model_0/1st_dense_layer/kernel`` ...).

* ``ckpt-<step>.safetensors``: the parameters (``save_params`` / ``load_params``), what ``predict``
  and ``warm_start`` read.
* ``state-<step>.safetensors``: everything a run needs to continue exactly (``Trainer.state()``):
  the parameters, every optimizer slot as per-parameter tensors ``<param>/<Optimizer>/<slot>``, and
  the metadata (step, dropout seed, optimizer configuration, the input stream's seed and shape) as
  one JSON document under the file's ``training_state`` metadata key.  DESIGN.md §3j.
"""

from __future__ import annotations

import glob
import json
import logging
import os
import re

import numpy as np

log = logging.getLogger("ignnition_amd")

STATE_KEY = "training_state"
_STATE_FILE = re.compile(r"state-(\d+)\.safetensors$")


def save_params(params: dict, path: str, metadata: dict | None = None):
    from safetensors.numpy import save_file
    save_file({k: np.ascontiguousarray(v, np.float32) for k, v in params.items()}, path,
              metadata={k: str(v) for k, v in (metadata or {}).items()})


def load_params(path: str) -> dict:
    from safetensors.numpy import load_file
    return dict(load_file(path))


def save_training_state(state: dict, path: str):
    """``state``: {"tensors": {name: array}, "meta": a JSON-able dict} -> one safetensors file.  Written
    beside ``path`` and moved into place, so a run killed while writing leaves the previous newest
    file the newest one."""
    from safetensors.numpy import save_file
    tmp = path + ".tmp"
    save_file({k: np.ascontiguousarray(v, np.float32) for k, v in state["tensors"].items()}, tmp,
              metadata={STATE_KEY: json.dumps(state["meta"], sort_keys=True)})
    os.replace(tmp, path)


def load_training_state(path: str) -> dict:
    """The state ``save_training_state`` wrote.  Raises ValueError for a file that is not a training
    state, and whatever safetensors raises for a truncated one."""
    from safetensors import safe_open
    with safe_open(path, framework="numpy") as f:
        meta = (f.metadata() or {}).get(STATE_KEY)
        if meta is None:
            raise ValueError("%s holds no training state (a ckpt-* file holds the parameters only)" % path)
        tensors = {k: f.get_tensor(k) for k in f.keys()}
    return {"tensors": tensors, "meta": json.loads(meta)}


def state_files(directory: str) -> list:
    """[(step, path)] of the ``state-<step>.safetensors`` files of a directory, by rising step."""
    out = []
    for p in glob.glob(os.path.join(glob.escape(directory), "state-*.safetensors")):
        m = _STATE_FILE.search(os.path.basename(p))
        if m:
            out.append((int(m.group(1)), p))
    return sorted(out)


def latest_state(directory: str):
    """(path, state) of the highest-step state file of ``directory`` that loads, or None.  A file that
    does not load (truncated by a full disk or a kill outside the writer) is skipped with a warning."""
    for _, path in reversed(state_files(directory)):
        try:
            return path, load_training_state(path)
        except Exception as e:   # noqa: BLE001 (safetensors raises its own error types)
            log.warning("IGNNITION: skipping the unreadable state file %s (%s)", path, e)
    return None
