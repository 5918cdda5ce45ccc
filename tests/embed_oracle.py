"""CPU restatement of Ultralytics feature embeddings — `BaseModel._predict_once(x, embed=...)` (8.3.x, restated from
memory: the package is not available offline), over the oracle network (oracle/yolo11.py).  TEST INFRASTRUCTURE ONLY.

    embed = frozenset(embed); for every layer m in index order: x = m(x); if m.i in embed:
        embeddings.append(adaptive_avg_pool2d(x, (1, 1)).squeeze(-1).squeeze(-1))          # (B, C_i)
        if m.i == max(embed): return torch.unbind(torch.cat(embeddings, 1), dim=0)

So the slices come in ascending layer order whatever order the caller wrote, a duplicate index counts once, and nothing
behind the last named layer runs.  `Model.embed(source)` is `predict(source, embed=[len(model.model) - 2])`: layer 22.

The Upsample (11, 14) and Concat (12, 15, 18, 21) outputs are rebuilt here from their inputs (F.interpolate(nearest),
torch.cat), the way the GPU plan sees them: it never materialises either.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch
import torch.nn.functional as F

N_LAYERS = 23
UPSAMPLE = {11: 10, 14: 13}                                  # layer -> its source
CONCAT = {12: (11, 6), 15: (14, 4), 18: (17, 13), 21: (20, 10)}  # layer -> its inputs, in concat order
DEFAULT = (N_LAYERS - 1,)


def _compute_layers(layers) -> set:
    """The layers the network itself has to return so that every requested output can be formed."""
    need, todo = set(), list(layers)
    while todo:
        i = todo.pop()
        if i in UPSAMPLE:
            todo.append(UPSAMPLE[i])
        elif i in CONCAT:
            todo.extend(CONCAT[i])
        else:
            need.add(i)
    return need


@torch.no_grad()
def layer_outputs(net, x: torch.Tensor, layers: Sequence[int]) -> Dict[int, torch.Tensor]:
    """NCHW outputs of the named layers for the preprocessed batch x, in the dtype of `net` and x."""
    _, saved = net(x, keep=tuple(sorted(_compute_layers(layers))))

    def out(i):
        if i in UPSAMPLE:
            return F.interpolate(out(UPSAMPLE[i]), scale_factor=2, mode="nearest")
        if i in CONCAT:
            return torch.cat([out(j) for j in CONCAT[i]], 1)
        return saved[i]

    return {i: out(i) for i in layers}


def pooled(t: torch.Tensor) -> torch.Tensor:
    return F.adaptive_avg_pool2d(t, (1, 1)).squeeze(-1).squeeze(-1)


@torch.no_grad()
def embed(net, x: torch.Tensor, layers: Sequence[int] = DEFAULT):
    """_predict_once(x, embed=layers): a tuple of B 1-D tensors."""
    idx = sorted(frozenset(int(i) for i in layers))
    outs = layer_outputs(net, x, idx)
    return torch.unbind(torch.cat([pooled(outs[i]) for i in idx], 1), dim=0)


def preprocess(x: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """predict's tensor preprocessing (LoadTensor's /255 rule), then the working dtype."""
    from oracle import postprocess as pp
    return pp.load_tensor_check(x.float().cpu()).to(dtype)
