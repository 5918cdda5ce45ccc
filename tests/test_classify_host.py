"""Host tests of classification: the classify graph and its parameters, architecture inference, the synthetic weights'
softmax conditions (float64 oracle, tests/classify_oracle.py), the facade's refusal and the image transform."""
import numpy as np
import pytest
import torch

from tests import classify_oracle as CO
from yolomi.arch import GraphBuilder, infer_arch
from yolomi.synth import synth_weights

CASES = [("n", 1000, 32, 32, 5), ("n", 37, 96, 160, 3), ("n", 1000, 224, 224, 2), ("s", 2, 160, 224, 1),
         ("n", 37, 320, 288, 9)]  # the GPU tests'


@pytest.mark.parametrize("scale,nc,c1", [("n", 1000, 256), ("n", 37, 256), ("s", 1000, 512), ("s", 37, 512)])
def test_infer_arch_and_head_parameters(scale, nc, c1):
    sd = synth_weights(scale, "classify", 0, nc=nc)
    assert infer_arch(sd) == (scale, "classify", nc)
    g = GraphBuilder(scale, "classify", nc=nc)
    shapes = {p.name: (tuple(p.shape), p.kind) for p in g.params}
    assert shapes["model.10.conv.conv.weight"] == ((1280, c1, 1, 1), "conv_w")
    assert shapes["model.10.conv.bn.running_var"] == ((1280,), "bn_var")
    assert shapes["model.10.linear.weight"] == ((nc, 1280), "linear_w")
    assert shapes["model.10.linear.bias"] == ((nc,), "linear_b")
    assert set(shapes) == set(sd) and all(tuple(np.shape(sd[k])) == v[0] for k, v in shapes.items())
    assert sorted(g.layers) == list(range(10)) and g.layers[9][0].C == c1
    assert [op.kind for op in g.ops][-1] == "classify" and not any(op.kind in ("sppf", "decode", "nms") for op in g.ops)


def test_other_dicts_keep_their_answers():
    assert GraphBuilder("n", "classify").nc == 1000
    assert infer_arch(synth_weights("n", "detect", 0)) == ("n", "detect", 80)
    with pytest.raises(ValueError, match="not a YOLO11 detect/segment state dict"):
        infer_arch({"model.0.conv.weight": np.zeros((16, 3, 3, 3), np.float32)})
    from yolomi.plan import pack_graph
    with pytest.raises(ValueError, match="classify"):
        GraphBuilder("n", "classify", quant=True)
    with pytest.raises(ValueError, match="classify"):
        g = GraphBuilder("n", "classify", nc=3)
        g.quant = True
        pack_graph(g, synth_weights("n", "classify", 0, nc=3), "i8", {"backend": "qnnpack"})


def test_bare_classify_task_still_refuses():
    from core.model import YOLO11Model
    with pytest.raises(NotImplementedError, match="pass model_path"):
        YOLO11Model(task="classify", device="cuda")


@pytest.mark.parametrize("scale,nc,H,W,B", CASES, ids=[f"{c[0]}-nc{c[1]}-{c[2]}x{c[3]}" for c in CASES])
def test_synthetic_softmax_is_neither_flat_nor_saturated(scale, nc, H, W, B):
    """Float64 logits of the GPU tests' images: standard deviation of order 1 across classes, top-1 probability in
    (2 / nc, 0.99) (nc = 2: 2 / nc is 1, which no probability exceeds, so the lower bound there is 1 / nc), the five
    best logits at least 1e-3 of the logit spread apart."""
    logits, _ = CO.build_cls(scale, synth_weights(scale, "classify", 0, nc=nc), nc, torch.float64)(
        CO.cls_input(B, H, W).double())
    top1 = torch.softmax(logits, 1).max(1).values
    best = torch.sort(logits, 1, descending=True).values[:, :min(5, nc)]
    gap = (best[:, :-1] - best[:, 1:]).min(1).values / (logits.max(1).values - logits.min(1).values)
    print(f"std {logits.std(1).tolist()} top1 {top1.tolist()} gap / spread {gap.tolist()}")
    assert bool(((logits.std(1) > 0.3) & (logits.std(1) < 3.0)).all())
    assert bool(((top1 > (2.0 / nc if nc > 2 else 1.0 / nc)) & (top1 < 0.99)).all())
    assert bool((gap >= 1e-3).all())


@pytest.mark.parametrize("h,w", [(120, 90), (300, 500)])
def test_image_transform_geometry(h, w):
    from PIL import Image
    from yolomi.preprocess import classify_batch
    bgr = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    short, long_ = min(h, w), max(h, w)
    rl = int(224 * long_ / short)
    rh, rw = (224, rl) if h <= w else (rl, 224)
    top, left = int(round((rh - 224) / 2.0)), int(round((rw - 224) / 2.0))
    pil = Image.fromarray(bgr[..., ::-1].copy()).resize((rw, rh), Image.BILINEAR).crop((left, top, left + 224, top + 224))
    want = torch.from_numpy(np.asarray(pil).copy()).permute(2, 0, 1).float() / 255
    got = classify_batch([bgr], 224)
    assert got.shape == (1, 3, 224, 224) and torch.equal(got[0], want)
