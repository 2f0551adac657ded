"""What the GPU tests of the training ops share (test_gpu_attn_bwd.py, test_gpu_linear_bwd.py, test_gpu_layer_train.py,
test_gpu_mlp_train.py, test_gpu_conv_train.py): the error pairs against fp64 and the `<= 2 x torch` yardstick, the parity-JSON record
of a run, bit comparison, the 2-layer encoder and the gradients of an encoder.  TEST INFRASTRUCTURE; where the files differed in a
detail, the detail is a parameter.  Their CPU-side counterpart is tests/train_cpu.py."""
import json
import os

import pytest
import torch
import torch.nn as nn


def errs(got, ref):
    """(max, mean) absolute error of `got` against the fp64 `ref`"""
    e = (got.double() - ref).abs()
    return float(e.max()), float(e.mean())


def pooled(parts):
    """(max, mean) over a list of error tensors"""
    e = torch.cat([p.reshape(-1) for p in parts])
    return float(e.max()), float(e.mean())


class Parity:
    """The (ours, torch) error pairs a test module measures.  `fixture()` is the module's autouse fixture that writes them, with the
    device, torch's version and `note`, to the path in the environment variable `env` when that is set."""

    def __init__(self, env, note=None):
        self.env, self.note, self.pairs = env, note, []

    def record(self, case, what, ours, torchs):
        self.pairs.append({"case": case, "what": what, "max": ours[0], "mean": ours[1], "torch_max": torchs[0], "torch_mean": torchs[1]})
        print(f"{case} {what}: max {ours[0]:.3e} (torch {torchs[0]:.3e})  mean {ours[1]:.3e} (torch {torchs[1]:.3e})")

    def within_2x(self, case, what, ours, torchs):
        self.record(case, what, ours, torchs)
        assert ours[0] <= 2 * torchs[0] and ours[1] <= 2 * torchs[1], (case, what, ours, torchs)

    def write(self, pairs=None):
        path = os.environ.get(self.env)
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
            head = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}
            if self.note is not None:
                head["note"] = self.note
            with open(path, "w") as f:
                json.dump({**head, "pairs": self.pairs if pairs is None else pairs}, f, indent=1)

    def fixture(self):
        @pytest.fixture(scope="module", autouse=True)
        def _parity_json():
            yield
            self.write()
        return _parity_json


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b, typed=True):
    """the same bits; typed: and the same dtype and shape"""
    return (not typed or (a.dtype == b.dtype and a.shape == b.shape)) and torch.equal(bits(a), bits(b))


def encoder(dropout, seed, jitter_norms=False):
    """nn.TransformerEncoder of 2 norm-first layers (768, 12 heads, d_ff 1024) and a final LayerNorm on the device, in training mode, seeded.
    jitter_norms: the LayerNorms' weight and bias moved off 1 / 0 by N(0, 0.1^2)."""
    torch.manual_seed(seed)
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(768, 12, 1024, dropout=dropout, norm_first=True), 2, nn.LayerNorm(768),
                                enable_nested_tensor=False).cuda()
    if jitter_norms:
        with torch.no_grad():
            for m in enc.modules():
                if isinstance(m, nn.LayerNorm):
                    m.weight.add_(0.1 * torch.randn_like(m.weight)), m.bias.add_(0.1 * torch.randn_like(m.bias))
    return enc


def encoder_grads(enc, x, mask, g, scale=1.0, dtype=None, fp64=True):
    """(out, {parameter name: gradient / scale}) of the loss sum(out * g) * scale.  dtype: the autocast dtype; None = no autocast, x
    in the encoder's own dtype.  fp64: the product out * g and the returned gradients in fp64; otherwise as torch leaves them."""
    enc.zero_grad(set_to_none=True)
    if dtype is None:
        out = enc(x.to(next(enc.parameters()).dtype), src_key_padding_mask=mask)
    else:
        with torch.autocast("cuda", dtype=dtype):
            out = enc(x, src_key_padding_mask=mask)
    ((out.double() * g).sum() * scale if fp64 else (out * g).sum()).backward()
    return out.detach(), {k: (p.grad.double() / scale if fp64 else p.grad.clone()) for k, p in enc.named_parameters()}
