"""Fixture F27: the gradients of the reference's own lepard.blocks.KPConv and of its resnetb_strided block under torch autograd on the
CPU, in float32 and in double, on the batch and the weights of fixture F23.

The reference's modules import with its `correspondence` directory on sys.path and run with a temporary directory OUTSIDE the
repository as the working directory (the reference writes its kernel-point cache into ./kernels/dispositions), as in
make_golden_kpfcn.py.  Numbers only are recorded -- inputs, weights, dy and gradients -- nothing of the reference's program text.  Run
once where the reference is present:

    python tests/golden/make_golden_kpconv_grad.py

Keys of tests/golden/F27_kpconv_grad.npz (the tables and points are F23's and are not repeated):
  a<i>.x, a<i>.weights, a<i>.kernel_points, a<i>.dy                  the three bare KPConv calls of _kpfcn_ref.F23_CONVS, 8 -> 8 channels
  a<i>.dx32 / dx64, a<i>.dW32 / dW64                                 d sum(y dy) / dx and / dweights: the float32 and the double run
  b2.sd.<name>, b2.x, b2.dy                                          the resnetb_strided block (16 -> 32) of F23, its input and dy
  b2.grad32.<name> / b2.grad64.<name>                                the gradient in every parameter and in x ("x")
x and dy hold float16 values (stored as float16, exact in float32); the double run takes the same float32 numbers."""
import copy
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import _kpfcn_ref as K  # noqa: E402

REF = "/root/reference/correspondence"


def main():
    tmp = tempfile.mkdtemp()
    assert not os.path.abspath(tmp).startswith(ROOT)
    os.chdir(tmp)
    sys.path.insert(0, REF)
    import torch
    from lepard import blocks as B

    torch.set_num_threads(8)
    cfg = SimpleNamespace(**K.F23_CONFIG)
    batch, f23 = K.load_f23()
    r0 = cfg.first_subsampling_dl * cfg.conv_radius

    def batch_of(dtype):
        b = {"points": [torch.from_numpy(p).to(dtype) for p in batch["points"]]}
        for key in ("neighbors", "pools", "upsamples"):
            b[key] = [torch.from_numpy(t.astype(np.int64)) for t in batch[key]]
        return b

    b32, b64 = batch_of(torch.float32), batch_of(torch.float64)
    g = torch.Generator().manual_seed(27)
    out = {}
    x8 = torch.from_numpy(f23["x8"].astype(np.float32))
    for i, (influence, aggregation, strided) in enumerate(K.F23_CONVS):
        conv = B.KPConv(cfg.num_kernel_points, 3, 8, 8, r0 * cfg.KP_extent / cfg.conv_radius, r0, fixed_kernel_points="center",
                        KP_influence=influence, aggregation_mode=aggregation)
        with torch.no_grad():
            conv.weights.copy_(torch.from_numpy(f23[f"a{i}.weights"]))
            conv.kernel_points.copy_(torch.from_numpy(f23[f"a{i}.kernel_points"]))
        tabs = lambda b: (b["points"][1], b["points"][0], b["pools"][0]) if strided else (b["points"][0], b["points"][0], b["neighbors"][0])
        nq = tabs(b32)[0].shape[0]
        dy = torch.randn(nq, 8, generator=g).half()
        out.update({f"a{i}.x": x8.half().numpy(), f"a{i}.weights": conv.weights.detach().numpy().copy(),
                    f"a{i}.kernel_points": conv.kernel_points.detach().numpy().copy(), f"a{i}.dy": dy.numpy()})
        for tag, module, b, dt in (("32", conv, b32, torch.float32), ("64", copy.deepcopy(conv).double(), b64, torch.float64)):
            x = x8.detach().clone().to(dt).requires_grad_(True)
            module.weights.grad = None
            y = module(*tabs(b), x)
            (y * dy.to(dt)).sum().backward()
            out[f"a{i}.dx{tag}"], out[f"a{i}.dW{tag}"] = x.grad.numpy().copy(), module.weights.grad.numpy().copy()
            if tag == "32":
                assert np.abs(y.detach().numpy() - f23[f"a{i}.out"]).max() == 0                    # the forward F23 recorded
    name, cin, cout = K.F23_BLOCKS[2]
    assert name == "resnetb_strided"
    block = B.block_decider(name, r0, cin, cout, 0, cfg)
    block.load_state_dict({k[len("b2.sd."):]: torch.from_numpy(f23[k]) for k in f23.files if k.startswith("b2.sd.")}, strict=True)
    x16 = torch.from_numpy(f23["x16"].astype(np.float32))
    dy = torch.randn(b32["points"][1].shape[0], cout, generator=g).half()
    out.update({"b2.x": x16.half().numpy(), "b2.dy": dy.numpy()})
    out.update({f"b2.sd.{k}": v.numpy().copy() for k, v in block.state_dict().items()})
    for tag, module, b, dt in (("32", block, b32, torch.float32), ("64", copy.deepcopy(block).double(), b64, torch.float64)):
        x = x16.detach().clone().to(dt).requires_grad_(True)
        y = module(x, b)
        (y * dy.to(dt)).sum().backward()
        out[f"b2.grad{tag}.x"] = x.grad.numpy().copy()
        for k, p in module.named_parameters():
            if p.requires_grad:
                out[f"b2.grad{tag}.{k}"] = p.grad.numpy().copy()
        if tag == "32":
            assert np.abs(y.detach().numpy() - f23["b2.out"]).max() == 0
    path = os.path.join(HERE, "F27_kpconv_grad.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items() if "grad64" in k or k.endswith("64")})
    print(os.path.getsize(path), "bytes; F23:", os.path.getsize(K.F23))
    assert os.path.getsize(path) <= os.path.getsize(K.F23)


if __name__ == "__main__":
    main()
