"""Fixture F26: gradients of the reference's own attention layers under torch autograd on the CPU.

The reference's outlier_rejection.geometry_attention.CorrespondenceAttentionLayer (with the compatibility of its pipeline) and
lepard.transformer.GeometryAttentionLayer import with its `correspondence` directory on sys.path and run with plain torch.  Numbers
only are recorded -- inputs, codes, state dicts (model weights are data) and gradients -- nothing of the reference's program text.
Run once where the reference is present:

    python tests/golden/make_golden_attention_grad.py

Keys of tests/golden/F26_attention_grad.npz, <kind> = outlier (L = S = 33, the rows of both sides at one pair's matches) or lepard ((L, S) =
(17, 33)), both C = 48, H = 4 with rotary codes:
  <kind>.x / source / x_pe / source_pe / w       the inputs, the codes [rows, C, 2] the reference's position encoding gave, the weights
  outlier.vec6d                                   of the sum; the correspondences behind the outlier layer's codes and compatibility
  <kind>.sd.<name>                               the layer's state dict (LayerNorm weights drawn, the first MLP weight times 8)
  <kind>.out64 / pre64                           the double output and the MLP's pre-ReLU values
  <kind>.grad64.<name> / grad32.<name>           d(sum w out) in x, source and every parameter, double and float32
The inputs are reseeded until every double pre-ReLU value is at least 2e-3 away from 0 (tests assert 1e-3)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import _lepard_ref as P  # noqa: E402
from tests import _outlier_ref as O  # noqa: E402

REF = "/root/reference/correspondence"
C, H = 48, 4


def main():
    tmp = tempfile.mkdtemp()
    assert not os.path.abspath(tmp).startswith(ROOT)
    os.chdir(tmp)
    sys.path.insert(0, REF)
    import torch
    from lepard.position_encoding import VolumetricPositionEncoding as LepardPE
    from lepard.transformer import GeometryAttentionLayer
    from outlier_rejection.geometry_attention import CorrespondenceAttentionLayer
    from outlier_rejection.position_encoding import VolumetricPositionEncoding as OutlierPE

    torch.set_num_threads(8)
    T = torch.from_numpy
    out = {}
    for kind in ("outlier", "lepard"):
        for seed in range(100):
            g = np.random.default_rng(2600 + seed)
            torch.manual_seed(2600 + seed)
            if kind == "outlier":
                L = S = 33
                cfg = O.config(C, H)
                layer = CorrespondenceAttentionLayer(cfg)
                vec6d = O.matches(L, 2600 + seed)
                with torch.no_grad():
                    x_pe = s_pe = OutlierPE(cfg)(T(vec6d)[None])[0].numpy()
            else:
                L, S = 17, 33
                cfg = P.transformer_config(C, H)
                layer = GeometryAttentionLayer(cfg)
                xpts, spts = (g.uniform(-1, 1, (n, 3)).astype(np.float32) for n in (L, S))
                with torch.no_grad():
                    x_pe, s_pe = (LepardPE(cfg)(T(p)[None])[0].numpy() for p in (xpts, spts))
            for m in layer.modules():
                if isinstance(m, torch.nn.LayerNorm):
                    m.weight.data = 1 + 0.2 * torch.randn(m.weight.shape)
                    m.bias.data = 0.2 * torch.randn(m.bias.shape)
            layer.mlp[0].weight.data *= 8
            x = g.standard_normal((L, C)).astype(np.float32)
            source = g.standard_normal((S, C)).astype(np.float32)
            w = g.standard_normal((L, C)).astype(np.float32)
            sd = {k: v.numpy().copy() for k, v in layer.state_dict().items()}
            rec = {}
            for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
                lay = type(layer)(cfg).to(dt)
                lay.load_state_dict({k: T(v).to(dt) for k, v in sd.items()})
                pre = []
                lay.mlp[0].register_forward_hook(lambda mod, args, res: pre.append(res.detach().clone()))
                xt, st = T(x).to(dt)[None].requires_grad_(True), T(source).to(dt)[None].requires_grad_(True)
                args = [xt, st, T(x_pe).to(dt)[None], T(s_pe).to(dt)[None]]
                if kind == "outlier":                                   # the pipeline's compatibility of the correspondences, in dt
                    v6 = T(vec6d).to(dt)[None]
                    ds = torch.norm(v6[:, :, None, :3] - v6[:, None, :, :3], dim=-1)
                    dtg = torch.norm(v6[:, :, None, 3:] - v6[:, None, :, 3:], dim=-1)
                    comp = torch.clamp(1.0 - (ds - dtg) ** 2 / cfg["sigma_spat"] ** 2, min=0)
                    res = lay(*args, None, None, comp)
                else:
                    res = lay(*args)
                (res[0] * T(w).to(dt)).sum().backward()
                rec[f"grad{tag}.x"], rec[f"grad{tag}.source"] = xt.grad[0].numpy(), st.grad[0].numpy()
                rec.update({f"grad{tag}.{k}": p.grad.numpy() for k, p in lay.named_parameters()})
                if tag == "64":
                    rec["out64"], rec["pre64"] = res[0].detach().numpy(), pre[0][0].numpy()
            gap = float(np.abs(rec["pre64"]).min())
            print(kind, "seed", seed, "smallest |pre-ReLU|", gap, flush=True)
            if gap >= 2e-3:
                break
        assert gap >= 2e-3, f"{kind}: no seed kept the pre-ReLU values away from 0"
        rec.update({"x": x, "source": source, "x_pe": x_pe, "source_pe": s_pe, "w": w})
        if kind == "outlier":
            rec["vec6d"] = vec6d
        rec.update({"sd." + k: v for k, v in sd.items()})
        out.update({f"{kind}.{k}": v for k, v in rec.items()})
    path = os.path.join(HERE, "F26_attention_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
