"""Fixture F21: the reference's coarse matcher on seeded inputs.

Imports /root/reference/correspondence/lepard/matching.py (with correspondence/ on sys.path; it needs only torch), builds
Matching(config) with entangled=True (no positional embedding: src_pe = tgt_pe = None), runs its forward in float32 and in float64
and records numbers only; nothing of the reference's source text is written anywhere.  Run once where the reference is present:

    python tests/golden/make_golden_matching.py

Keys of tests/golden/F21_matching.npz, per case <c> in (dsm, skh):
  <c>.src_feats, <c>.tgt_feats   data["src_feats"], data["tgt_feats"]: the projected features, float32 -- this project's inputs
  <c>.src_mask, <c>.tgt_mask     the bool masks handed to forward
  <c>.conf_matrix                float32 conf_matrix of the float32 run
  <c>.conf_matrix64              float64 conf_matrix of the same module in double ON THE RECORDED float32 FEATURES (the projection is
                                 skipped by making it the identity), the yardstick of the float32 run's own error
  <c>.coarse_match               int64 [M,3] rows (b, s, t) of the float32 run
  <c>.config                     confidence_threshold, dsmax_temperature | skh_init_bin_score, skh_iters
dsm: dual_softmax, B = 2, C = 48, valid sizes (37, 29) and (30, 20) inside a 37 x 29 padding.
skh: sinkhorn, B = 2, C = 32, 24 x 20, all-true masks.
Half of the target rows are noisy copies of source rows; the script asserts at least 10 matches per case."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/correspondence"


def planted(B, S, T, C, sizes, scale, g):
    x = torch.randn(B, S, C, generator=g)
    y = torch.randn(B, T, C, generator=g)
    for b, (s, t) in enumerate(sizes):
        k = t // 2
        ps, pt = torch.randperm(s, generator=g)[:k], torch.randperm(t, generator=g)[:k]
        y[b, pt] = x[b, ps] + 0.2 * torch.randn(k, C, generator=g)
    sm, tm = torch.zeros(B, S, dtype=torch.bool), torch.zeros(B, T, dtype=torch.bool)
    for b, (s, t) in enumerate(sizes):
        sm[b, :s] = True
        tm[b, :t] = True
    return x * scale, y * scale, sm, tm


def run(Matching, config, x, y, sm, tm, seed):
    torch.manual_seed(seed)
    m = Matching(config)
    data = {}
    with torch.no_grad():
        conf, match = m(x, y, None, None, sm, tm, data)
        fs, ft = data["src_feats"].clone(), data["tgt_feats"].clone()
        m64 = m.double()
        m64.src_proj.weight.copy_(torch.eye(x.shape[2], dtype=torch.float64))
        conf64, _ = m64(fs.double(), ft.double(), None, None, sm, tm, {})
    assert match.shape[0] >= 10, match.shape
    return {"src_feats": fs.numpy(), "tgt_feats": ft.numpy(), "src_mask": sm.numpy(), "tgt_mask": tm.numpy(),
            "conf_matrix": conf.numpy(), "conf_matrix64": conf64.numpy(), "coarse_match": match.numpy()}


def main():
    sys.path.insert(0, REF)
    from lepard.matching import Matching
    g = torch.Generator().manual_seed(21)
    out = {}
    cfg = {"match_type": "dual_softmax", "confidence_threshold": 0.1, "feature_dim": 48, "entangled": True, "dsmax_temperature": 0.1}
    c = run(Matching, cfg, *planted(2, 37, 29, 48, [(37, 29), (30, 20)], 2.0, g), seed=1)
    c["config"] = np.array([cfg["confidence_threshold"], cfg["dsmax_temperature"]])
    out.update({"dsm." + k: v for k, v in c.items()})
    cfg = {"match_type": "sinkhorn", "confidence_threshold": 0.1, "feature_dim": 32, "entangled": True, "skh_init_bin_score": 1.0,
           "skh_iters": 3, "skh_prefilter": False}
    c = run(Matching, cfg, *planted(2, 24, 20, 32, [(24, 20), (24, 20)], 4.0, g), seed=2)
    c["config"] = np.array([cfg["confidence_threshold"], cfg["skh_init_bin_score"], cfg["skh_iters"]])
    out.update({"skh." + k: v for k, v in c.items()})
    path = os.path.join(HERE, "F21_matching.npz")
    np.savez_compressed(path, **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype)
    print("dsm matches", out["dsm.coarse_match"].shape[0], "skh matches", out["skh.coarse_match"].shape[0], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
