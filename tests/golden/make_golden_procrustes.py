"""Fixture F20: the reference's weighted Procrustes on seeded inputs.

Imports /root/reference/correspondence/lepard/procrustes.py (it needs only torch), calls
SoftProcrustesLayer.batch_weighted_procrustes and records the inputs and its outputs -- numbers only; nothing of the reference's
source text is written anywhere.  Run once where the reference is present:
    python tests/golden/make_golden_procrustes.py
B = 4 problems of N = 257 correspondences with random positive weights:
  0  a rigid motion plus noise;
  1  the same kind with a quarter of the weights zero;
  2  a mirrored target: the best orthogonal fit is a reflection, det U det V = -1, and R flips the weakest direction;
  3  a nearly planar cloud (the third axis scaled by 0.02).
The clouds are anisotropic (axes scaled 1, 0.7, 0.4) so that the singular values are well separated and the fit well posed."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _rigid_ref as R  # noqa: E402

REF = "/root/reference/correspondence/lepard/procrustes.py"


def inputs():
    g = torch.Generator().manual_seed(20)
    B, n = 4, 257
    scale = torch.tensor([[1.0, 0.7, 0.4]] * 3 + [[1.0, 0.7, 0.02]])
    X = (torch.rand(B, n, 3, generator=g) - 0.5) * scale[:, None, :]
    Y = torch.empty_like(X)
    for b in range(B):
        rot = R.rotation((0.2 + 0.3 * b, 1.0 - 0.4 * b, 0.5), 0.4 + 0.5 * b).float()
        Y[b] = X[b] @ rot.T + torch.tensor([0.1 * b, -0.2, 0.05 * b]) + 0.01 * (torch.rand(n, 3, generator=g) - 0.5)
    Y[2, :, 2] = -Y[2, :, 2]                                       # mirrored
    w = torch.rand(B, n, 1, generator=g) + 0.05
    w[1, torch.randperm(n, generator=g)[: n // 4]] = 0.0
    return X.contiguous(), Y.contiguous(), w.contiguous()


def main():
    spec = importlib.util.spec_from_file_location("ref_procrustes", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    X, Y, w = inputs()
    Rm, t, cond = mod.SoftProcrustesLayer.batch_weighted_procrustes(X, Y, w)
    out = os.path.join(HERE, "F20_procrustes.npz")
    np.savez_compressed(out, X=X.numpy(), Y=Y.numpy(), w=w.numpy(), R=Rm.numpy(), t=t.numpy(), condition=cond.numpy())
    print("wrote", out, "det R =", torch.linalg.det(Rm.double()).tolist(), "condition =", cond.tolist())


if __name__ == "__main__":
    main()
