"""Sinkhorn (optimal-transport) baseline on the HIP path.

    run_optimal_transport(reg)        upstream model/registration.py:543-572

Upstream's loop is eleven Euler steps on the gradient of geomloss.SamplesLoss("sinkhorn", p=2, blur, reach).  The library is
not a dependency here: its arithmetic (tensorized backend, debiased, scaling 0.5, uniform weights) is restated in DESIGN.md
"Sinkhorn baseline" and runs in libndp_hip.so (`ndp_sinkhorn_divergence`: a streamed online log-sum-exp per Sinkhorn step,
csrc/ndp_sinkhorn.inc).  Parity with the library itself is unverified; the kernels are held to a float64 restatement of the same
definition.  The loop is host driven like upstream's, one diameter read per loss call.  No CPU fallback.
"""
import math

import torch

from . import ops


def epsilon_schedule(diameter, blur, scaling):
    """[diameter^2] + [exp(e) for e in arange(2 ln diameter, 2 ln blur, 2 ln scaling)] + [blur^2] in Python doubles, numpy's arange
    (count = ceil((stop - start) / step), none when diameter <= blur): what ndp_sinkhorn_schedule computes."""
    if not (diameter > 0 and math.isfinite(diameter) and blur > 0 and math.isfinite(blur) and 0 < scaling < 1):
        raise ValueError("epsilon_schedule: diameter and blur must be positive and finite, 0 < scaling < 1")
    start, stop, step = 2.0 * math.log(diameter), 2.0 * math.log(blur), 2.0 * math.log(scaling)
    count = max(0, math.ceil((stop - start) / step))
    return [diameter * diameter] + [math.exp(start + i * step) for i in range(count)] + [blur * blur]


def run_optimal_transport(reg, visualize=False):
    """registration.py:551-572, same order of operations: no centring, two CPU randperms, the first `samples` of each, Nsteps
    Euler steps x -= lr * len(x) * g.  Returns (x_i, select_ind): the moved source samples and their indices in the source."""
    if visualize:
        raise NotImplementedError("mayavi visualisation is outside the hot path")
    config = reg.config
    dev = reg._dev()
    reg.src_pcd = reg.src_pcd.to(dev).float()
    tgt_pcd = reg.tgt_pcd.to(dev).float()
    src = torch.randperm(reg.src_pcd.shape[0])                                  # :554-555 (CPU RNG)
    tgt = torch.randperm(tgt_pcd.shape[0])
    select_ind = src[: config.samples].to(dev)                                  # :558-559
    x_i = reg.src_pcd[select_ind].contiguous()
    y_j = tgt_pcd[tgt[: config.samples].to(dev)].contiguous()
    reach = getattr(config, "reach", None)
    loss = None
    for _ in range(config.Nsteps):                                              # :564-569
        loss, g, _ = ops.sinkhorn_divergence(x_i, y_j, config.blur, reach)
        x_i = x_i - (config.lr * len(x_i)) * g
    reg.last_sinkhorn = dict(steps=int(config.Nsteps), loss=loss)
    return x_i, select_ind
