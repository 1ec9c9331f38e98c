"""Plain-torch restatement of the Sinkhorn divergence the HIP kernels compute (DESIGN.md "Sinkhorn baseline"), on the CPU in
float64 -- the yardstick of tests/test_sinkhorn.py -- or in float32 -- the eager arithmetic the kernels' error is measured against.

Written from the published algorithm of geomloss.SamplesLoss("sinkhorn", p=2, debias=True, scaling) on its tensorized backend with
uniform weights; the library itself is not available, so parity with it is unverified.  Nothing here imports the package."""
import math
from types import SimpleNamespace

import numpy as np
import torch


def diameter(x, y):
    """Norm of the extent of the joint bounding box, in double whatever the clouds' dtype (one host read)."""
    lo = torch.minimum(x.min(dim=0).values, y.min(dim=0).values).double()
    hi = torch.maximum(x.max(dim=0).values, y.max(dim=0).values).double()
    return float((hi - lo).norm())


def schedule(diam, blur, scaling):
    mid = np.arange(2 * math.log(diam), 2 * math.log(blur), 2 * math.log(scaling))
    return [diam ** 2] + [float(math.exp(e)) for e in mid] + [blur ** 2]


def cost(u, v):
    return ((u[:, None, :] - v[None, :, :]) ** 2).sum(-1) / 2


def softmin(eps, C, h):
    return -eps * torch.logsumexp(h[None, :] - C / eps, dim=1)


def loss_of(F_ba, F_aa, G_ab, G_bb, eps, rho):
    if rho is None:
        return (F_ba - F_aa).mean() + (G_ab - G_bb).mean()
    return (rho + eps / 2) * ((torch.exp(-F_aa / rho) - torch.exp(-F_ba / rho)).mean() + (torch.exp(-G_bb / rho) - torch.exp(-G_ab / rho)).mean())


def sinkhorn_ref(x, y, blur, reach=None, scaling=0.5, dtype=torch.float64, device="cpu"):
    """-> namespace(loss, grad [n,3], potentials (F_ba, F_aa, G_ab, G_bb), duals (f_ba, f_aa, g_ab, g_bb), eps, damp, rho, backward_scale)."""
    diam = diameter(x, y)
    x, y = x.to(device=device, dtype=dtype), y.to(device=device, dtype=dtype)
    n, m = x.shape[0], y.shape[0]
    a_log = torch.full((n,), -math.log(n), dtype=dtype, device=device)
    b_log = torch.full((m,), -math.log(m), dtype=dtype, device=device)
    rho = None if reach is None else reach ** 2
    damp = lambda e: 1.0 if rho is None else 1.0 / (1.0 + e / rho)
    C_xy, C_xx, C_yy = cost(x, y), cost(x, x), cost(y, y)
    C_yx = C_xy.t()
    eps_list = schedule(diam, blur, scaling)
    eps = eps_list[0]
    d = damp(eps)
    g_ab, f_ba = d * softmin(eps, C_yx, a_log), d * softmin(eps, C_xy, b_log)
    f_aa, g_bb = d * softmin(eps, C_xx, a_log), d * softmin(eps, C_yy, b_log)
    for eps in eps_list:
        d = damp(eps)
        ft_ba = d * softmin(eps, C_xy, b_log + g_ab / eps)
        gt_ab = d * softmin(eps, C_yx, a_log + f_ba / eps)
        ft_aa = d * softmin(eps, C_xx, a_log + f_aa / eps)
        gt_bb = d * softmin(eps, C_yy, b_log + g_bb / eps)
        f_ba, g_ab, f_aa, g_bb = (f_ba + ft_ba) / 2, (g_ab + gt_ab) / 2, (f_aa + ft_aa) / 2, (g_bb + gt_bb) / 2
    h_xy, h_xx = b_log + g_ab / eps, a_log + f_aa / eps
    F_ba, F_aa = d * softmin(eps, C_xy, h_xy), d * softmin(eps, C_xx, h_xx)
    G_ab, G_bb = d * softmin(eps, C_yx, a_log + f_ba / eps), d * softmin(eps, C_yy, b_log + g_bb / eps)
    loss = loss_of(F_ba, F_aa, G_ab, G_bb, eps, rho)
    W_xy = torch.softmax(h_xy[None, :] - C_xy / eps, dim=1)
    W_xx = torch.softmax(h_xx[None, :] - C_xx / eps, dim=1)
    dF_ba, dF_aa = d * (x - W_xy @ y), d * (x - W_xx @ x)
    if rho is None:
        grad, bscale = (dF_ba - dF_aa) / n, 1.0
    else:
        grad = (1 + eps / rho) / n * (torch.exp(-F_ba / rho)[:, None] * dF_ba - torch.exp(-F_aa / rho)[:, None] * dF_aa)
        bscale = (rho + eps) / (rho + eps / 2)                     # the backward weight is rho + eps, the forward's rho + eps / 2
    return SimpleNamespace(loss=loss, grad=grad, potentials=(F_ba, F_aa, G_ab, G_bb), duals=(f_ba, f_aa, g_ab, g_bb), eps=eps, damp=d,
                           rho=rho, backward_scale=bscale, n_eps=len(eps_list))


def extrapolation_loss(x, y, r):
    """The loss as a differentiable function of x through the extrapolation's two x-row softmins only (second arguments and duals detached)."""
    n, m = x.shape[0], y.shape[0]
    f_ba, f_aa, g_ab, g_bb = [t.detach() for t in r.duals]
    xd, yd = x.detach(), y.detach()
    F_ba = r.damp * softmin(r.eps, cost(x, yd), -math.log(m) + g_ab / r.eps)
    F_aa = r.damp * softmin(r.eps, cost(x, xd), -math.log(n) + f_aa / r.eps)
    return loss_of(F_ba, F_aa, r.potentials[2].detach(), r.potentials[3].detach(), r.eps, r.rho)


def euler(x, y, blur, reach, nsteps, lr, dtype=torch.float64):
    """registration.py:564-569 on the restatement: nsteps times x -= lr * len(x) * grad."""
    x, y = x.to(dtype), y.to(dtype)
    for _ in range(nsteps):
        x = x - lr * len(x) * sinkhorn_ref(x, y, blur, reach, dtype=dtype).grad
    return x


def box_clouds(n, m, seed):
    """The accuracy cases' inputs: uniform in a 1 x 0.8 x 0.6 box, y offset by 0.15 (float32)."""
    g = torch.Generator().manual_seed(seed)
    box = torch.tensor([1.0, 0.8, 0.6])
    return torch.rand(n, 3, generator=g) * box, torch.rand(m, 3, generator=g) * box + 0.15
